#!/usr/bin/env python3
"""CPU model of the coarse Newton steps of the tuned mel-cepstral forward (csrc/mcep_mfma_f16.h).

    python tools/proto/proto_coarse_steps.py [--utterances 32]

No GPU: numpy and torch on the CPU, nothing read outside the repository.  The iteration is the kernel's, in the arithmetic of
oracle/torch_port.py with the composed matrices (utils/tables.py: mc0 = log X G, t = log2 X - 2 log2(e) mc D, rt = exp2(t) E), a
float32 solve of (Toeplitz + Hankel) x = r - alpha_vec per frame, the kernel's stopping rule (u <= 2^-20, or u <= 2^-16 and
16 u <= u_prev; the stopping step's update applied) and tiles of 16 frames, which leave the loop when their last frame has stopped.
A COARSE step rounds both operands of both chains to binary16 (11 significant bits) at the kernel's scales -- mc 2^10, D 2^4,
E 2^16, e shifted so that the frame's largest value is in (2^14, 2^15], binary16 subnormals below 2^-14 -- and accumulates in
float32: what one v_mfma_f32_16x16x32_f16 per chain computes.  The Nyquist bin and the rt[48] column stay float32, as in the kernel,
and so does the rounding residual of the gain term mc[0] D[0][.], which is constant over the bins and travels with the exponent shift.
No frame stops on a coarse step, and u_prev = 0 behind it.

Printed, for the bench input (seeded randn), the speech recording of tests/golden tiled as bench.py tiles it, the same noise 60 dB
down, and two sines over a -80 dB noise floor (the slow convergers):
  * steps per tile (mean and histogram) with no coarse step, against the kernel's measured profiles/r09_quadratic_stop_steps.txt;
  * steps 1 - 2 coarse with early stop: tile steps, frames that stop one step later, and the largest deviation from the all-full
    result as a fraction of the tolerance 5e-6 + 1e-4 |y|;
  * fixed step counts, steps 1 - 2 coarse (and step 1 alone) against the same count all-full;
  * a third coarse step, for the record of why it was left out."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from diffsptk_amd.utils import tables   # noqa: E402
from oracle import torch_port as TP    # noqa: E402

M, H, NFFT, ALPHA = 24, 256, 512, 0.42
SD, SM, SE, EMAX = 16.0, 1024.0, 65536.0, 15
TAU, FACTOR = 2.0 ** -20, 16.0
F32 = torch.float32


def h16(v, scale):
    """v at `scale` rounded to binary16 (round to nearest even, subnormals kept), back at its own scale"""
    return (v * scale).half().float() / scale


class Model:
    def __init__(self, gain_residual=True):
        self.gain_residual = gain_residual
        G, D, E, av, *_ = tables.mcep_matrices(NFFT, M, ALPHA)
        self.G = torch.from_numpy(G).to(F32)
        self.Dk = torch.from_numpy(-2.0 * np.log2(np.e) * D).to(F32)      # t = log2 X + mc Dk
        self.E = torch.from_numpy(E).to(F32)
        self.av = torch.from_numpy(av).to(F32)
        self.Dk_h, self.E_h = h16(self.Dk, SD), h16(self.E, SE)
        i = torch.arange(M + 1)
        self.toep, self.hank = (i[:, None] - i[None, :]).abs(), i[:, None] + i[None, :]

    def step(self, logx2, mc, coarse):
        if coarse:
            mh = h16(mc, SM)
            # row 0 of D is constant over the bins: what mc[0] and that row lose in binary16 is one number per frame (a factor on every e),
            # which the kernel forms in float32 and adds with the exponent shift (--no-gain-residual: left out, as first built)
            gres = mc[:, :1] * self.Dk[0, 0] - mh[:, :1] * self.Dk_h[0, 0] if self.gain_residual else 0.0
            t = logx2 + mh @ self.Dk_h + gres
            t[:, H] = logx2[:, H] + mc @ self.Dk[:, H]                      # the Nyquist bin: float32 on the vector unit
        else:
            t = logx2 + mc @ self.Dk
        mi = torch.ceil(t.amax(-1, keepdim=True))
        e = torch.exp2(t + (EMAX - mi))                                     # largest value in (2^14, 2^15]
        rt = e @ self.E
        if coarse:
            rt[:, :48] = e[:, :H].half().float() @ self.E_h[:H, :48] + e[:, H:] * self.E[H:, :48]
        rt = torch.ldexp(rt, (mi - EMAX).to(torch.int32))
        r = rt[:, : M + 1]
        return torch.linalg.solve(r[:, self.toep] + rt[:, self.hank], r - self.av)

    def run(self, X, n_iter, n_coarse, early):
        """-> (mc, stop step per frame (1-based; n_iter where the frame never stops))"""
        logx2 = torch.log2(X)
        mc = (torch.log(X)) @ self.G
        frozen = torch.zeros(X.size(0), dtype=torch.bool)
        stop = torch.full((X.size(0),), n_iter)
        u_prev = torch.zeros(X.size(0))
        for k in range(1, n_iter + 1):
            coarse = k <= n_coarse
            x = self.step(logx2, mc, coarse)
            mnorm = mc.abs().amax(-1).clamp(min=1.0)
            xinf = x.abs().amax(-1)
            u = xinf / mnorm
            small = (xinf <= TAU * mnorm) | ((xinf <= FACTOR * TAU * mnorm) & (FACTOR * u <= u_prev))
            if coarse or not early:
                small = torch.zeros_like(small)
            u_prev = torch.zeros_like(u) if coarse else u
            mc = torch.where(frozen[:, None], mc, mc + x)
            stop = torch.where(small & ~frozen, torch.full_like(stop, k), stop)
            frozen = frozen | small
            if bool(frozen.all()):
                break
        return mc, stop


def tile_steps(stop):
    t = stop[: stop.numel() // 16 * 16].view(-1, 16).amax(-1)
    return t, float(t.float().mean()), torch.bincount(t, minlength=11).tolist()


def frac(y, ref):
    return float(((y - ref).abs().double() / (5e-6 + 1e-4 * ref.abs().double())).max())


def inputs(U):
    x = {"randn": torch.randn(U, 16000, generator=torch.Generator().manual_seed(1234))}
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "datawav.npz"))["pcm"].astype(np.float64) / 32768.0
    idx = (997 * np.arange(U)[:, None] + np.arange(16000)[None, :]) % pcm.size                 # bench.py: speech_like_batch
    x["speech-like"] = torch.from_numpy(pcm[idx].astype(np.float32))
    t = torch.arange(16000, dtype=torch.float64) / 16000.0
    s = torch.sin(2 * np.pi * 440.0 * t) + 0.5 * torch.sin(2 * np.pi * 3000.0 * t)
    x["near-silent"] = 1e-3 * torch.randn(U, 16000, generator=torch.Generator().manual_seed(17))   # |mc[0]| ~ 14: the gain residual's case
    x["two sines"] = (s[None] + 1e-4 * torch.randn(U, 16000, generator=torch.Generator().manual_seed(3), dtype=torch.float64)).float()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--no-gain-residual", action="store_true", help="coarse steps without the float32 residual of the gain coefficient")
    args = ap.parse_args()
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m = Model(not args.no_gain_residual)
    for name, x in inputs(args.utterances).items():
        X = TP.stft_power(x, 400, 80, NFFT).reshape(-1, H + 1).contiguous()
        print(f"== {name}: {X.size(0)} frames")
        full, stop_f = m.run(X, 10, 0, True)
        _, mean_f, hist_f = tile_steps(stop_f)
        print(f"all-full, early stop: steps per tile mean {mean_f:.3f}, tiles per number of steps {hist_f}")
        for nc in (2, 3):
            y, stop = m.run(X, 10, nc, True)
            _, mean_c, hist_c = tile_steps(stop)
            print(f"steps 1..{nc} coarse, early stop: steps per tile mean {mean_f:.3f} -> {mean_c:.3f}, tiles per number of steps {hist_c}; "
                  f"frames one step later {float((stop > stop_f).float().mean()) * 100:.2f} %, earlier {float((stop < stop_f).float().mean()) * 100:.2f} %; "
                  f"largest deviation from all-full {frac(y, full):.3f} of the tolerance")
        for nc, counts in ((2, (3, 4, 5, 6, 7, 8, 10)), (1, (5, 6, 7))):
            row = []
            for n_iter in counts:
                ref, _ = m.run(X, n_iter, 0, False)
                y, _ = m.run(X, n_iter, nc, False)
                row.append(f"{n_iter}: {frac(y, ref):.3g}")
            print(f"fixed steps, the first {nc} coarse whatever n_iter, against the same count all-full (fraction of the tolerance): " + ", ".join(row))
    print(f"({time.time() - t0:.1f} s)")


if __name__ == "__main__":
    main()
