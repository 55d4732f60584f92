#!/usr/bin/env python3
"""Timing of the lapped transforms (csrc/mdct.hip) at 1024 utterances of one second, float32: 16 kHz with frame lengths 512 (the fast
kernels) and 400 (the generic ones), 48 kHz with frame length 2048 (fast).  Per set-up the analysis (mdct), the synthesis (imdct) and
forward + backward of each.  Device time by HIP events around --inner calls, median of --reps windows after --warmup, the two
alternatives alternated window by window in one process:
  * hip    the library's entries through the public modules (one launch per direction);
  * chain  the reference's _forward restated with stock torch operators on the GPU (mdct.py:166-176: pad, unfold, multiply by the window,
           matmul with the dense (L, L/2) basis; imdct.py:169-181: matmul, multiply, F.fold of the frames and of the squared rectangular
           window, divide, slice), its backward by autograd.  It is the yardstick: there is no earlier implementation in this library.
Beside each time the least traffic of the operation -- L/2 samples in and L/2 coefficients out per frame, 8 P bytes in float32 (twice
that forward + backward) -- and the share of the HBM peak that it amounts to.

    python tools/time_mdct.py [--reps 15] [--warmup 3] [--inner 10] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as NF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib  # noqa: E402
from diffsptk_amd.utils import tables  # noqa: E402
from time_parcor import HBM_PEAK, alternate  # noqa: E402

B = 1024
SETUPS = ((512, 16000), (400, 16000), (2048, 48000))


def chain_mdct(x, w, W, P):
    L = w.numel()
    x = NF.pad(NF.pad(x, (0, P)), (L // 2, (L - 1) // 2))   # mdct.py:175, frame.py:134-137
    return torch.matmul(x.unfold(-1, L, P) * w, W)


def chain_imdct(y, w, Wt, P, out_length):
    L, N = w.numel(), y.size(-2)
    ones = torch.ones(1, L, 1, device=y.device, dtype=y.dtype).repeat(1, 1, N)   # Unframe's rectangular window (unframe.py:201-205)

    def fold(t):
        return NF.fold(t, (1, (N - 1) * P + L), (1, L), stride=(1, P))[..., 0, 0, L // 2:L // 2 + out_length]

    v = (torch.matmul(y, Wt) * w).transpose(-2, -1)
    return fold(v * ones) / (fold(ones * ones) + 1e-16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    ap.add_argument("--batch", type=int, default=B)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for L, T in SETUPS:
        P = L // 2
        x = torch.randn(args.batch, T, device=dev, generator=g)
        mdct, imdct = dsp.MDCT(L, device=dev), dsp.IMDCT(L, device=dev)
        w = torch.from_numpy(tables.window_table(L, "sine", "none", True)).to(dev, torch.float32)
        W = torch.from_numpy(tables.mdct_basis(L, "sine", "cosine")).to(dev, torch.float32)
        Wt = W.T.contiguous()
        with torch.no_grad():
            y = mdct(x)
            kernels = []
            for fn in (lambda: mdct(x), lambda: imdct(y, T)):
                fn()
                kernels.append(_lib.last_kernel())
            diff_a = float((y - chain_mdct(x, w, W, P)).abs().max())
            diff_s = float((imdct(y, T) - chain_imdct(y, w, Wt, P, T)).abs().max())
            rt = float((imdct(y, T) - x).abs().max())
        N = y.size(-2)
        least = 8 * P * args.batch * N
        xg, yg = x.clone().requires_grad_(), y.clone().requires_grad_()
        gy, gx = torch.randn_like(y), torch.randn_like(x)

        def both(fn, inp, cot):
            def run():
                inp.grad = None
                fn(inp).backward(cot)
            return run

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        pairs = {
            "analysis": (no_grad(lambda: mdct(x)), no_grad(lambda: chain_mdct(x, w, W, P)), least, diff_a, kernels[0]),
            "synthesis": (no_grad(lambda: imdct(y, T)), no_grad(lambda: chain_imdct(y, w, Wt, P, T)), least, diff_s, kernels[1]),
            "analysis fwd+bwd": (both(mdct, xg, gy), both(lambda t: chain_mdct(t, w, W, P), xg, gy), 2 * least, diff_a, kernels[0]),
            "synthesis fwd+bwd": (both(lambda t: imdct(t, T), yg, gx), both(lambda t: chain_imdct(t, w, Wt, P, T), yg, gx), 2 * least, diff_s, kernels[1]),
        }
        for name, (hip, chain, nbytes, diff, kernel) in pairs.items():
            hip_ms, chain_ms = alternate([hip, chain], args.reps, args.warmup, args.inner)
            rows.append({"L": L, "T": T, "frames": args.batch * N, "op": name, "kernel": kernel, "hip_ms": hip_ms, "chain_ms": chain_ms,
                         "least_bytes": nbytes, "hbm_peak_ms": nbytes / HBM_PEAK * 1e3, "share_of_hbm_peak": nbytes / HBM_PEAK * 1e3 / hip_ms,
                         "max_abs_diff_to_chain": diff, "round_trip_error": rt})
    lines = [f"mdct  utterances={args.batch} float32  {torch.cuda.get_device_name(0)}  (device events, median of {args.reps} windows of "
             f"{args.inner} calls, hip and chain alternated; least traffic 8 P bytes per frame and direction; HBM peak {HBM_PEAK / 1e12:.1f} TB/s)",
             f"{'L':>5s} {'T':>6s} {'frames':>8s} {'operation':18s} {'kernel family':23s} {'hip ms':>9s} {'chain ms':>9s} {'chain/hip':>9s} {'least MB':>9s} "
             f"{'ms at peak':>10s} {'share of peak':>13s} {'|hip - chain|':>13s} {'round trip':>10s}"]
    for r in rows:
        lines.append(f"{r['L']:5d} {r['T']:6d} {r['frames']:8d} {r['op']:18s} {r['kernel']:23s} {r['hip_ms']:9.4f} {r['chain_ms']:9.4f} "
                     f"{r['chain_ms'] / r['hip_ms']:9.1f} {r['least_bytes'] / 1e6:9.2f} {r['hbm_peak_ms']:10.4f} {r['share_of_hbm_peak']:13.2f} "
                     f"{r['max_abs_diff_to_chain']:13.2e} {r['round_trip_error']:10.2e}")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
