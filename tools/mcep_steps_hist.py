"""What the stopping rule of the tuned mel-cepstral forward does on the bench inputs, read from the public Newton history.

    python tools/mcep_steps_hist.py [--utterances 64]

For the bench input (seeded randn, 1 s utterances) and the speech-like batch of bench.py (tests/golden/datawav.npz tiled):
  * frames per freeze step -- the first s with hist[s + 1] == hist[s] bitwise (n_iter: never);
  * steps run per 16-frame tile when no history is kept: the tile leaves the loop after the step at which its slowest frame stops,
    which is the first repeated step of that frame (the stopping step's own update is still applied);
  * the update floor: max over frames of |hist[s + 1] - hist[s]|_inf / max(1, |hist[s]|_inf) per step with DSA_ALGO_FIXED_STEPS --
    what the threshold 2^-20 has to stay above on converged frames -- and its per-frame distribution at steps 8..10;
  * the quadratic phase the rule's second clause (round 9) relies on: C = u_(k+1) / u_k^2 of the fixed-step run over frames and steps
    with 2^-10 <= u_k < 3e-2 (below 2^-10 the next update is within reach of the float32 floor, which would pass for a large C), and
    C_max (16 tau)^2 -- the update the clause declines to run -- against a quarter of the floor;
  * frames stopped through each clause: the rule re-evaluated in float64 on the fixed-step history (the history's differences are
    the kernel's updates up to the rounding of one float32 addition, so a few frames at a threshold may be attributed differently)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffsptk_amd as dsp
from diffsptk_amd import _lib, ops

DEV = "cuda"
N_ITER = 10
TAU = 2.0 ** -20     # mh::STOP_TAU
FACTOR = 16.0        # mh::STOP_FACTOR


def history(stft, mcep, x, fixed):
    T = x.size(-1)
    B = x.numel() // T
    N = ops.num_frames(T, 80)
    mc = torch.empty(B, N, 25, device=DEV)
    hist = torch.empty(N_ITER + 1, B * N, 25, device=DEV)
    images = ops.mcep_images(mcep.G, mcep.D, mcep.E, 512, 24)
    scratch = torch.zeros(_lib.SCRATCH_BYTES, dtype=torch.uint8, device=DEV)
    ops._call("dsa_stft_mcep_fwd", x.data_ptr(), B, T, 400, 80, 512, stft.window.data_ptr(), stft.twiddle.data_ptr(), 1, float(stft.eps),
              24, N_ITER, mcep.G.data_ptr(), mcep.D.data_ptr(), mcep.E.data_ptr(), mcep.alpha_vector.data_ptr(), _lib.F32,
              _lib.ALGO_AUTO | (_lib.ALGO_FIXED_STEPS if fixed else 0), images.data_ptr(), scratch.data_ptr(), mc.data_ptr(), hist.data_ptr(),
              None, ops._stream())
    torch.cuda.synchronize()
    return hist


def report(name, stft, mcep, x):
    hist = history(stft, mcep, x, fixed=False)
    bits = hist.view(torch.int32)
    same = (bits[1:] == bits[:-1]).all(-1)
    first = torch.where(same, torch.arange(N_ITER, device=DEV)[:, None], N_ITER).amin(0)     # per frame
    F = first.numel()
    print(f"== {name}: {x.size(0)} utterances, {F} frames")
    print("frames per freeze step (first s with hist[s+1] == hist[s]; 10: never):", torch.bincount(first, minlength=N_ITER + 1).tolist())
    pad = (-F) % 16
    tiles = torch.cat([first, first[-1:].expand(pad)]).view(-1, 16).amax(1).clamp(max=N_ITER)
    print("tiles per number of steps run (no history):", torch.bincount(tiles, minlength=N_ITER + 1).tolist(),
          f" mean {float(tiles.float().mean()):.3f} of {N_ITER}")
    hf = history(stft, mcep, x, fixed=True).double()
    upd = (hf[1:] - hf[:-1]).abs().amax(-1) / hf[:-1].abs().amax(-1).clamp(min=1.0)                     # (n_iter, F)
    print("fixed steps, largest relative update |x|_inf / max(1, |mc|_inf) over frames, steps 1..10:",
          " ".join(f"{float(v):.2e}" for v in upd.amax(1)))
    for s in (7, 8, 9):
        q = torch.quantile(upd[s], torch.tensor([0.5, 0.9, 0.99, 0.999], device=DEV, dtype=torch.float64))
        print(f"  step {s + 1}: median {float(q[0]):.2e}  90% {float(q[1]):.2e}  99% {float(q[2]):.2e}  99.9% {float(q[3]):.2e}  "
              f"above 2^-20: {int((upd[s] > 2.0 ** -20).sum())}  above 2^-19: {int((upd[s] > 2.0 ** -19).sum())}  "
              f"above 2^-18: {int((upd[s] > 2.0 ** -18).sum())} frames")
    floor = float(upd[7:].amax())
    quad = (upd[:-1] >= 2.0 ** -10) & (upd[:-1] < 3e-2)
    C = (upd[1:] / upd[:-1] ** 2)[quad]
    q = torch.quantile(C, torch.tensor([0.5, 0.99], device=DEV, dtype=torch.float64))
    cmax = float(C.max())
    print(f"quadratic phase, C = u_(k+1) / u_k^2 over {C.numel()} (frame, step) pairs with 2^-10 <= u_k < 3e-2: median {float(q[0]):.3g}  "
          f"99% {float(q[1]):.3g}  max {cmax:.4g}")
    print(f"  C_max (16 tau)^2 = {cmax * (FACTOR * TAU) ** 2:.3g} against a quarter of the update floor (largest update of steps 8..10) "
          f"{floor / 4:.3g}: {'holds' if cmax * (FACTOR * TAU) ** 2 <= floor / 4 else 'EXCEEDED -- lower the factor'}")
    prev = torch.cat([torch.zeros_like(upd[:1]), upd[:-1]])
    c1 = upd <= TAU
    c2 = (upd <= FACTOR * TAU) & (upd <= prev / FACTOR)
    c2[0] = False
    steps = torch.arange(N_ITER, device=DEV)[:, None]
    stop = torch.where(c1 | c2, steps, N_ITER).amin(0)                                                  # index of the stopping step
    at = stop.clamp(max=N_ITER - 1)[None]
    by1 = (stop < N_ITER) & c1.gather(0, at)[0]
    by2 = (stop < N_ITER) & ~c1.gather(0, at)[0]
    early1 = by2 & (stop < N_ITER - 1) & c1.gather(0, (at + 1).clamp(max=N_ITER - 1))[0]
    print(f"rule on the fixed-step history: stopped through u <= tau {int(by1.sum())}, through the second clause alone {int(by2.sum())} "
          f"({int(early1.sum())} of them one step before u <= tau would have), never {int((stop == N_ITER).sum())} of {F} frames")
    print("  frames per predicted freeze step:", torch.bincount((stop + 1).clamp(max=N_ITER), minlength=N_ITER + 1).tolist(),
          f" agreeing with the early-stop history in {int(((stop + 1).clamp(max=N_ITER) == first).sum())} frames")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    stft = dsp.STFT(400, 80, 512, device=DEV)
    mcep = dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=N_ITER, device=DEV)
    x = torch.randn(1024, 16000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1234))[: args.utterances].contiguous()
    report("bench input (randn, seed 1234)", stft, mcep, x)
    report("speech-like batch (bench.py)", stft, mcep, bench.speech_like_batch(1024, DEV)[: args.utterances].contiguous())


if __name__ == "__main__":
    main()
