#!/usr/bin/env python3
"""Timing of mlsacheck (csrc/mlsacheck.hip) at the bench size: 204 800 frames, M = 24, float32, alpha 0.42, the threshold of
pade_order 4 (4.5), n_fft 256.  Device time by HIP events around --inner calls, median of --reps windows after --warmup, the alternatives
alternated window by window in one process:
  * hip    the library's entry through the public functional, warn_type "ignore" (one launch forward, one backward);
  * chain  the same operation written with stock torch operators on the GPU -- the reference's _forward (mlsacheck.py:181-230) without
           its torch.any, which would synchronise: rfft / abs / amax / clip / irfft and the concatenations.
The three modes (fast, scale, clip), forward alone (no_grad) and forward + backward.  Every third frame is 1.3 .. 3 times over the
threshold, the others 0.2 .. 0.8 of it (by scaling the frame; in fast mode by moving mc_1, since the plain sum can cancel).  The two C
entries are also timed alone per mode, on buffers allocated once, beside the bytes they move and the time those bytes take at the HBM
peak.

    python tools/time_mlsacheck.py [--reps 15] [--warmup 3] [--inner 10] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd.functional as F  # noqa: E402
from diffsptk_amd import _lib, ops as O  # noqa: E402
from time_parcor import HBM_PEAK, alternate  # noqa: E402

FRAMES, M = 204800, 24
ALPHA, THR, N_FFT = 0.42, 4.5, 256
MODES = {"fast": dict(fast=True), "scale": dict(fast=False, mod_type="scale"), "clip": dict(fast=False, mod_type="clip")}


def chain_mlsacheck(mc, alpha_vector, fast, mod_type):
    gain = (mc * alpha_vector).sum(-1, keepdim=True)
    if fast:
        max_amplitude = mc.sum(-1, keepdim=True) - gain
    else:
        c1 = torch.cat((mc[..., :1] - gain, mc[..., 1:]), dim=-1)
        C1 = torch.fft.rfft(c1, n=N_FFT)
        C1_amplitude = C1.abs()
        max_amplitude = torch.amax(C1_amplitude, dim=-1, keepdim=True)
    max_amplitude = torch.clip(max_amplitude, min=1e-16)
    scale = torch.clip(THR / (C1_amplitude if mod_type == "clip" else max_amplitude), max=1)
    if fast:
        c0, c1 = torch.split(mc, [1, mc.size(-1) - 1], dim=-1)
        return torch.cat(((c0 - gain) * scale + gain, c1 * scale), dim=-1)
    c2 = torch.fft.irfft(C1 * scale)[..., : mc.size(-1)]
    return torch.cat((c2[..., :1] + gain, c2[..., 1:]), dim=-1)


def amplitude(mc, alpha_vector, fast):
    gain = (mc * alpha_vector).sum(-1, keepdim=True)
    c1 = torch.cat((mc[..., :1] - gain, mc[..., 1:]), dim=-1)
    return c1.sum(-1) if fast else torch.fft.rfft(c1, n=N_FFT).abs().amax(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    av = (-ALPHA) ** torch.arange(M + 1, device=dev, dtype=torch.float64)
    av = av.float()
    base = 0.5 * torch.randn(FRAMES, M + 1, device=dev, generator=g) * torch.linspace(1, 0.05, M + 1, device=dev)
    want = torch.where(torch.arange(FRAMES, device=dev) % 3 == 0, torch.rand(FRAMES, device=dev, generator=g) * 1.7 + 1.3,
                       torch.rand(FRAMES, device=dev, generator=g) * 0.6 + 0.2) * THR
    cot = torch.randn(FRAMES, M + 1, device=dev, generator=g)
    row_bytes = FRAMES * (M + 1) * 4
    rows, diffs, erows, inputs = [], {}, [], {}
    for name, kw in MODES.items():
        if kw["fast"]:   # the plain sum may cancel: moved to its target through mc_1, whose weight in it is 1 + alpha
            x = base.clone()
            x[:, 1] += (want - amplitude(base, av, True)) / (1 + ALPHA)
        else:
            x = base * (want / amplitude(base, av, False)).unsqueeze(-1)
        inputs[name] = x
        hip = lambda t, kw=kw: F.mlsacheck(t, alpha=ALPHA, n_fft=N_FFT, warn_type="ignore", **kw)   # noqa: E731
        chain = lambda t, kw=kw: chain_mlsacheck(t, av, kw["fast"], kw.get("mod_type", "scale"))   # noqa: E731
        with torch.no_grad():
            y = hip(x)
            diffs[name] = float((y - chain(x)).abs().max())
            moved = float((y != x).any(-1).float().mean())
        xg = x.clone().requires_grad_(True)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(x)
            return run

        def both(fn):
            def run():
                xg.grad = None
                fn(xg).backward(cot)
            return run

        for what, wrap, n in (("fwd", fwd, 2), ("fwd+bwd", both, 2 + 3)):
            ms = alternate([wrap(hip), wrap(chain)], args.reps, args.warmup, args.inner)
            floor_ms = n * row_bytes / HBM_PEAK * 1e3
            rows.append({"mode": name, "what": what, "hip_ms": ms[0], "chain_ms": ms[1], "bytes": n * row_bytes, "hbm_peak_ms": floor_ms,
                         "share_of_hbm_peak": floor_ms / ms[0], "frames_moved": moved})
    # the two entries alone: no autograd, no allocation
    L, st, p = _lib.load(), O._stream(), (lambda t: t.data_ptr())
    out = torch.empty_like(base)
    entries = {}
    for name, x in inputs.items():
        code = O.MLSACHECK_MODES[name]
        entries[f"dsa_mlsacheck {name}"] = (lambda x=x, code=code: L.dsa_mlsacheck(p(x), FRAMES, M, ALPHA, THR, code, N_FFT, _lib.F32, p(out), None, st), 2)
        entries[f"dsa_mlsacheck_vjp {name}"] = (lambda x=x, code=code: L.dsa_mlsacheck_vjp(p(cot), p(x), FRAMES, M, ALPHA, THR, code, N_FFT, _lib.F32, p(out), st), 3)
    for fn, _ in entries.values():
        _lib.check(fn())
    ems = alternate([fn for fn, _ in entries.values()], args.reps, args.warmup, 5 * args.inner)
    erows = [{"entry": name, "ms": t, "bytes": n * row_bytes, "hbm_peak_ms": n * row_bytes / HBM_PEAK * 1e3,
              "share_of_hbm_peak": n * row_bytes / HBM_PEAK * 1e3 / t} for (name, (_, n)), t in zip(entries.items(), ems)]
    lines = [f"mlsacheck  frames={FRAMES} M={M} float32 alpha={ALPHA} threshold={THR} n_fft={N_FFT}  {torch.cuda.get_device_name(0)}  "
             f"(median of {args.reps} windows of {args.inner} calls, hip and chain alternating; every third frame over the threshold)",
             "max |hip - chain|: " + "  ".join(f"{n} {v:.2e}" for n, v in diffs.items()),
             f"{'mode':6s} {'':8s} {'hip ms':>9s} {'chain ms':>9s} {'chain/hip':>9s} {'MB moved':>9s} {'ms at 8 TB/s':>13s} {'share of peak':>13s} {'frames moved':>13s}"]
    for r in rows:
        lines.append(f"{r['mode']:6s} {r['what']:8s} {r['hip_ms']:9.4f} {r['chain_ms']:9.3f} {r['chain_ms'] / r['hip_ms']:9.1f} {r['bytes'] / 1e6:9.2f} "
                     f"{r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f} {r['frames_moved']:13.3f}")
    lines.append(f"{'entry alone':24s} {'ms':>9s} {'MB moved':>9s} {'ms at 8 TB/s':>13s} {'share of peak':>13s}")
    for r in erows:
        lines.append(f"{r['entry']:24s} {r['ms']:9.4f} {r['bytes'] / 1e6:9.2f} {r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f}")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "frames": FRAMES, "M": M, "dtype": "float32", "hbm_peak_bytes_per_s": HBM_PEAK,
                       "reps": args.reps, "inner": args.inner, "max_abs_diff": diffs, "rows": rows, "entries": erows}, f, indent=1)


if __name__ == "__main__":
    main()
