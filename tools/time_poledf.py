#!/usr/bin/env python3
"""Timing of AllPoleDigitalFilter (csrc/poledf.hip): forward, and forward + backward (gx and ga), at T = 16 000, M = 24, P = 80
over batches of 1 .. 4096 utterances (float32; float64 at 1024).  Device time by HIP events, median of --reps after --warmup.
Cycles per sample per wave = ms x clock / T, one wave per utterance (at the 2.4 GHz peak engine clock unless --clock-ghz).

    python tools/time_poledf.py [--reps 20] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd.functional as F  # noqa: E402
from diffsptk_amd import _lib  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    T, M, P = 16000, 24, 80
    N = T // P
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    print(f"poledf  T={T} M={M} P={P}  (median of {args.reps}; cycles/sample at {args.clock_ghz} GHz)")
    print(f"{'dtype':8s} {'B':>5s} {'fwd ms':>9s} {'fwd+bwd ms':>11s} {'fwd cyc/s':>10s} {'f+b cyc/s':>10s}  kernels")
    for dt, B in [(torch.float32, b) for b in (1, 16, 256, 1024, 4096)] + [(torch.float64, 1024)]:
        x = torch.randn(B, T, device=dev, dtype=dt, generator=g) * 0.1
        a = (torch.rand(B, N, M + 1, device=dev, dtype=dt, generator=g) * 2 - 1) * (0.6 / M)
        a[..., 0] = 1.0
        gy = torch.randn(B, T, device=dev, dtype=dt, generator=g)
        xg, ag = x.clone().requires_grad_(True), a.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                F.poledf(x, a, P)

        def fwdbwd():
            y = F.poledf(xg, ag, P)
            xg.grad = ag.grad = None
            y.backward(gy)

        fwd()
        kf = _lib.last_kernel()
        t_f = timed(fwd, args.reps, args.warmup)
        t_fb = timed(fwdbwd, args.reps, args.warmup)
        cyc = lambda ms: ms * 1e-3 * args.clock_ghz * 1e9 / T   # noqa: E731
        name = str(dt).replace("torch.", "")
        print(f"{name:8s} {B:5d} {t_f:9.3f} {t_fb:11.3f} {cyc(t_f):10.1f} {cyc(t_fb):10.1f}  {kf}")
        rows.append(dict(dtype=name, B=B, T=T, M=M, P=P, fwd_ms=t_f, fwdbwd_ms=t_fb, fwd_cycles_per_sample=cyc(t_f),
                         fwdbwd_cycles_per_sample=cyc(t_fb), fwd_kernel=kf))
        del x, a, gy, xg, ag
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "clock_ghz": args.clock_ghz, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
