#!/usr/bin/env python3
"""Timing of the pseudo-QMF bank (csrc/pqmf.hip) against the reference's own op sequence, at B = 1024 utterances x T = 16 000
samples, float32, K = 4, M = 40 and 62:

    PQMF                     ours: dsa_pqmf_fwd              reference: ConstantPad1d, ReplicationPad1d, conv1d (pqmf.py:257)
    fuse(pqmf, decimate)     ours: dsa_pqmf_fwd (K, 0)       reference: the same, then [..., ::K] (decimate.py:92)
    IPQMF                    ours: dsa_ipqmf_fwd             reference: pads, conv1d (ipqmf.py:137), on (B, K, T)
    fuse(interpolate, ipqmf) ours: dsa_ipqmf_fwd (K, 0)      reference: zeros + index_copy_ (interpolate.py:93-95), pads, conv1d

each forward and forward + backward (input gradient), in the same process on the same device, alternated per repetition.  Device
time by HIP events, median of --reps after --warmup.  Bytes and multiply-adds are computed from the shapes; the floors use
6.29 TB/s (measured copy rate) and 39 T FMA/s (unpacked v_fma_f32) from MI355X_MICROARCH.md.  Kernel times: run under
`rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/time_pqmf.py [--reps 20] [--warmup 3] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as tF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib  # noqa: E402

HBM = 6.29e12
FMA = 39e12


def timed_pair(fa, fb, reps, warmup):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]


def pads(M, analysis):
    if M % 2 == 0:
        return M // 2, M // 2
    return ((M + 1) // 2, (M - 1) // 2) if analysis else ((M - 1) // 2, (M + 1) // 2)


def ref_pad(x, dl, dr):
    return tF.pad(tF.pad(x, (dl, 0)), (0, dr), mode="replicate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    B, T, K = 1024, 16000, 4
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows, lines = [], []
    head = (f"pqmf B={B} T={T} K={K} float32 (median of {args.reps}, alternated with the reference op sequence)\n"
            f"{'route':24s} {'M':>3s} {'ours fwd':>9s} {'ref fwd':>9s} {'x':>5s} {'ours f+b':>9s} {'ref f+b':>9s} {'x':>5s} "
            f"{'MB':>6s} {'mem us':>7s} {'fma us':>7s} {'HBM %':>6s}  kernel")
    print(head)
    lines.append(head)
    x = torch.randn(B, T, device=dev, generator=g)
    for M in (40, 62):
        pq, ip = dsp.PQMF(K, M, device=dev), dsp.IPQMF(K, M, device=dev)
        fa, fs = dsp.fuse(pq, dsp.Decimation(K)), dsp.fuse(dsp.Interpolation(K), ip)
        wa, ws = pq.filters, ip.filters
        al, ar = pads(M, True)
        sl, sr = pads(M, False)
        yfull = torch.randn(B, K, T, device=dev, generator=g)
        ysub = torch.randn(B, K, T // K, device=dev, generator=g)
        idx = torch.arange(0, T, K, device=dev)

        def ref_pqmf(v):
            return tF.conv1d(ref_pad(v.unsqueeze(1), al, ar), wa)

        def ref_ipqmf(v):
            return tF.conv1d(ref_pad(v, sl, sr), ws)

        def ref_interp(v):
            return torch.zeros(v.size(0), K, v.size(-1) * K, device=dev).index_copy_(2, idx, v)

        routes = [
            ("pqmf", x, pq, ref_pqmf, 4 * B * T * (1 + K), B * T * K * (M + 1)),
            ("fuse(pqmf, decimate)", x, fa, lambda v: ref_pqmf(v)[..., ::K], 4 * B * T * 2, B * T * (M + 1)),
            ("ipqmf", yfull, lambda v: ip(v), ref_ipqmf, 4 * B * T * (K + 1), B * T * K * (M + 1)),
            ("fuse(interpolate, ipqmf)", ysub, lambda v: fs(v), lambda v: ref_ipqmf(ref_interp(v)), 4 * B * T * 2, B * T * (M + 1)),
        ]
        for name, inp, ours, ref, nbytes, nfma in routes:
            ig = inp.clone().requires_grad_(True)
            with torch.no_grad():
                o2 = ref(inp)
                o1 = ours(inp)
                kern = _lib.last_kernel()
            err = float((o1 - o2).abs().max() / o2.abs().max())
            gout = torch.randn(o1.shape, device=dev, generator=g)

            def fwd_ours():
                with torch.no_grad():
                    ours(inp)

            def fwd_ref():
                with torch.no_grad():
                    ref(inp)

            def fb_ours():
                ig.grad = None
                ours(ig).backward(gout)

            def fb_ref():
                ig.grad = None
                ref(ig).backward(gout)

            tf, tfr = timed_pair(fwd_ours, fwd_ref, args.reps, args.warmup)
            tb, tbr = timed_pair(fb_ours, fb_ref, args.reps, args.warmup)
            mem_us, fma_us = nbytes / HBM * 1e6, nfma / FMA * 1e6
            share = mem_us / (tf * 1e3)
            line = (f"{name:24s} {M:3d} {tf:9.4f} {tfr:9.4f} {tfr / tf:5.2f} {tb:9.4f} {tbr:9.4f} {tbr / tb:5.2f} "
                    f"{nbytes / 1e6:6.1f} {mem_us:7.1f} {fma_us:7.1f} {100 * share:6.1f}  {kern}  (max rel diff {err:.1e})")
            print(line)
            lines.append(line)
            rows.append(dict(route=name, K=K, M=M, B=B, T=T, fwd_ms=tf, ref_fwd_ms=tfr, fwdbwd_ms=tb, ref_fwdbwd_ms=tbr,
                             fwd_speedup=tfr / tf, fwdbwd_speedup=tbr / tb, bytes=nbytes, fma=nfma, mem_floor_us=mem_us,
                             fma_floor_us=fma_us, hbm_share_fwd=share, kernel=kern, max_rel_diff_vs_reference=err))
            del ig, gout, o1, o2
        del yfull, ysub
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
