#!/usr/bin/env python3
"""Timing of lpc2par / par2lpc / lpccheck (csrc/parcor.hip) at the bench size: 204 800 frames, M = 24, float32.  Device time by HIP
events around --inner calls, median of --reps windows after --warmup, the two alternatives alternated window by window in one
process:
  * hip    the library's entry through the public functional (one launch forward, one backward);
  * chain  the same operation written with stock torch operators on the GPU, one slice / flip / multiply / divide / cat per
           order -- what a user has without this library.
Forward alone (no_grad) and forward + backward (a gradient for the input); these include the host's work per call (autograd, allocation),
which at these kernel lengths can be what the device waits for.  The six C entries are therefore also timed alone, on buffers
allocated once.  Beside each time: the bytes the launches need, computed
from the shape, the time those bytes take at the HBM peak, and the share of that peak the measured time stands for.

    python tools/time_parcor.py [--reps 15] [--warmup 3] [--inner 10] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd.functional as F  # noqa: E402
from diffsptk_amd import _lib, ops as O  # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s, the HBM3E specification of the MI355X (6.29e12 measured with a float4 copy)
FRAMES, M = 204800, 24


def chain_lpc2par(a, gamma=1.0):
    K, c = a[..., :1], a[..., 1:] * gamma
    ks = []
    for m in range(c.size(-1), 0, -1):
        km = c[..., m - 1:m]
        ks.append(km)
        if m > 1:
            low = c[..., :m - 1]
            c = (low - km * low.flip(-1)) / (1 - km * km)
    return torch.cat([K] + ks[::-1], -1)


def chain_par2lpc(k, gamma=1.0):
    c = k[..., 1:2]
    for m in range(2, k.size(-1)):
        km = k[..., m:m + 1]
        c = torch.cat((c + km * c.flip(-1), km), -1)
    return torch.cat((k[..., :1], c), -1) / gamma


def chain_lpccheck(a, margin):
    k = chain_lpc2par(a)
    return chain_par2lpc(torch.cat((k[..., :1], torch.clip(k[..., 1:], margin - 1, 1 - margin)), -1))


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fns, reps, warmup, inner):
    """Median ms per call of each fn, the fns taking turns window by window."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(window(fn, inner))
    return [sorted(v)[len(v) // 2] for v in ms]


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
    # stable, well-conditioned rows: PARCOR U(-0.9, 0.9) / m, K in (0.5, 1.5); nothing gets clipped (the time does not depend on it)
    k = (torch.rand(FRAMES, M + 1, device=dev, generator=g) * 1.8 - 0.9) / torch.arange(M + 1, device=dev).clamp(min=1)
    k[:, 0] = torch.rand(FRAMES, device=dev, generator=g) + 0.5
    a = F.par2lpc(k)
    w = torch.randn(FRAMES, M + 1, device=dev, generator=g)
    row_bytes = FRAMES * (M + 1) * 4
    ops = {   # name: (hip, chain, input, tensors moved forward, tensors moved forward + backward)
        "lpc2par": (lambda t: F.lpc2par(t), chain_lpc2par, a, 2, 2 + 3),
        "par2lpc": (lambda t: F.par2lpc(t), chain_par2lpc, k, 2, 2 + 3),
        "lpccheck": (lambda t: F.lpccheck(t, 0.01, "ignore"), lambda t: chain_lpccheck(t, 0.01), a, 2, 3 + 3),
    }
    rows, diffs = [], {}
    for name, (hip, chain, x, n_fwd, n_both) in ops.items():
        with torch.no_grad():
            diffs[name] = float((hip(x) - chain(x)).abs().max())
        xg = x.clone().requires_grad_(True)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(x)
            return run

        def both(fn):
            def run():
                xg.grad = None
                fn(xg).backward(w)
            return run

        for what, wrap, n in (("fwd", fwd, n_fwd), ("fwd+bwd", both, n_both)):
            t_hip, t_chain = alternate([wrap(hip), wrap(chain)], args.reps, args.warmup, args.inner)
            floor_ms = n * row_bytes / HBM_PEAK * 1e3
            rows.append({"op": name, "what": what, "hip_ms": t_hip, "chain_ms": t_chain, "chain_over_hip": t_chain / t_hip,
                         "bytes": n * row_bytes, "hbm_peak_ms": floor_ms, "share_of_hbm_peak": floor_ms / t_hip})
    # the six entries alone: no autograd, no allocation
    L, st, p = _lib.load(), O._stream(), (lambda t: t.data_ptr())
    out, kk, g1 = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    entries = {
        "dsa_lpc2par_fwd": (lambda: L.dsa_lpc2par_fwd(p(a), FRAMES, M, 1.0, _lib.F32, p(out), st), 2),
        "dsa_lpc2par_bwd": (lambda: L.dsa_lpc2par_bwd(p(w), p(k), FRAMES, M, 1.0, _lib.F32, p(g1), st), 3),
        "dsa_par2lpc_fwd": (lambda: L.dsa_par2lpc_fwd(p(k), FRAMES, M, 1.0, _lib.F32, p(out), st), 2),
        "dsa_par2lpc_bwd": (lambda: L.dsa_par2lpc_bwd(p(w), p(k), FRAMES, M, 1.0, _lib.F32, p(g1), st), 3),
        "dsa_lpccheck_fwd": (lambda: L.dsa_lpccheck_fwd(p(a), FRAMES, M, 0.99, _lib.F32, p(out), None, None, st), 2),
        "dsa_lpccheck_fwd+k": (lambda: L.dsa_lpccheck_fwd(p(a), FRAMES, M, 0.99, _lib.F32, p(out), p(kk), None, st), 3),
        "dsa_lpccheck_bwd": (lambda: L.dsa_lpccheck_bwd(p(w), p(k), FRAMES, M, 0.99, _lib.F32, p(g1), st), 3),
    }
    for fn, _ in entries.values():
        _lib.check(fn())
    ems = alternate([fn for fn, _ in entries.values()], args.reps, args.warmup, 5 * args.inner)
    erows = [{"entry": name, "ms": t, "bytes": n * row_bytes, "hbm_peak_ms": n * row_bytes / HBM_PEAK * 1e3,
              "share_of_hbm_peak": n * row_bytes / HBM_PEAK * 1e3 / t} for (name, (_, n)), t in zip(entries.items(), ems)]
    lines = [f"parcor  frames={FRAMES} M={M} float32  {torch.cuda.get_device_name(0)}  (median of {args.reps} windows of {args.inner} calls, "
             "hip and chain alternating)",
             "max |hip - chain|: " + "  ".join(f"{n} {d:.2e}" for n, d in diffs.items()),
             f"{'op':9s} {'':8s} {'hip ms':>9s} {'chain ms':>9s} {'chain/hip':>9s} {'MB moved':>9s} {'ms at 8 TB/s':>13s} {'share of peak':>13s}"]
    for r in rows:
        lines.append(f"{r['op']:9s} {r['what']:8s} {r['hip_ms']:9.4f} {r['chain_ms']:9.3f} {r['chain_over_hip']:9.1f} {r['bytes'] / 1e6:9.2f} "
                     f"{r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f}")
    lines.append(f"{'entry alone':20s} {'ms':>9s} {'MB moved':>9s} {'ms at 8 TB/s':>13s} {'share of peak':>13s}")
    for r in erows:
        lines.append(f"{r['entry']:20s} {r['ms']:9.4f} {r['bytes'] / 1e6:9.2f} {r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f}")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "frames": FRAMES, "M": M, "dtype": "float32", "hbm_peak_bytes_per_s": HBM_PEAK,
                       "reps": args.reps, "inner": args.inner, "max_abs_diff_vs_chain": diffs, "rows": rows, "entries": erows}, f, indent=1)


if __name__ == "__main__":
    main()
