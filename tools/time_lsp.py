#!/usr/bin/env python3
"""Timing of lpc2lsp / lsp2lpc / lspcheck (csrc/lsp.hip) at the bench size: 204 800 frames, M = 24, float32.  Device time by HIP events
around --inner calls, median of --reps windows after --warmup, the alternatives alternated window by window in one process:
  * hip    the library's entry through the public functional (one launch forward, one backward);
  * chain  the same operation written with stock torch operators on the GPU -- what a user has without this library:
           lpc2lsp   the deflated sum and difference polynomials, their companion matrices, torch.linalg.eigvals, angle, sort.  The
                     eigenvalue solver works matrix by matrix with the host in the loop, so it is timed on --eig-frames frames only,
                     forward only, once; the table gives that time and the time per frame beside the kernel's;
           lsp2lpc   the product of real second-order sections, one pad / multiply / add group per section;
           lspcheck  the reference's Python double loop (n_iter = 10) with its batch-wide break.
Forward alone (no_grad) and forward + backward.  The six C entries are also timed alone, on buffers allocated once, beside the
bytes they move and the time those bytes take at the HBM peak.

    python tools/time_lsp.py [--reps 15] [--warmup 3] [--inner 10] [--eig-frames 2048] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd.functional as F  # noqa: E402
from diffsptk_amd import _lib, ops as O  # noqa: E402
from time_parcor import HBM_PEAK, alternate  # noqa: E402

FRAMES, M = 204800, 24
RATE, N_ITER = 0.01, 10
pad = torch.nn.functional.pad


def chain_lsp2lpc(w):
    def product(cols):
        poly = torch.ones_like(w[..., :1])
        for j in range(cols.size(-1)):
            poly = pad(poly, (0, 2)) - 2 * torch.cos(cols[..., j:j + 1]) * pad(poly, (1, 1)) + pad(poly, (2, 0))
        return poly

    q, p = product(w[..., 1::2]), product(w[..., 2::2])   # M even
    q, p = pad(q, (0, 1)) + pad(q, (1, 0)), pad(p, (0, 1)) - pad(p, (1, 0))
    return torch.cat((w[..., :1], 0.5 * (p + q)[..., 1:w.size(-1)]), -1)


def chain_lpc2lsp(a):
    a1 = pad(torch.cat((torch.ones_like(a[..., :1]), a[..., 1:]), -1), (0, 1))
    p, q = a1 - a1.flip(-1), a1 + a1.flip(-1)
    p, q = torch.cumsum(p, -1)[..., :-1], (torch.cumsum(q * (-1.0) ** torch.arange(q.size(-1), device=a.device), -1)
                                           * (-1.0) ** torch.arange(q.size(-1), device=a.device))[..., :-1]   # / (1 - z^-1), / (1 + z^-1)
    angles = []
    for poly in (p, q):
        n = poly.size(-1) - 1
        comp = torch.zeros(*poly.shape[:-1], n, n, device=a.device, dtype=a.dtype)
        comp[..., 0, :] = -poly[..., 1:] / poly[..., :1]
        comp[..., 1:, :-1] = torch.eye(n - 1, device=a.device, dtype=a.dtype)
        ang = torch.angle(torch.linalg.eigvals(comp))
        angles.append(torch.sort(ang, -1).values[..., n // 2:])
    return torch.cat((a[..., :1], torch.sort(torch.cat(angles, -1), -1).values), -1)


def chain_lspcheck(w, rate=RATE, n_iter=N_ITER):
    d = rate * math.pi / w.size(-1)
    K, w1 = torch.split(w, [1, w.size(-1) - 1], dim=-1)
    w1 = w1.clone()
    for _ in range(n_iter):
        for m in range(w1.size(-1) - 1):
            step = 0.5 * torch.clip(d - (w1[..., m + 1] - w1[..., m]), min=0)
            w1[..., m] -= step
            w1[..., m + 1] += step
        w1 = torch.clip(w1, min=d, max=math.pi - d)
        if torch.all(d - 1e-16 <= torch.diff(w1, dim=-1)):
            break
    return torch.cat((K, w1), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--eig-frames", type=int, default=2048)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    # LSPs at (i + jitter) pi / (M + 1), jitter within +-0.3, K in (0.5, 1.5); for lspcheck every third row has one pair 1e-4 apart
    w = (torch.arange(M + 1, device=dev) + torch.rand(FRAMES, M + 1, device=dev, generator=g) * 0.6 - 0.3) * (math.pi / (M + 1))
    w[:, 0] = torch.rand(FRAMES, device=dev, generator=g) + 0.5
    a = F.lsp2lpc(w)
    wbad = w.clone()
    wbad[::3, 8] = wbad[::3, 7] + 1e-4
    cot = torch.randn(FRAMES, M + 1, device=dev, generator=g)
    row_bytes = FRAMES * (M + 1) * 4
    ops = {   # name: (hip, chain, input, tensors moved forward, tensors moved forward + backward)
        "lsp2lpc": (lambda t: F.lsp2lpc(t), chain_lsp2lpc, w, 2, 2 + 3),
        "lspcheck": (lambda t: F.lspcheck(t, RATE, N_ITER, "ignore"), chain_lspcheck, wbad, 2, 2 + 3),
        "lpc2lsp": (lambda t: F.lpc2lsp(t), None, a, 2, 2 + 4),
    }
    rows, diffs = [], {}
    for name, (hip, chain, x, n_fwd, n_both) in ops.items():
        if chain is not None:
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
                fn(xg).backward(cot)
            return run

        for what, wrap, n in (("fwd", fwd, n_fwd), ("fwd+bwd", both, n_both)):
            fns = [wrap(hip)] + ([wrap(chain)] if chain is not None else [])
            ms = alternate(fns, args.reps, args.warmup, args.inner)
            floor_ms = n * row_bytes / HBM_PEAK * 1e3
            rows.append({"op": name, "what": what, "hip_ms": ms[0], "chain_ms": ms[1] if chain is not None else None,
                         "bytes": n * row_bytes, "hbm_peak_ms": floor_ms, "share_of_hbm_peak": floor_ms / ms[0]})
    with torch.no_grad():
        diffs["lpc2lsp (round trip against the LSPs it came from)"] = float((F.lpc2lsp(a) - w).abs().max())
    # the eigenvalue route, on a slice, once after one warm-up call: wall time with a synchronisation (the solver involves the host)
    eig = {"frames": args.eig_frames}
    try:
        sl = a[:args.eig_frames]
        with torch.no_grad():
            y = chain_lpc2lsp(sl)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chain_lpc2lsp(sl)
            torch.cuda.synchronize()
            eig["ms"] = (time.perf_counter() - t0) * 1e3
            eig["max_abs_diff_vs_hip"] = float((y - F.lpc2lsp(sl)).abs().max())
        eig["us_per_frame"] = eig["ms"] * 1e3 / args.eig_frames
    except Exception as e:   # noqa: BLE001  (a build of torch without a device eigenvalue solver)
        eig["error"] = f"{type(e).__name__}: {e}"[:300]
    # the six entries alone: no autograd, no allocation
    L, st, p = _lib.load(), O._stream(), (lambda t: t.data_ptr())
    out, g1 = torch.empty_like(a), torch.empty_like(a)
    lsp = F.lpc2lsp(a)
    d = RATE * math.pi / (M + 1)
    entries = {
        "dsa_lpc2lsp_fwd": (lambda: L.dsa_lpc2lsp_fwd(p(a), FRAMES, M, 0, 1.0, _lib.F32, p(out), None, st), 2),
        "dsa_lpc2lsp_bwd": (lambda: L.dsa_lpc2lsp_bwd(p(cot), p(a), p(lsp), FRAMES, M, 0, 1.0, _lib.F32, p(g1), st), 4),
        "dsa_lsp2lpc_fwd": (lambda: L.dsa_lsp2lpc_fwd(p(w), FRAMES, M, 0, 1.0, _lib.F32, p(out), st), 2),
        "dsa_lsp2lpc_bwd": (lambda: L.dsa_lsp2lpc_bwd(p(cot), p(w), FRAMES, M, 0, 1.0, _lib.F32, p(g1), st), 3),
        "dsa_lspcheck_fwd": (lambda: L.dsa_lspcheck_fwd(p(wbad), FRAMES, M, d, N_ITER, _lib.F32, p(out), None, st), 2),
        "dsa_lspcheck_bwd": (lambda: L.dsa_lspcheck_bwd(p(cot), p(wbad), FRAMES, M, d, N_ITER, _lib.F32, p(g1), st), 3),
    }
    for fn, _ in entries.values():
        _lib.check(fn())
    ems = alternate([fn for fn, _ in entries.values()], args.reps, args.warmup, 5 * args.inner)
    erows = [{"entry": name, "ms": t, "bytes": n * row_bytes, "hbm_peak_ms": n * row_bytes / HBM_PEAK * 1e3,
              "share_of_hbm_peak": n * row_bytes / HBM_PEAK * 1e3 / t} for (name, (_, n)), t in zip(entries.items(), ems)]
    lines = [f"lsp  frames={FRAMES} M={M} float32  {torch.cuda.get_device_name(0)}  (median of {args.reps} windows of {args.inner} calls, "
             f"hip and chain alternating; lspcheck rate {RATE}, n_iter {N_ITER})",
             "max |hip - chain|: " + "  ".join(f"{n} {v:.2e}" for n, v in diffs.items()),
             f"{'op':9s} {'':8s} {'hip ms':>9s} {'chain ms':>9s} {'chain/hip':>9s} {'MB moved':>9s} {'ms at 8 TB/s':>13s} {'share of peak':>13s}"]
    for r in rows:
        chain_ms = f"{r['chain_ms']:9.3f} {r['chain_ms'] / r['hip_ms']:9.1f}" if r["chain_ms"] is not None else f"{'-':>9s} {'-':>9s}"
        lines.append(f"{r['op']:9s} {r['what']:8s} {r['hip_ms']:9.4f} {chain_ms} {r['bytes'] / 1e6:9.2f} {r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f}")
    hip_us = next(r["hip_ms"] for r in rows if r["op"] == "lpc2lsp" and r["what"] == "fwd") * 1e3 / FRAMES
    lines.append("lpc2lsp by companion-matrix eigvals, forward, " + (f"{eig['frames']} frames: {eig['ms']:.1f} ms = {eig['us_per_frame']:.2f} us per frame "
                 f"(hip: {hip_us:.5f} us per frame; max |eig - hip| {eig['max_abs_diff_vs_hip']:.2e})" if "ms" in eig else eig["error"]))
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
                       "reps": args.reps, "inner": args.inner, "max_abs_diff": diffs, "rows": rows, "eigvals_route": eig, "entries": erows}, f, indent=1)


if __name__ == "__main__":
    main()
