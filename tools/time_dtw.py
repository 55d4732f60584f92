#!/usr/bin/env python3
"""Timing of DynamicTimeWarping (csrc/dtw.hip): 256 pairs of D = 25 at T1 = T2 = 200 and at T1 = T2 = 1000, float32, p = 4,
softness 1e-3 -- the distance alone (no tables stored) and the distance with its gradient (tables stored, the reverse sweep).
  * hip    the public functional: device time by HIP events around --inner calls, median of --reps windows after --warmup;
  * chain  the reference's algorithm (dtw.py:26-125 at p = 4) restated here with stock torch operators, vectorised over the batch AND
           over the anti-diagonal -- (B, T1) tensors, T1 + T2 - 1 steps of about thirty launches, the gradient by autograd.  This is
           what one would write without a kernel; the fair yardstick.  Host clock around a synchronise, median of --chain-reps runs;
  * cells  the reference's own cell-by-cell loop (one-element tensor operations, T1 T2 Python iterations) at B = 1, T = 100, once.
Both yardsticks live in this tool, not in the library.  Also timed: one pair of T = 1000 alone (a single workgroup), and the path.

    python tools/time_dtw.py [--reps 9] [--warmup 2] [--inner 10] [--chain-reps 3] [--txt profiles/dtw_time_v1.txt] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd.functional as F  # noqa: E402
from time_parcor import alternate  # noqa: E402

B, D, P, GAMMA = 256, 25, 4, 1e-3
INF = float("inf")


def softmin(c, gamma):
    """-gamma logsumexp(-c / gamma) over dim 0 with +inf candidates left out, +inf where there is none; safe under autograd"""
    m = c.min(0).values
    none = m == INF
    shift = torch.where(none, torch.zeros_like(m), m)
    e = torch.where(c == INF, torch.zeros_like(c), torch.exp(-(torch.where(c == INF, shift.expand_as(c), c) - shift) / gamma))
    total = torch.where(none, torch.ones_like(m), e.sum(0))
    return torch.where(none, torch.full_like(m, INF), shift - gamma * torch.log(total))


def chain_dtw(x, y, gamma=GAMMA):
    """p = 4 by anti-diagonals: the steps (1,0) and (0,1) read R_ of diagonal s - 1, (1,1) reads R of diagonal s - 2 and alone makes R_"""
    T1, T2 = x.size(1), y.size(1)
    dist = torch.cdist(x, y)
    rows = torch.arange(T1, device=x.device)
    blank = torch.full((x.size(0), T1), INF, device=x.device, dtype=x.dtype)
    up = lambda v: torch.cat([blank[:, :1], v[:, :-1]], 1)   # noqa: E731   row i - 1
    r1, r2, q1 = blank, blank, blank
    for s in range(T1 + T2 - 1):
        j = s - rows
        inside = (j >= 0) & (j < T2)
        d = dist[:, rows, j.clamp(0, T2 - 1)]
        if s == 0:
            r0, q0 = torch.where(inside, d, blank), blank
        else:
            q0 = torch.where(inside, 2 * d + up(r2), blank)
            r0 = torch.where(inside, softmin(torch.stack([d + up(q1), d + q1, q0]), gamma), blank)
        r1, r2, q1 = r0, r1, q0
    return r1[:, -1] / (T1 + T2)


def cells_dtw(x, y, gamma=GAMMA):
    """the reference's loop over the cells at p = 4, B = 1 (dtw.py:44-104 without the back-pointers)"""
    dist = torch.cdist(x, y)
    T1, T2 = dist.shape[1:]
    R = torch.full_like(dist, INF)
    Q = R.clone()
    R[:, 0, 0] = dist[:, 0, 0]
    for i in range(T1):
        for j in range(T2):
            rs, qs = [], []
            d = dist[:, i, j]
            for a, b in ((1, 0), (0, 1), (1, 1)):
                if i - a < 0 or j - b < 0:
                    continue
                if a == 0 or b == 0:
                    if Q[:, i - a, j - b] != INF:
                        rs.append(d * (a + b) + Q[:, i - a, j - b])
                elif R[:, i - a, j - b] != INF:
                    rs.append(d * (a + b) + R[:, i - a, j - b])
                    qs.append(rs[-1])
            if rs:
                R[:, i, j] = -gamma * torch.logsumexp(-torch.stack(rs) / gamma, 0)
            if qs:
                Q[:, i, j] = -gamma * torch.logsumexp(-torch.stack(qs) / gamma, 0)
    return R[:, -1, -1] / (T1 + T2)


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def sequences(batch, T, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    walk = lambda: 0.05 * torch.randn(batch, T, D, device=dev, generator=g).cumsum(1) + 0.1 * torch.randn(batch, T, D, device=dev, generator=g)   # noqa: E731
    return walk(), walk()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--chain-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dtw_time_v1.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for T in (200, 1000):
        x, y = sequences(B, T, T, dev)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

        def hip_fwd():
            return F.dtw(x, y, p=P, softness=GAMMA)

        def hip_both():
            xg.grad = yg.grad = None
            F.dtw(xg, yg, p=P, softness=GAMMA).sum().backward()

        def chain_both():
            xg.grad = yg.grad = None
            chain_dtw(xg, yg).sum().backward()

        with torch.no_grad():
            a, b = hip_fwd(), chain_dtw(x, y)
        hip_both()
        ga = xg.grad.clone()
        chain_both()
        diff = (float((a - b).abs().max()), float((ga - xg.grad).abs().max()), float(a.abs().max()), float(ga.abs().max()))
        fwd_ms, both_ms = alternate([hip_fwd, hip_both], args.reps, args.warmup, args.inner)
        with torch.no_grad():
            chain_fwd_ms = host_ms(lambda: chain_dtw(x, y), args.chain_reps)
        chain_both_ms = host_ms(chain_both, args.chain_reps)
        cells = B * T * T
        rows.append({"T": T, "hip_fwd_ms": fwd_ms, "hip_fwd_bwd_ms": both_ms, "chain_fwd_ms": chain_fwd_ms, "chain_fwd_bwd_ms": chain_both_ms,
                     "cells": cells, "fwd_ns_per_cell": fwd_ms * 1e6 / cells, "fwd_us_per_diagonal": fwd_ms * 1e3 / (2 * T - 1),
                     "max_distance_diff": diff[0], "max_gx_diff": diff[1], "max_distance": diff[2], "max_gx": diff[3]})
        del xg, yg
    # one long pair: a single workgroup
    x1, y1 = sequences(1, 1000, 7, dev)
    one_ms = alternate([lambda: F.dtw(x1, y1, p=P, softness=GAMMA)], args.reps, args.warmup, args.inner)[0]
    with torch.no_grad():
        one_chain_ms = host_ms(lambda: chain_dtw(x1, y1), args.chain_reps)
    # the path on top of the distance (tables stored, one thread per pair traces, one host read)
    x2, y2 = sequences(B, 200, 9, dev)
    path_ms = host_ms(lambda: F.dtw(x2, y2, return_indices=True, p=P, softness=GAMMA), 5)
    # the reference's loop, once
    xc, yc = sequences(1, 100, 11, dev)
    xc.requires_grad_(True)
    t0 = time.perf_counter()
    dc = cells_dtw(xc, yc)
    torch.cuda.synchronize()
    cells_fwd_s = time.perf_counter() - t0
    dc.sum().backward()
    torch.cuda.synchronize()
    cells_both_s = time.perf_counter() - t0
    with torch.no_grad():
        cells_diff = float((dc - F.dtw(xc, yc, p=P, softness=GAMMA)).abs().max())

    lines = [f"dtw  pairs={B} D={D} p={P} softness={GAMMA} float32  {torch.cuda.get_device_name(0)}  (hip: device events, median of {args.reps} windows of "
             f"{args.inner} calls; chain: host clock around a synchronise, median of {args.chain_reps})",
             f"{'T1=T2':>6s} {'hip fwd ms':>11s} {'hip fwd+bwd ms':>15s} {'chain fwd ms':>13s} {'chain fwd+bwd ms':>17s} {'chain/hip fwd':>14s} {'chain/hip f+b':>14s} "
             f"{'ns per cell':>12s} {'us per diagonal':>16s} {'max |d diff|':>13s} {'max |gx diff|':>14s}"]
    for r in rows:
        lines.append(f"{r['T']:6d} {r['hip_fwd_ms']:11.3f} {r['hip_fwd_bwd_ms']:15.3f} {r['chain_fwd_ms']:13.1f} {r['chain_fwd_bwd_ms']:17.1f} "
                     f"{r['chain_fwd_ms'] / r['hip_fwd_ms']:14.0f} {r['chain_fwd_bwd_ms'] / r['hip_fwd_bwd_ms']:14.0f} {r['fwd_ns_per_cell']:12.4f} "
                     f"{r['fwd_us_per_diagonal']:16.3f} {r['max_distance_diff']:13.2e} {r['max_gx_diff']:14.2e}")
    lines.append(f"one pair of T = 1000 (one workgroup): hip fwd {one_ms:.3f} ms, chain fwd {one_chain_ms:.1f} ms")
    lines.append(f"distance + paths, {B} pairs of T = 200 (host clock, one read of the counts): {path_ms:.3f} ms")
    lines.append(f"the reference's cell loop restated, B = 1, T = 100, once: forward {cells_fwd_s:.2f} s, forward + backward {cells_both_s:.2f} s "
                 f"(|distance - hip| = {cells_diff:.2e})")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "pairs": B, "D": D, "p": P, "softness": GAMMA, "dtype": "float32", "rows": rows,
                       "one_pair_T1000": {"hip_fwd_ms": one_ms, "chain_fwd_ms": one_chain_ms}, "paths_T200_ms": path_ms,
                       "cell_loop_T100": {"fwd_s": cells_fwd_s, "fwd_bwd_s": cells_both_s, "distance_diff": cells_diff}}, f, indent=1)


if __name__ == "__main__":
    main()
