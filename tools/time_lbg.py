#!/usr/bin/env python3
"""Timing of the vector quantiser and of LindeBuzoGrayAlgorithm (csrc/vq.hip): T = 100 000 vectors, L in {25, 50}, K in {16, 64, 1024},
float32.
  * hip step     one iteration (ops.lbg_step: search, accumulation, update; no host read): device time by HIP events around --inner
                 calls, median of --reps windows after --warmup;
  * hip kernels  the same iteration launch by launch (each timed alone, the same way);
  * chain step   the reference's iteration (lbg.py:214-285) restated here with stock torch operators on the device, float32: cdist,
                 argmin, the distance, bincount, scatter_add_ and the masked division, over all T vectors at once.  Timed the same way.
                 The yardstick lives in this tool, not in the library;
  * f32 search   torch.cdist + argmin alone, float32: what a search that does not form its sums in float64 costs, and `agree`, the share
                 of the vectors it assigns as the float64 search does;
  * f64 share    the search's 3 T K L floating-point operations (difference, product, sum) per second, against the chip's float64
                 vector rate of --peak-tflops (78.6: the MI355X data sheet);
  * design       LindeBuzoGrayAlgorithm.forward to K = 64 (n_iter = 20, eps = 1e-5, seed 0; one small host read per iteration): host
                 clock around a synchronise, median of --chain-reps runs, with the iterations it ran.

    python tools/time_lbg.py [--reps 7] [--warmup 2] [--inner 5] [--chain-reps 3] [--txt profiles/lbg_time_v1.txt] [--json out.json]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import ops  # noqa: E402
from diffsptk_amd.ops._core import _call, _dtype_code, _p, _stream  # noqa: E402
from time_parcor import alternate  # noqa: E402

T = 100_000


def chain_step(x, codebook, min_data=1):
    """one iteration with stock operators; returns (centroids, indices, distance)"""
    K, L = codebook.shape
    indices = torch.cdist(x, codebook).argmin(1)
    distance = (x - codebook[indices]).square().sum() / x.size(0)
    n_data = torch.bincount(indices, minlength=K).to(x.dtype)
    centroids = torch.zeros(K, L, device=x.device, dtype=x.dtype).scatter_add_(0, indices.unsqueeze(1).expand(-1, L), x)
    keep = n_data >= min_data
    centroids = torch.where(keep.unsqueeze(1), centroids / n_data.clamp(min=1).unsqueeze(1), torch.zeros((), device=x.device))
    return centroids, indices, distance


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def problem(L, K, n, dev):
    g = torch.Generator(device=dev).manual_seed(L * 1000 + K)
    centres = torch.randn(K, L, device=dev, generator=g) * 2.5 / math.sqrt(L)
    x = centres[torch.randint(0, K, (n,), device=dev, generator=g)] + torch.randn(n, L, device=dev, generator=g)
    return x, (centres + 0.3 * torch.randn(K, L, device=dev, generator=g) / math.sqrt(L)).contiguous()


def kernel_fns(x, codebook):
    """the three launches of one iteration, each on buffers of its own"""
    n, L = x.shape
    K, code, dev = codebook.size(0), _dtype_code(x), x.device
    indices = torch.empty(n, device=dev, dtype=torch.int64)
    rows = dsp._lib.VQ_TILE_BYTES // x.element_size()
    partial = torch.empty((n + rows - 1) // rows, device=dev, dtype=torch.float64)
    ws = torch.empty(dsp._lib.load().dsa_vq_accum_workspace_bytes(n, K, L) // 8, device=dev, dtype=torch.float64)
    n_data, pending = torch.empty(K, device=dev, dtype=torch.int64), torch.empty(K, L, device=dev)
    readback = torch.empty(3, device=dev, dtype=torch.float64)
    fns = {
        "search": lambda: _call("dsa_vq_search", _p(x), _p(codebook), n, K, L, code, _p(indices), None, _p(partial), None, 0.0, _stream()),
        "accum": lambda: _call("dsa_vq_accum", _p(x), _p(indices), n, K, L, code, _p(ws), _stream()),
        "update": lambda: _call("dsa_vq_update", _p(ws), _p(partial), partial.numel(), n, K, L, 1, _p(n_data), _p(pending), _p(readback), _stream()),
    }
    for fn in fns.values():   # in order once: every launch then has its inputs
        fn()
    return fns, indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--chain-reps", type=int, default=3)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lbg_time_v1.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for L in (25, 50):
        for K in (16, 64, 1024):
            x, codebook = problem(L, K, T, dev)
            readback = torch.empty(3, device=dev, dtype=torch.float64)
            fns, indices = kernel_fns(x, codebook)
            step_ms, chain_ms, f32_ms, *kernel_ms = alternate([lambda: ops.lbg_step(x, codebook, 1, readback), lambda: chain_step(x, codebook),
                                                               lambda: torch.cdist(x, codebook).argmin(1)] + list(fns.values()),
                                                              args.reps, args.warmup, args.inner)
            _, pending, _ = ops.lbg_step(x, codebook, 1, readback)
            centroids, chain_idx, chain_d = chain_step(x, codebook)
            k = dict(zip(fns, kernel_ms))
            rows.append({"L": L, "K": K, "T": T, "hip_step_ms": step_ms, "hip_kernels_ms": k, "chain_step_ms": chain_ms, "f32_search_ms": f32_ms,
                         "f64_tflops": 3.0 * T * K * L / (k["search"] * 1e-3) / 1e12, "agree": float((chain_idx == indices).double().mean()),
                         "diff_centroids_distance": [float((centroids - pending).abs().max()), abs(float(chain_d) - float(readback[0]))]})
            print(rows[-1], flush=True)
            del x, codebook, fns
            torch.cuda.empty_cache()

    designs = []
    for L in (25, 50):
        x, _ = problem(L, 64, T, dev)
        made = []

        def design():
            lbg = dsp.LBG(L - 1, 64, n_iter=20, seed=0, device=dev)
            lbg(x)
            made.append(sum(len(d) for d in lbg.distances))

        designs.append({"L": L, "K": 64, "ms": host_ms(design, args.chain_reps), "iterations": made[-1]})
        print(designs[-1], flush=True)

    lines = [f"lbg  T={T} float32  {torch.cuda.get_device_name(0)}  (device events, median of {args.reps} windows of {args.inner} calls; design: host clock "
             f"around a synchronise, median of {args.chain_reps})",
             f"{'L':>3s} {'K':>5s} {'hip step ms':>12s} {'search':>8s} {'accum':>8s} {'update':>8s} {'chain step ms':>14s} {'chain/hip':>10s} {'f32 cdist+argmin':>17s} "
             f"{'search/f32':>11s} {'f64 TFLOP/s':>12s} {'share':>6s} {'agree':>9s}  max |diff| of the centroids, |diff| of the distance"]
    for r in rows:
        k = r["hip_kernels_ms"]
        lines.append(f"{r['L']:3d} {r['K']:5d} {r['hip_step_ms']:12.3f} {k['search']:8.3f} {k['accum']:8.3f} {k['update']:8.3f} {r['chain_step_ms']:14.3f} "
                     f"{r['chain_step_ms'] / r['hip_step_ms']:10.2f} {r['f32_search_ms']:17.3f} {k['search'] / r['f32_search_ms']:11.2f} {r['f64_tflops']:12.2f} "
                     f"{r['f64_tflops'] / args.peak_tflops:6.3f} {r['agree']:9.6f}  {r['diff_centroids_distance'][0]:.1e} {r['diff_centroids_distance'][1]:.1e}")
    lines += [f"design to K = 64, L = {d['L']}: {d['ms']:.2f} ms for {d['iterations']} iterations ({d['ms'] / d['iterations']:.3f} ms each, host read included)"
              for d in designs]
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "T": T, "dtype": "float32", "rows": rows, "designs": designs}, f, indent=1)


if __name__ == "__main__":
    main()
