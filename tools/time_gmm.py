#!/usr/bin/env python3
"""Timing of GaussianMixtureModeling (csrc/gmm.hip): T = 100 000 vectors, L in {25, 50}, K in {16, 64}, the diagonal and the full route,
float32.
  * hip step     one EM iteration (ops.gmm_em_step: factorisation, E-step, its total, moment sums, M-step; no host read): device time
                 by HIP events around --inner calls, median of --reps windows after --warmup;
  * hip kernels  the same iteration launch by launch (each timed alone, the same way): what the iteration is made of;
  * hip forward  GaussianMixtureModeling.forward with n_iter = 10 and eps = 0 (ten iterations, one small host read each): host clock
                 around a synchronise, median of --chain-reps runs;
  * chain        the reference's iteration (gmm.py:299-378 and 434-486) restated here with stock torch operators on the device, with
                 its data flow: the broadcast matmuls of the E-step, outer(x) of T L^2 values and the einsum of the second moments.
                 Host clock around a synchronise, median of --chain-reps runs.  If it does not fit in memory at T it is timed at half T,
                 and so on; the row says at which T.
The yardstick lives in this tool, not in the library.

    python tools/time_gmm.py [--reps 7] [--warmup 2] [--inner 5] [--chain-reps 3] [--txt profiles/gmm_time_v1.txt] [--json out.json]
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


def chain_step(x, w, mu, sigma, diag, weight_floor=1e-5, var_floor=1e-6):
    """one iteration with the reference's operators and intermediates; returns (w, mu, sigma, log-likelihood)"""
    n, L = x.shape
    K = w.numel()
    diff = x.unsqueeze(1) - mu.unsqueeze(0)
    if diag:
        var = sigma.diagonal(dim1=-2, dim2=-1)
        log_det = var.log().sum(-1)
        maha = (diff ** 2 * var.reciprocal()).sum(-1)
    else:
        col = torch.linalg.cholesky(sigma)
        log_det = col.diagonal(dim1=-2, dim2=-1).log().sum(-1) * 2
        precision = torch.cholesky_inverse(col).unsqueeze(0)
        right = torch.matmul(precision, diff.unsqueeze(-1))
        maha = torch.matmul(diff.unsqueeze(-2), right).squeeze(-1).squeeze(-1)
    numer = w.log() - 0.5 * (L * math.log(2 * math.pi) + log_det + maha)
    denom = torch.logsumexp(numer, dim=-1, keepdim=True)
    post = torch.exp(numer - denom)
    z = post.sum(0)
    neww = torch.clip(z / n, min=weight_floor)
    a = (1 - weight_floor * K) / (neww.sum() - weight_floor * K)
    neww = a * neww + weight_floor * (1 - a)
    newmu = torch.matmul(post.t(), x) / z.view(-1, 1)
    if diag:
        var = torch.matmul(post.t(), x ** 2) / z.view(-1, 1) - newmu ** 2
        newsigma = sigma.clone()
        newsigma.diagonal(dim1=-2, dim2=-1).copy_(var.clip(min=var_floor))
    else:
        xx = x.unsqueeze(-1) * x.unsqueeze(-2)
        newsigma = torch.einsum("bk,blm->klm", post, xx) / z.view(-1, 1, 1) - newmu.unsqueeze(-1) * newmu.unsqueeze(-2)
        newsigma.diagonal(dim1=-2, dim2=-1).clip_(min=var_floor)
    return neww, newmu, newsigma, denom.sum()


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
    init = (torch.full((K,), 1.0 / K, device=dev), centres + 0.3 * torch.randn(K, L, device=dev, generator=g) / math.sqrt(L),
            (1.3 * torch.eye(L, device=dev)).repeat(K, 1, 1))
    return x, init


def kernel_fns(x, w, mu, sigma, mask, diag):
    """the five launches of one iteration, each on buffers of its own"""
    n, L = x.shape
    K, code, dev, dt = w.numel(), _dtype_code(x), x.device, x.dtype
    prec = torch.empty(K, L if diag else L * L, device=dev, dtype=dt)
    cst, failed = torch.empty(K, device=dev, dtype=dt), torch.empty(K, device=dev, dtype=torch.int32)
    post, ll = torch.empty(n, K, device=dev, dtype=dt), torch.empty(n, device=dev, dtype=dt)
    rows = dsp._lib.GMM_TILE_BYTES // x.element_size()
    partial = torch.empty((n + rows - 1) // rows, device=dev, dtype=torch.float64)
    ws = torch.empty(dsp._lib.load().dsa_gmm_accum_workspace_bytes(n, K, L, int(diag), code) // x.element_size(), device=dev, dtype=dt)
    w2, mu2, sigma2 = w.clone(), mu.clone(), sigma.clone()
    fns = {
        "prepare": lambda: _call("dsa_gmm_prepare", _p(w), _p(sigma), K, L, L, int(diag), code, _p(prec), _p(cst), _p(failed), _stream()),
        "estep": lambda: _call("dsa_gmm_estep", _p(x), _p(mu), _p(prec), _p(cst), _p(failed), n, K, L, L, int(diag), code, _p(post), _p(ll), _p(partial),
                               None, None, _stream()),
        "accum": lambda: _call("dsa_gmm_accum", _p(x), _p(post), n, K, L, int(diag), code, _p(ws), _stream()),
        "update": lambda: _call("dsa_gmm_update", _p(ws), None, None, None, None, _p(mask), n, K, L, int(diag), 0.0, 1e-5, 1e-6, code, _p(w2), _p(mu2),
                                _p(sigma2), _stream()),
    }
    for fn in fns.values():   # in order once: every launch then has its inputs
        fn()
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--chain-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gmm_time_v1.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for diag in (True, False):
        for L in (25, 50):
            for K in (16, 64):
                x, init = problem(L, K, T, dev)
                gmm = dsp.GMM(L - 1, K, n_iter=10, eps=0.0, var_type="diag" if diag else "full", device=dev)
                readback = torch.empty(2, device=dev, dtype=torch.float64)

                def step():
                    w, mu, sigma = (t.clone() for t in init)
                    return ops.gmm_em_step(x, w, mu, sigma, gmm.mask, None, diag, 0.0, 1e-5, 1e-6, readback), (w, mu, sigma)

                def forward():
                    gmm.w, gmm.mu, gmm.sigma = (t.clone() for t in init)   # (rebound, not set_params: trained buffers are inference tensors)
                    return gmm(x)

                fns = kernel_fns(x, *init, gmm.mask, diag)
                step_ms, *kernel_ms = alternate([lambda: step()] + list(fns.values()), args.reps, args.warmup, args.inner)
                forward_ms = host_ms(forward, args.chain_reps)
                ll, (w1, mu1, sigma1) = step()
                n, chain_ms, diff = T, None, None
                while n >= 1000:
                    try:
                        got = chain_step(x[:n], *init, diag)
                        torch.cuda.synchronize()
                        if n == T:
                            diff = (float((got[0] - w1).abs().max()), float((got[1] - mu1).abs().max()), float((got[2] - sigma1).abs().max()),
                                    float((got[3] - ll).abs() / ll.abs()))
                        del got
                        chain_ms = host_ms(lambda: chain_step(x[:n], *init, diag), args.chain_reps)
                        break
                    except torch.cuda.OutOfMemoryError:
                        torch.cuda.empty_cache()
                        n //= 2
                    except RuntimeError as e:   # the stock operator is not available on this build
                        chain_ms, diff = None, str(e).splitlines()[0][:80]
                        break
                rows.append({"route": "diag" if diag else "full", "L": L, "K": K, "T": T, "hip_step_ms": step_ms,
                             "hip_kernels_ms": dict(zip(fns, kernel_ms)), "hip_forward10_ms": forward_ms, "chain_T": n, "chain_step_ms": chain_ms,
                             "diff_w_mu_sigma_loglik": diff})
                print(rows[-1], flush=True)
                del x, init, gmm, fns
                torch.cuda.empty_cache()

    lines = [f"gmm  T={T} float32  {torch.cuda.get_device_name(0)}  (hip step and kernels: device events, median of {args.reps} windows of {args.inner} "
             f"calls; forward of 10 iterations and chain: host clock around a synchronise, median of {args.chain_reps})",
             f"{'route':>5s} {'L':>3s} {'K':>3s} {'hip step ms':>12s} {'prepare':>8s} {'estep':>8s} {'accum':>8s} {'update':>8s} {'forward10 ms':>13s} "
             f"{'chain step ms':>14s} {'chain T':>8s} {'chain/hip':>10s}  max |diff| of w, mu, sigma; relative of the log-likelihood"]
    for r in rows:
        k = r["hip_kernels_ms"]
        chain = "n/a" if r["chain_step_ms"] is None else f"{r['chain_step_ms']:.2f}"
        ratio = "n/a" if r["chain_step_ms"] is None else f"{r['chain_step_ms'] * (T / r['chain_T']) / r['hip_step_ms']:.1f}"
        diff = r["diff_w_mu_sigma_loglik"]
        diff = diff if isinstance(diff, str) or diff is None else " ".join(f"{d:.1e}" for d in diff)
        lines.append(f"{r['route']:>5s} {r['L']:3d} {r['K']:3d} {r['hip_step_ms']:12.3f} {k['prepare']:8.3f} {k['estep']:8.3f} {k['accum']:8.3f} "
                     f"{k['update']:8.3f} {r['hip_forward10_ms']:13.2f} {chain:>14s} {r['chain_T']:8d} {ratio:>10s}  {diff}")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "T": T, "dtype": "float32", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
