#!/usr/bin/env python3
"""Timing of delta / mlpg / mcpf (csrc/paramgen.hip) at 1024 utterances of 200 frames, D = 25, the default windows, float32; mcpf at
M = 24, alpha = 0.42, beta = 0.2, ir_length = 128.  For mlpg also T = 1000, a single utterance of 1000 frames (B = 1: the sweep is a
dependent chain of length T with B D lanes of parallelism, so this one is bound by latency), and the cost of constructing the module.
Per operator forward and forward + backward.  Device time by HIP events around --inner calls, median of --reps windows after --warmup,
the two alternatives alternated window by window in one process:
  * hip    the library's entries through the public modules (one launch per direction);
  * chain  the reference's _forward restated with stock torch operators on the GPU: delta.py:181-201 (replicate pad, conv2d, permute),
           mlpg.py:165-171 (the einsum with a prebuilt dense (T, T H) matrix M), mcpf.py:191-209 (freqt, rfft, exp, hfft twice, mc2b,
           b2mc, every linear stage a matmul), its backward by autograd.  It is the yardstick: there is no earlier implementation here.
Construction is host time (time.perf_counter, median of three): the banded factor against the reference's loop over T, dense inverse
and product (mlpg.py:139-163), both in float64 on the host.

    python tools/time_paramgen.py [--reps 15] [--warmup 3] [--inner 10] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as NF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib  # noqa: E402
from diffsptk_amd.utils import tables  # noqa: E402
from time_parcor import HBM_PEAK, alternate  # noqa: E402

B, T, D, M = 1024, 200, 25, 24
SEED = [[-0.5, 0, 0.5], [1, -2, 1]]
ALPHA, BETA, ONSET, IR = 0.42, 0.2, 2, 128


def chain_delta(x, window):
    W = window.size(-1)
    x = NF.pad(x.unsqueeze(1), (0, 0, (W - 1) // 2, (W - 1) // 2), mode="replicate")
    y = NF.conv2d(x, window.view(-1, 1, W, 1), padding="valid")
    return y.permute(0, 2, 1, 3).reshape(y.size(0), y.size(2), -1)


def dense_mlpg_matrix(size, window, th):
    """M = (W^T W)^-1 W^T, (T, T H) float64 on the host, built as the reference builds it: a loop over T, a dense inverse, a product"""
    H, L = window.shape
    N = (L - 1) // 2
    W = torch.zeros(size * H, size, dtype=torch.float64)
    w, th = torch.from_numpy(window), torch.from_numpy(th.astype(np.float64)).unsqueeze(1)
    for t in range(size):
        rows = slice(H * t, H * t + H)
        if t < N:
            W[rows, :t + N + 1] = w[:, N - t:] * (th <= t)
        elif size < t + N + 1:
            W[rows, t - N:] = w[:, :size - t + N] * (th < size - t)
        else:
            W[rows, t - N:t + N + 1] = w
    return torch.linalg.inv(W.T @ W) @ W.T


def chain_mlpg(u, Mt):
    Tn = u.size(-2)
    return torch.einsum("...Td,tT->...td", u.reshape(*u.shape[:-2], Tn * (Mt.size(-1) // Tn), -1), Mt)


def chain_mcpf(mc, A, weight, to_b, to_mc, n):
    def energy(c):
        return torch.fft.hfft(torch.exp(2 * torch.fft.rfft(torch.matmul(c, A), n=n).real), norm="forward")[..., :1]

    mc2 = mc * weight
    b2 = torch.matmul(mc2, to_b)
    b2 = torch.cat([b2[..., :1] + 0.5 * torch.log(energy(mc) / energy(mc2)), b2[..., 1:]], -1)
    return torch.matmul(b2, to_mc)


def host_ms(fn, n=3):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


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

    def both(fn, inp, cot):
        def run():
            inp.grad = None
            fn(inp).backward(cot)
        return run

    def no_grad(fn, inp):
        def run():
            with torch.no_grad():
                fn(inp)
        return run

    def measure(op, shape, hip, chain, inp, least):
        with torch.no_grad():
            y = hip(inp)
            kernel = _lib.last_kernel()
            diff = float((y - chain(inp)).abs().max())
        leaf, cot = inp.clone().requires_grad_(), torch.randn(y.shape, device=dev, generator=g)
        for name, fns, nbytes in ((op, [no_grad(hip, inp), no_grad(chain, inp)], least),
                                  (op + " fwd+bwd", [both(hip, leaf, cot), both(chain, leaf, cot)], 2 * least)):
            hip_ms, chain_ms = alternate(fns, args.reps, args.warmup, args.inner)
            rows.append({"op": name, "shape": shape, "kernel": kernel, "hip_ms": hip_ms, "chain_ms": chain_ms, "least_bytes": nbytes,
                         "hbm_peak_ms": nbytes / HBM_PEAK * 1e3, "share_of_hbm_peak": nbytes / HBM_PEAK * 1e3 / hip_ms, "max_abs_diff_to_chain": diff})

    window, th = tables.delta_window(SEED), tables.mlpg_threshold(SEED)
    H = window.shape[0]
    # delta
    x = torch.randn(args.batch, T, D, device=dev, generator=g)
    delta = dsp.Delta(SEED, device=dev)
    wdev = torch.from_numpy(window).to(dev, torch.float32)
    measure("delta", f"B={args.batch} T={T} D={D}", delta, lambda t: chain_delta(t, wdev), x, 4 * x.numel() * (1 + H))
    # mlpg: the batch, a batch of long utterances, a single long utterance
    for Bn, Tn in ((args.batch, T), (args.batch, 1000), (1, 1000)):
        u = torch.randn(Bn, Tn, D * H, device=dev, generator=g)
        mlpg = dsp.MLPG(Tn, SEED, device=dev)
        Mt = dense_mlpg_matrix(Tn, window, th).to(dev, torch.float32)
        measure("mlpg", f"B={Bn} T={Tn} D={D}", mlpg, lambda t: chain_mlpg(t, Mt), u, 4 * u.numel() // H * (1 + H))
    # mcpf
    mc = torch.randn(args.batch * T, M + 1, device=dev, generator=g) * (0.5 * torch.exp(-torch.arange(M + 1, device=dev) / 6.0))
    mc[:, 0] += 2
    mcpf = dsp.MelCepstrumPostfiltering(M, ALPHA, BETA, ONSET, IR, device=dev)
    A = torch.from_numpy(tables.freqt_matrix(M, IR - 1, -ALPHA)).to(dev, torch.float32)
    weight = torch.full((M + 1,), 1 + BETA, device=dev)
    weight[:ONSET] = 1
    to_b, to_mc = (torch.from_numpy(f(M, ALPHA)).to(dev, torch.float32) for f in (tables.mc2b_matrix, tables.b2mc_matrix))
    measure("mcpf", f"frames={args.batch * T} M={M} ir_length={IR}", mcpf, lambda t: chain_mcpf(t, A, weight, to_b, to_mc, IR), mc, 8 * mc.numel())
    # construction on the host
    build = []
    for Tn in (T, 1000, 2000):
        build.append({"T": Tn, "factor_ms": host_ms(lambda: tables.mlpg_factor(Tn, window, th)),
                      "dense_ms": host_ms(lambda: dense_mlpg_matrix(Tn, window, th)), "factor_bytes": 4 * Tn * window.shape[1], "dense_bytes": 4 * Tn * Tn * H})

    lines = [f"paramgen  float32  {torch.cuda.get_device_name(0)}  (device events, median of {args.reps} windows of {args.inner} calls, hip and chain "
             f"alternated; least traffic: the operands once; HBM peak {HBM_PEAK / 1e12:.1f} TB/s)",
             f"{'operation':14s} {'shape':36s} {'kernel':17s} {'hip ms':>9s} {'chain ms':>9s} {'chain/hip':>9s} {'least MB':>9s} {'ms at peak':>10s} "
             f"{'share of peak':>13s} {'|hip - chain|':>13s}"]
    for r in rows:
        lines.append(f"{r['op']:14s} {r['shape']:36s} {r['kernel']:17s} {r['hip_ms']:9.4f} {r['chain_ms']:9.4f} {r['chain_ms'] / r['hip_ms']:9.2f} "
                     f"{r['least_bytes'] / 1e6:9.2f} {r['hbm_peak_ms']:10.4f} {r['share_of_hbm_peak']:13.3f} {r['max_abs_diff_to_chain']:13.2e}")
    lines.append("construction of MLPG on the host (float64, median of three): the banded Cholesky factor against the reference's dense matrix")
    for r in build:
        lines.append(f"  T={r['T']:5d}  factor {r['factor_ms']:9.2f} ms, {r['factor_bytes'] / 1e3:9.1f} kB in float32    dense {r['dense_ms']:9.2f} ms, "
                     f"{r['dense_bytes'] / 1e6:8.2f} MB in float32")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows, "construction": build}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
