#!/usr/bin/env python3
"""Timing of PLP (csrc/plp.hip) at the bench size: 1024 utterances x 1 s at 16 kHz through STFT(400, 80, 512), i.e. 204 800 frames
(200 per utterance), PLP(fft 512, C = 20, M = 12, lifter 22, n_fft 512), float32.  Device time by HIP events, median of --reps after
--warmup:
  * dsa_plp_fwd and dsa_plp_bwd alone (on filter-bank outputs already in memory);
  * plp(stft(x)) and fuse(stft, plp)(x), forward and forward + backward (gradient for the waveform);
  * the baseline: the reference's plp.py:312-320 chain from this library's existing entries (STFT, filter bank, LevinsonDurbin,
    mgc2mgc) and stock torch operators (exp, pow, replicate, hfft, lifter, cat).

    python tools/time_plp.py [--reps 20] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib, ops  # noqa: E402


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
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    B, T, C, M, N = 1024, 16000, 20, 12, 512
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, T, device=dev, generator=g) * 0.1
    stft = dsp.STFT(400, 80, 512, device=dev)
    plp = dsp.PLP(fft_length=512, plp_order=M, n_channel=C, sample_rate=16000, lifter=22, out_format="yc", device=dev)
    fused = dsp.fuse(stft, plp)
    # baseline pieces (plp.py:247-300 with this library's modules)
    fbank = dsp.MelFilterBankAnalysis(fft_length=512, n_channel=C, sample_rate=16000, use_power=True, out_format="y,E", device=dev)
    levdur = dsp.LevinsonDurbin(M, eps=0, device=dev)
    lpc2c = dsp.MelGeneralizedCepstrumToMelGeneralizedCepstrum(M, M, in_gamma=-1, in_norm=True, in_mul=True, n_fft=N, device=dev)
    J = N // 2 + 1
    q, lift = torch.split(plp.table, [C, (C + 2) * (M + 1) + 2 * (M + 1) * J + J, M + 1])[::2]

    def baseline(X):
        y, E = fbank(X)
        y = (torch.exp(y) * q) ** 0.33
        y = torch.cat((y[..., :1], y, y[..., -1:]), dim=-1)
        y = torch.fft.hfft(y, norm="forward").real[..., : M + 1]
        y = lpc2c(levdur(y)) * lift
        c, y = torch.split(y, [1, M], dim=-1)
        return torch.cat((y, c), dim=-1)

    with torch.no_grad():
        X = stft(x)
        y, E = ops.FbankFn.apply(X, plp.H, 1e-5, 0.0, True)
    Fr = y.numel() // C
    out = torch.empty(Fr, M + 1, device=dev)
    save = torch.empty(Fr, M + 1, device=dev)
    gout = torch.randn(Fr, M + 1, device=dev, generator=g)
    gy = torch.empty(Fr, C, device=dev)
    tab = plp.table

    def plp_fwd():
        _lib.check(_lib.load().dsa_plp_fwd(y.data_ptr(), None, Fr, C, M, N, 0.33, 2, tab.data_ptr(), _lib.F32, out.data_ptr(),
                                           save.data_ptr(), ops._stream()), "dsa_plp_fwd")

    def plp_bwd():
        _lib.check(_lib.load().dsa_plp_bwd(gout.data_ptr(), y.data_ptr(), save.data_ptr(), Fr, C, M, N, 0.33, 2, tab.data_ptr(),
                                           _lib.F32, gy.data_ptr(), None, ops._stream()), "dsa_plp_bwd")

    plp_fwd()
    # the baseline's and the kernel's results agree (a sanity check of the timed chains)
    with torch.no_grad():
        ref = baseline(X)
        e = float((plp(X) - ref).abs().max())
        e_fused = float((fused(x) - ref).abs().max())
        del ref
    xg = x.clone().requires_grad_(True)
    gz = torch.randn(B, Fr // B, M + 1, device=dev, generator=g)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn(x)
        return run

    def with_grad(fn):
        def run():
            xg.grad = None
            fn(xg).backward(gz)
        return run

    rows = {
        "dsa_plp_fwd": timed(plp_fwd, args.reps, args.warmup),
        "dsa_plp_bwd": timed(plp_bwd, args.reps, args.warmup),
        "plp(stft(x)) fwd": timed(no_grad(lambda t: plp(stft(t))), args.reps, args.warmup),
        "plp(stft(x)) fwd+bwd": timed(with_grad(lambda t: plp(stft(t))), args.reps, args.warmup),
        "fuse(stft, plp) fwd": timed(no_grad(fused), args.reps, args.warmup),
        "fuse(stft, plp) fwd+bwd": timed(with_grad(fused), args.reps, args.warmup),
        "baseline fwd": timed(no_grad(lambda t: baseline(stft(t))), args.reps, args.warmup),
        "baseline fwd+bwd": timed(with_grad(lambda t: baseline(stft(t))), args.reps, args.warmup),
    }
    assert fused.last_path == "fused"
    print(f"plp  B={B} T={T} frames={Fr} fft 512 C={C} M={M} n_fft={N} lifter 22 float32  (median of {args.reps})")
    print(f"max |plp - baseline| = {e:.2e}, max |fuse - baseline| = {e_fused:.2e}")
    for k, v in rows.items():
        print(f"{k:26s} {v:8.3f} ms")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "B": B, "T": T, "frames": Fr, "C": C, "M": M, "n_fft": N,
                       "max_abs_diff_vs_baseline": e, "max_abs_diff_fused_vs_baseline": e_fused, "ms": rows}, f, indent=1)


if __name__ == "__main__":
    main()
