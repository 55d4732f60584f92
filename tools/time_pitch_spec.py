#!/usr/bin/env python3
"""Timing of PitchAdaptiveSpectralAnalysis (csrc/pitch_spec.hip): --batch utterances of --seconds at 48 kHz, frame period 240,
fft_length 2048 (the Aperiodicity workload of tools/bench_ap.py), float32 and float64; a harmonic signal with noise, F0 between 100 and
300 Hz with unvoiced runs.
  * the module's forward and forward + backward, its two randn draws included: device time by HIP events around a window of enqueued
    calls, the median of --reps windows, after a 0.3 s clock ramp (as tools/bench_ap.py);
  * the three entries on their own, with the noise made once outside the windows;
  * the reference's forward restated from stock torch operators on the device (`stock` below: unfold, rfft, gather, cumsum, irfft, hfft,
    with its host read of the widest boundary), forward and forward + backward through autograd, and how far its float64 result is from
    the kernel's with the same noise;
  * the peak memory of a forward + backward, both ways.

    python tools/time_pitch_spec.py [--reps 10] [--inner 5] [--window-ms 30] [--batch 8] [--seconds 10] [--txt profiles/pitch_spec_time_v1.txt]
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib, ops  # noqa: E402
from diffsptk_amd.modules.spec import device_twiddle  # noqa: E402


def stock(x, f0, P, sr, L, noise=None, default_f0=500.0, q1=-0.15, noise_eps=None):
    """The CheapTrick envelope from stock torch operators, power format; noise: (noise1, noise2) or None for two randn_like draws"""
    K, rate, f_min = L // 2 + 1, sr / L, 3 * sr / (L - 3)
    f = torch.where(f0 <= f_min, default_f0, f0).unsqueeze(-1)
    ramp = torch.arange(L, device=x.device, dtype=x.dtype)
    j = ramp - L // 2
    inside = j.abs() <= torch.round(1.5 * sr / f)
    w = (0.5 + 0.5 * torch.cos(torch.pi * (j / (1.5 * sr)) * f)) * inside
    w = w / torch.linalg.vector_norm(w, dim=-1, keepdim=True)
    s = F.pad(x, (L // 2, (L - 1) // 2), mode="replicate").unfold(-1, L, P) * w
    s = s + (torch.randn_like(s) if noise is None else noise[0]) * 1e-12 * inside
    s = s - w * (s.sum(-1, keepdim=True) / w.sum(-1, keepdim=True))
    p = torch.fft.rfft(s).abs() ** 2
    axis = ramp[:K] * rate

    def linear(table, z):
        base = z.long().clamp(min=0)
        step = torch.diff(table, dim=-1, append=table[..., -1:])
        return table.gather(-1, base) + step.gather(-1, base) * (z - base)

    p = p + linear(p, (f - axis) / rate) * (axis < f)
    width = f * (2 / 3)
    bnd = (width / rate).long() + 1
    widest = int(bnd.max())   # the host read
    keep = torch.cat([(widest - bnd) <= ramp[:widest], torch.ones(*bnd.shape[:-1], K + widest, device=x.device, dtype=torch.bool)], -1)
    seg = torch.cumsum(F.pad(p, (widest, widest), mode="reflect") * keep * rate, -1)
    origin = (widest - 0.5) * rate
    p = (linear(seg, (axis + width / 2 + origin) / rate) - linear(seg, (axis - width / 2 + origin) / rate)) / width
    tiny = torch.finfo(x.dtype).eps if noise_eps is None else noise_eps
    p = p + (torch.randn_like(p) if noise is None else noise[1]).abs() * tiny
    z = f * (ramp[:K] / sr)
    lifter = torch.sinc(z) * ((1 - 2 * q1) + 2 * q1 * torch.cos(2 * torch.pi * z))
    return torch.exp(torch.fft.hfft(torch.fft.irfft(torch.log(p))[..., :K] * lifter)[..., :K])


def window(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def device(call, reps, inner, window_ms):
    """(ms per call, calls per window): the median of `reps` windows of n calls, n >= inner sized so that a window lasts window_ms"""
    call()
    n = max(inner, min(20000, math.ceil(window_ms / max(window(call, 3), 1e-4))))
    return statistics.median(window(call, n) for _ in range(reps)), n


def peak(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    call()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--inner", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=30.0)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--txt", default=None)
    a = p.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sr, P, L, B = 48000, 240, 2048, a.batch
    K = L // 2 + 1
    T = int(a.seconds * sr)
    N = (T - 1) // P + 1
    g = torch.Generator().manual_seed(0)
    t = torch.arange(T, dtype=torch.float64) / sr
    f = 100 + 200 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x64 = 0.4 * torch.sin(2 * torch.pi * f * t) + 0.2 * torch.sin(4 * torch.pi * f * t + 1) + 0.05 * torch.randn(B, T, generator=g, dtype=torch.float64)
    f064 = f.expand(B, N) * (torch.arange(N) % 30 < 20)
    say(f"# {torch.cuda.get_device_name()}; {B} x {N} frames of {P} samples at {sr} Hz, fft_length {L}; {ops.pitch_spec_lds_bytes(L)} bytes of LDS per "
        f"workgroup of 256 threads; device time: median of {a.reps} windows of at least {a.inner} calls and {a.window_ms:g} ms, after a 0.3 s clock ramp")
    ramp = torch.randn(1 << 24, device="cuda")   # clock ramp: the first ~20 ms after idle run 10 % slower (bench.py)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        ramp.mul_(1.0)
    torch.cuda.synchronize()
    for dtype, code in ((torch.float32, _lib.F32), (torch.float64, _lib.F64)):
        x, f0 = x64.to("cuda", dtype), f064.to("cuda", dtype)
        m = dsp.PitchAdaptiveSpectralAnalysis(P, sr, L, device="cuda", dtype=dtype)
        gy = torch.ones(B, N, K, device="cuda", dtype=dtype)
        xg = x.clone().requires_grad_(True)

        def ours(grad):
            if grad:
                xg.grad = None
                m(xg, f0).backward(gy)
            else:
                m(x, f0)

        def theirs(grad):
            if grad:
                xg.grad = None
                stock(xg, f0, P, sr, L).backward(gy)
            else:
                with torch.no_grad():
                    stock(x, f0, P, sr, L)

        tag = str(dtype).split(".")[-1]
        for label, call in (("kernels", ours), ("stock torch operators", theirs)):
            (fwd, nf), (both, nb) = device(lambda: call(False), a.reps, a.inner, a.window_ms), device(lambda: call(True), a.reps, a.inner, a.window_ms)
            say(f"{tag} {label:22s}: forward {fwd:9.3f} ms ({nf} calls per window)   forward + backward {both:9.3f} ms ({nb})   peak of forward + "
                f"backward {peak(lambda: call(True)):7.0f} MiB")

        # the entries on their own, the noise made once
        q, st = ops._p, ops._stream()
        n1, n2 = torch.randn(B, N, L, device="cuda", dtype=dtype), torch.randn(B, N, K, device="cuda", dtype=dtype)
        tw = device_twiddle(L, x.device, torch.float64)
        y = torch.empty(B, N, K, device="cuda", dtype=dtype)
        gframes = torch.empty(B, N, L, device="cuda", dtype=torch.float64)
        gx = torch.empty_like(x)
        common = (q(x), q(f0), q(n1), q(n2), q(tw), B, N, T, P, sr, L, 500.0, -0.15, 0.0, 0.0, 3, code)
        for label, call in (("dsa_pitch_spec", lambda: ops._call("dsa_pitch_spec", *common, q(y), st)),
                            ("dsa_pitch_spec_vjp_frames", lambda: ops._call("dsa_pitch_spec_vjp_frames", q(gy), *common, q(gframes), st)),
                            ("dsa_pitch_spec_vjp_gather", lambda: ops._call("dsa_pitch_spec_vjp_gather", q(gframes), B, N, T, P, L, code, q(gx), st)),
                            ("two randn draws", lambda: (torch.randn(B, N, L, device="cuda", dtype=dtype), torch.randn(B, N, K, device="cuda", dtype=dtype)))):
            ms, n = device(call, a.reps, a.inner, a.window_ms)
            say(f"  {label:28s} {ms:9.4f} ms ({n} calls per window; {1e3 * ms / (B * N):.3f} us per frame)")
        if dtype == torch.float64:   # the same noise through both: how far the stock operators' float64 result is from the kernel's
            with torch.no_grad():
                ref = stock(x[:1], f0[:1], P, sr, L, noise=(n1[:1], n2[:1]))
            err = ((y[:1] - ref).abs().max() / ref.abs().max().clamp(min=1.0)).item()
            say(f"  float64, first utterance, same noise: kernel against the stock operators {err:.3g} of max(1, max |value|)")
    if a.txt:
        os.makedirs(os.path.dirname(os.path.abspath(a.txt)), exist_ok=True)
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
