#!/usr/bin/env python3
"""Timing of Aperiodicity (csrc/ap.hip): --batch utterances of --seconds at 48 kHz, frame period 240, fft_length 2048, float32 and
float64; a harmonic signal with noise, F0 between 100 and 300 Hz with unvoiced runs.
  * the module's forward and forward + backward: device time by HIP events around a window of enqueued calls, the median of --reps
    windows (the operator has no host read, so the device time is the operator's time).  As in tools/bench_fwdbwd.py the clocks are
    spun up for 0.3 s first (the first 20 ms after idle run 10 % slower), and a window holds at least --inner calls and at least
    --window-ms of work: the calls per window are sized from a first timed call, so a 6 us launch is timed over thousands of calls, not
    three.  The input is made once outside the windows; nothing but the operator is inside them;
  * each entry on its own, the same way: the levels of the QMF pyramid, the fits with the epilogue, the fits' adjoint with the overlap-add
    (one entry, two launches), the levels of the pyramid's transpose; and the share of the pyramid in the sum of the entries.  Back to
    back in one stream, so a small entry's figure is its launch-to-launch time, the launch overhead included;
  * the peak memory of a forward + backward.

    python tools/bench_ap.py [--reps 10] [--inner 30] [--window-ms 30] [--batch 8] [--seconds 10] [--txt profiles/ap_time_v2.txt]
"""
import argparse
import os
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib, ops  # noqa: E402


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
    p.add_argument("--inner", type=int, default=30)
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
    T = int(a.seconds * sr)
    N = T // P
    g = torch.Generator().manual_seed(0)
    t = torch.arange(T, dtype=torch.float64) / sr
    f = 100 + 200 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    x64 = 0.4 * torch.sin(2 * torch.pi * f * t) + 0.2 * torch.sin(4 * torch.pi * f * t + 1) + 0.05 * torch.randn(B, T, generator=g, dtype=torch.float64)
    f064 = f.expand(B, N) * (torch.arange(N) % 30 < 20)
    n_band, _, seg = ops.ap_bands(sr)
    lens = ops.ap_band_lengths(T, n_band)
    say(f"# {torch.cuda.get_device_name()}; {B} x {N} frames of {P} samples at {sr} Hz, fft_length {L}; {n_band} bands, segments {seg}; "
        f"device time: median of {a.reps} windows of at least {a.inner} calls and {a.window_ms:g} ms, after a 0.3 s clock ramp")
    ramp = torch.randn(1 << 24, device="cuda")   # clock ramp: the first ~20 ms after idle run 10 % slower (bench.py)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        ramp.mul_(1.0)
    torch.cuda.synchronize()
    for dtype, code in ((torch.float32, _lib.F32), (torch.float64, _lib.F64)):
        x, f0 = x64.to("cuda", dtype), f064.to("cuda", dtype)
        m = dsp.Aperiodicity(P, sr, L, device="cuda", dtype=dtype)
        e = m.extractor
        gy = torch.ones(B, N, L // 2 + 1, device="cuda", dtype=dtype)

        xg = x.clone().requires_grad_(True)

        def ours(grad):
            if grad:
                xg.grad = None
                m(xg, f0).backward(gy)
            else:
                m(x, f0)

        tag = str(dtype).split(".")[-1]
        (fwd, nf), (both, nb) = device(lambda: ours(False), a.reps, a.inner, a.window_ms), device(lambda: ours(True), a.reps, a.inner, a.window_ms)
        say(f"{tag}: forward {fwd:9.3f} ms ({nf} calls per window)   forward + backward {both:9.3f} ms ({nb})   peak of forward + backward "
            f"{peak(lambda: ours(True)):7.0f} MiB")

        # the entries on their own
        q, st, ld = ops._p, ops._stream(), sum(lens)
        bands, gbands = (torch.empty(B, ld, device="cuda", dtype=torch.float64) for _ in range(2))   # float64 whatever the dtype
        levels = [x] + [torch.empty(B, n, device="cuda", dtype=torch.float64) for n in lens[:-1]]
        glevels = [torch.empty_like(v) for v in levels]
        y = torch.empty(B, N, L // 2 + 1, device="cuda", dtype=dtype)
        gruns = torch.empty(B, N, 3 * (sum(seg) + 2 * n_band), device="cuda", dtype=dtype)
        starts = torch.empty(B, N, n_band, _lib.AP_START_WORDS, device="cuda", dtype=torch.int64)
        offs = [sum(lens[:i]) for i in range(n_band)]
        common = (q(bands), ld, q(f0), q(e.window), q(e.window_sqrt), e.window.stride(0), q(e.interp_indices), q(e.interp_weights), B, N, T, P, sr, 30.0,
                  L // 2 + 1, 1e-5, 0.001, 0.999, 0, code)
        entries, pyramid = [], 0.0
        for i in range(n_band - 1):
            Tl, last = levels[i].shape[1], i == n_band - 2
            low = bands[:, offs[-1]:] if last else levels[i + 1]
            entries.append((f"qmf level {i} ({Tl} samples)", True, lambda i=i, Tl=Tl, low=low, last=last: ops._call(
                "dsa_ap_qmf", q(levels[i]), B, Tl, Tl, code if i == 0 else _lib.F64, q(bands[:, offs[i]:]), ld, q(low), ld if last else lens[i], st)))
        entries.append(("tandem (fits + epilogue)", False, lambda: ops._call("dsa_ap_tandem", *common, q(y), st)))
        entries.append(("tandem_vjp (adjoint + overlap-add)", False, lambda: ops._call("dsa_ap_tandem_vjp", q(gy), *common, q(gruns), q(starts), q(gbands), ld,
                                                                                      st)))
        for i in range(n_band - 2, -1, -1):
            Tl, last = levels[i].shape[1], i == n_band - 2
            glow = gbands[:, offs[-1]:] if last else glevels[i + 1]
            entries.append((f"qmf_vjp level {i}", True, lambda i=i, Tl=Tl, glow=glow, last=last: ops._call(
                "dsa_ap_qmf_vjp", q(gbands[:, offs[i]:]), ld, q(glow), ld if last else lens[i], B, Tl, code if i == 0 else _lib.F64, q(glevels[i]), Tl, st)))
        total = 0.0
        for label, is_pyramid, call in entries:
            ms, n = device(call, a.reps, a.inner, a.window_ms)
            total += ms
            pyramid += ms if is_pyramid else 0.0
            say(f"  {label:36s} {ms:9.4f} ms ({n} calls per window)")
        say(f"  sum of the entries {total:9.3f} ms, of which the pyramid and its transpose {pyramid:9.3f} ms ({100 * pyramid / total:.1f} %)")
    if a.txt:
        os.makedirs(os.path.dirname(os.path.abspath(a.txt)), exist_ok=True)
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
