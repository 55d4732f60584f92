#!/usr/bin/env python3
"""Timing of Yingram (csrc/yingram.hip), float32, device time by HIP events around --inner enqueued calls (so that the host's submission
of one call hides behind the device's work on the one before), divided by --inner: the median of --reps such windows after --warmup calls.
  * the docstring shape of the reference: 22 050 Hz, Frame(2048, 441), Yingram(2048), --batch waveforms of one second (50 frames each):
    Yingram on frames by each route, fuse(Frame, Yingram) from the waveform by each route, Frame + Yingram as two launches, and the
    backward of Yingram by each route;
  * the crossing of the two routes: forward and backward by each route at --frames frames of L = 32 .. 1024 (lag_max the longest the
    grid of notes allows), which is where DSA_YINGRAM_FFT_MIN_FRAME_LENGTH comes from.

    python tools/time_yingram.py [--reps 20] [--warmup 3] [--inner 10] [--batch 256] [--frames 16384] [--txt profiles/yingram_time_v1.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp  # noqa: E402
from diffsptk_amd import _lib  # noqa: E402

ROUTES = {"direct": _lib.ALGO_GENERIC, "fft": _lib.ALGO_TUNED}


INNER = 10


def timed(call, reps, warmup):
    """median milliseconds of one call() on the device, from windows of INNER enqueued calls"""
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(INNER):
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / INNER)
    return statistics.median(times)


def yingram_for(L, **kw):
    for lag_max in (None, L - 2, L - 3, L - 4):   # the longest lag range whose largest lag stays inside
        try:
            return dsp.Yingram(L, lag_max=lag_max, device="cuda", **kw)
        except ValueError:
            continue
    raise ValueError(L)


def backward_call(m, x):
    x = x.clone().requires_grad_(True)
    y = m(x)
    gy = torch.ones_like(y)
    return lambda: torch.autograd.grad(y, x, gy, retain_graph=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--txt", default=None)
    a = ap.parse_args()
    global INNER
    INNER = a.inner
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(0)
    wave = torch.randn(a.batch, 22050, generator=g).cuda()
    frame, m = dsp.Frame(2048, 441), dsp.Yingram(2048, device="cuda")
    frames = frame(wave)
    say(f"# {torch.cuda.get_device_name()}; float32; median of {a.reps} windows of {a.inner} calls after {a.warmup}; {a.batch} x 22050 samples -> {tuple(frames.shape)} frames -> M = {len(m.lags)}")
    for route, algo in ROUTES.items():
        m.algo = algo
        fused = dsp.fuse(frame, m)
        say(f"L=2048 {route:6s} yingram(frames) {timed(lambda: m(frames), a.reps, a.warmup):8.3f} ms   fuse(frame, yingram)(x) "
            f"{timed(lambda: fused(wave), a.reps, a.warmup):8.3f} ms   yingram(frame(x)) {timed(lambda: m(frame(wave)), a.reps, a.warmup):8.3f} ms   "
            f"backward {timed(backward_call(m, frames), a.reps, a.warmup):8.3f} ms")
    say(f"L=2048 frame(x) alone {timed(lambda: frame(wave), a.reps, a.warmup):8.3f} ms")
    del frames, wave
    say(f"# the crossing: {a.frames} frames, sample_rate 16000, lag_min 8, n_bin 20; ms forward / backward")
    for L in (32, 48, 64, 96, 128, 192, 256, 384, 512, 1024):
        m = yingram_for(L, sample_rate=16000, lag_min=8)
        x = torch.randn(a.frames, L, generator=g).cuda()
        row = f"L={L:5d} lag_max={len(m.ramp) + 1:5d} M={len(m.lags):4d}"
        for route, algo in ROUTES.items():
            m.algo = algo
            row += f"   {route} {timed(lambda: m(x), a.reps, a.warmup):7.4f} / {timed(backward_call(m, x), a.reps, a.warmup):7.4f}"
        say(row)
    if a.txt:
        os.makedirs(os.path.dirname(os.path.abspath(a.txt)), exist_ok=True)
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
