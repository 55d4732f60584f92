#!/usr/bin/env python3
"""Timing of WorldSynthesis (csrc/world_synth.hip): --batch utterances of one second at 16 kHz, frame period 80, fft_length 1024, float32,
two thirds of the frames voiced (runs of 20 voiced and 10 unvoiced frames, F0 between 100 and 300 Hz).
  * the module's forward and forward + backward, wall clock around a call and a synchronisation (the forward reads the pulse counts
    back, so the host is part of it): the median of --reps calls after --warmup;
  * each entry on its own, device time by HIP events around --inner enqueued calls: the two launches of the pulse list (without the
    host read between them), the responses, the overlap-add, and the two launches of the backward;
  * beside them the reference's forward restated here from stock torch operators on the device (torch.fft for the transforms, nonzero,
    gathers and scatter_add_), gradient by autograd; and the peak memory of both.

    python tools/time_world_synth.py [--reps 10] [--warmup 2] [--inner 5] [--batch 256] [--txt profiles/world_synth_time_v1.txt]
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

TAU = math.tau


def interp(x, y, xq):
    m = torch.diff(y) / torch.diff(x)
    b = y[..., :-1] - m * x[..., :-1]
    idx = torch.searchsorted(x, xq, right=False)
    m = F.pad(m, (1, 1))
    b = torch.cat([y[..., :1], b, y[..., -1:]], dim=-1)
    return m.gather(-1, idx) * xq + b.gather(-1, idx)


def minimum_phase(s):
    D = s.shape[-1]
    c = torch.fft.irfft(0.5 * torch.log(s))
    c = torch.cat((c[..., :1], 2 * c[..., 1:D - 1], c[..., D - 1:D]), dim=-1)
    return torch.exp(torch.fft.rfft(c, n=2 * (D - 1)))


def stock(f0, ap, sp, noise_of, P, sr, L, default_f0, ramp, remover):
    """world_synth.py:166-321 from stock torch operators (batched input, no out_length)"""
    B, N, D = sp.shape
    T, H = N * P, L // 2
    ap, sp = torch.clip(ap, 1e-6, 1 - 1e-6), torch.clip(sp, min=1e-6)
    cf0 = torch.where(f0 < sr / L + 1, 0, f0).detach()
    vuv = (0 < cf0).type(cf0.dtype)
    t = (torch.arange(T, device=f0.device, dtype=f0.dtype) / sr).repeat(B, 1)
    ct = (torch.arange(N, device=f0.device, dtype=f0.dtype) * (P / sr)).repeat(B, 1)
    iv = 0.5 < interp(ct, vuv, t)
    if0 = torch.where(iv, interp(ct, cf0, t), default_f0)
    wrap = torch.fmod(torch.cumsum(TAU / sr * if0.double(), dim=-1).type(f0.dtype), TAU)
    where = torch.nonzero(torch.pi < torch.abs(torch.diff(wrap)), as_tuple=True)
    bi, ti = where
    v = iv[where].unsqueeze(-1)
    y1 = wrap[where] - TAU
    shift = -y1 / (wrap[bi, ti + 1] - y1) / sr
    frame = t[where] * (sr / P)
    fl, ce = frame.floor().long().clip(max=N - 1), frame.ceil().long().clip(max=N - 1)
    up = (frame - fl).unsqueeze(-1)
    se = (1 - up) * sp[bi, fl] + up * sp[bi, ce]
    ar = ((1 - up) * ap[bi, fl] + up * ap[bi, ce]) ** 2

    def response(spec):
        r = torch.fft.hfft(spec)
        return torch.fft.fftshift(torch.cat([r[..., :1], r[..., 1:].flip(-1)], dim=-1), dim=-1)

    per = response(minimum_phase((1 - ar) * se) * torch.exp(-1j * ramp[:D] * (TAU * sr / L * shift).unsqueeze(-1)))
    dd = -per[..., H:].sum(-1, keepdim=True) * remover
    per = torch.cat((dd[..., :H], per[..., H:] + dd[..., H:]), dim=-1) * (0.5 < v)
    ns = torch.diff(ti, append=ti[-1:]).clip(min=0).unsqueeze(-1)
    mask = ramp < ns
    nz = noise_of(per) * mask
    nz = (nz - torch.nan_to_num(nz.sum(-1, keepdim=True) / ns)) * mask
    apr = response(minimum_phase(torch.where(0 < v, ar, 1) * se) * torch.fft.rfft(nz))
    resp = (per * torch.sqrt(ns) + apr) / L
    T_ = T + (L + P - 1) // P * P
    y = torch.zeros((B, T_), device=sp.device, dtype=sp.dtype)
    y.view(-1).scatter_add_(-1, ((bi * T_ + ti).unsqueeze(-1) + ramp).view(-1), resp.view(-1))
    return torch.narrow(y, -1, H, T)


def wall(call, reps, warmup):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def device(call, reps, warmup, inner):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times)


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
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--inner", type=int, default=5)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--txt", default=None)
    a = p.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    P, sr, L, N, B = 80, 16000, 1024, 200, a.batch
    D = L // 2 + 1
    g = torch.Generator().manual_seed(0)
    voiced = (torch.arange(N) % 30 < 20).float()
    f0 = ((100 + 200 * torch.rand(B, N, generator=g)) * voiced).cuda()
    ap = (0.05 + 0.9 * torch.rand(B, N, D, generator=g)).cuda()
    sp = (torch.rand(B, N, D, generator=g) * torch.exp(-4 * torch.arange(D) / D) + 1e-3).cuda()
    m = dsp.WorldSynthesis(P, sr, L, device="cuda")
    offsets, irec, frec, pulses = ops.world_pulses(f0, P, sr, L, m.default_f0)
    say(f"# {torch.cuda.get_device_name()}; float32; {B} x {N} frames of {P} samples at {sr} Hz, fft_length {L}, {voiced.mean():.2f} voiced; {pulses} pulses; "
        f"wall: median of {a.reps} calls after {a.warmup}; device: median of {a.reps} windows of {a.inner} calls")

    def ours(grad):
        x, z = ap.clone().requires_grad_(grad), sp.clone().requires_grad_(grad)
        y = m(f0, x, z)
        if grad:
            y.backward(torch.ones_like(y))

    def theirs(grad):
        x, z = ap.clone().requires_grad_(grad), sp.clone().requires_grad_(grad)
        y = stock(f0, x, z, torch.randn_like, P, sr, L, m.default_f0, m.ramp, m.dc_remover)
        if grad:
            y.backward(torch.ones_like(y))

    for label, grad in (("forward", False), ("forward + backward", True)):
        say(f"{label:18s} WorldSynthesis {wall(lambda: ours(grad), a.reps, a.warmup):9.3f} ms, peak {peak(lambda: ours(grad)):8.0f} MiB   "
            f"stock torch {wall(lambda: theirs(grad), a.reps, a.warmup):9.3f} ms, peak {peak(lambda: theirs(grad)):8.0f} MiB")

    # the entries on their own
    q, code, st = ops._p, _lib.F32, ops._stream()
    counts = torch.zeros(B, dtype=torch.int64, device="cuda")
    noise, tw = m._randn(pulses, L), device_twiddle(L, f0.device, f0.dtype)
    resp, y, gy = torch.empty(pulses, L, device="cuda"), torch.empty(B, N * P, device="cuda"), torch.ones(B, N * P, device="cuda")
    grows, gap, gsp = torch.empty(pulses, 2, D, device="cuda"), torch.empty_like(ap), torch.empty_like(sp)
    entries = [
        ("pulses (count)", lambda: ops._call("dsa_world_synth_pulses", q(f0), B, N, P, sr, L, float(m.default_f0), None, code, q(counts), None, None, st)),
        ("pulses (records)", lambda: ops._call("dsa_world_synth_pulses", q(f0), B, N, P, sr, L, float(m.default_f0), q(offsets), code, q(counts), q(irec),
                                               q(frec), st)),
        ("responses", lambda: ops._call("dsa_world_synth_responses", q(ap), q(sp), q(noise), q(irec), q(frec), q(offsets), q(m.dc_remover), q(tw), B, N, sr,
                                        L, pulses, code, q(resp), st)),
        ("overlap_add", lambda: ops._call("dsa_world_synth_overlap_add", q(resp), q(irec), q(offsets), B, N * P, L, pulses, code, q(y), st)),
        ("vjp_pulses", lambda: ops._call("dsa_world_synth_vjp_pulses", q(gy), q(ap), q(sp), q(noise), q(irec), q(frec), q(offsets), q(m.dc_remover), q(tw), B,
                                         N, N * P, sr, L, pulses, code, q(grows), st)),
        ("vjp_frames", lambda: ops._call("dsa_world_synth_vjp_frames", q(grows), q(ap), q(sp), q(irec), q(frec), q(offsets), B, N, L, pulses, code, q(gap),
                                         q(gsp), st)),
        ("torch.randn (the noise)", lambda: m._randn(pulses, L)),
    ]
    for label, call in entries:
        say(f"{label:24s} {device(call, a.reps, a.warmup, a.inner):9.3f} ms")
    if a.txt:
        os.makedirs(os.path.dirname(os.path.abspath(a.txt)), exist_ok=True)
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
