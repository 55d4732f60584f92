#!/usr/bin/env python3
"""Timing of excite (csrc/excite.hip) at 1024 utterances of 200 frames, frame period 80, float32: "pulse" and "sinusoidal" with
unvoiced_region "zeros" and "gauss".  Device time by HIP events around --inner calls, median of --reps windows after --warmup, the
alternatives alternated window by window in one process:
  * hip    the library's entry through the public functional (one launch; "gauss": plus torch's generator and one select);
  * chain  the same operation as the reference computes it (excite.py:222-310), written with stock torch operators on the GPU: the
           masks, the in-place extension, F.interpolate, the reciprocal through a boolean gather, cumsum in float64, cummax, the
           shape through boolean gathers and scatters.  Every boolean gather reads a count back to the host, so the chain's time is
           a host clock around a synchronise; it works on a copy of the pitch, which it overwrites.
The entry is also timed alone on buffers allocated once, beside the 4 bytes per sample that it must write and the time those take at
the HBM peak, and once on a single utterance of 16 000 frames, which one workgroup walks.  Pitch tracks: voiced runs of 5 .. 40 frames
with periods of 40 .. 320 samples drifting by 2 % per frame, unvoiced runs of 3 .. 20 frames between them.

    python tools/time_excite.py [--reps 15] [--warmup 3] [--inner 10] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as NF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd.functional as F  # noqa: E402
from diffsptk_amd import _lib, ops as O  # noqa: E402
from time_parcor import HBM_PEAK, alternate  # noqa: E402

B, N, P = 1024, 200, 80
LONG = 16000   # frames of the single long utterance


def tracks(B=B, N=N, seed=0):
    rng = np.random.default_rng(seed)
    p = np.zeros((B, N), dtype=np.float32)
    for u in range(B):
        n, voiced = 0, bool(rng.integers(2))
        while n < N:
            L = int(rng.integers(5, 41) if voiced else rng.integers(3, 21))
            if voiced:
                run = rng.uniform(40.0, 320.0) * np.exp(np.cumsum(rng.normal(0, 0.02, L)))
                p[u, n:n + L] = np.clip(run, 20.0, 400.0)[:N - n]
            n += L
            voiced = not voiced
    return p


def chain_excite(pitch, voiced_region, unvoiced_region):
    """The reference's sequence of operators for a (B, N) float32 input, polarity "auto", init_phase "zeros"."""
    p = pitch.clone()
    unit = torch.clip(p, min=0, max=1)
    mask = torch.repeat_interleave(unit != 0, P, dim=-1)
    fell = torch.diff(NF.pad(unit, (1, 0))) == -1
    p[fell] = torch.roll(p, 1, dims=-1)[fell]
    x = NF.pad(p.unsqueeze(0), (0, 1), mode="replicate")
    p = NF.interpolate(x, size=N * P + 1, mode="linear", align_corners=True)[0, :, :-1]
    p = p * mask
    pos = p > 0
    q = torch.zeros_like(p)
    q[pos] = torch.reciprocal(p[pos])
    s = torch.cumsum(q.double(), dim=-1)
    bias, _ = torch.cummax(s * ~mask, dim=-1)
    phase = (s - bias).to(p.dtype)
    if voiced_region == "pulse":
        up = torch.diff(torch.ceil(NF.pad(phase, (1, 0)))) >= 1
        e = torch.zeros_like(p)
        e[up] = torch.sqrt(p[up])
    else:
        e = torch.zeros_like(p)
        e[mask] = torch.sin(math.tau * phase[mask])
    if unvoiced_region == "gauss":
        e[~mask] = torch.randn_like(e[~mask])
    return e


def host_ms(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    p = torch.from_numpy(tracks()).to(dev)
    voiced_share = float((p != 0).float().mean())
    out_bytes = B * N * P * 4
    floor_ms = out_bytes / HBM_PEAK * 1e3
    rows, diffs = [], {}
    for vr in ("pulse", "sinusoidal"):
        for ur in ("zeros", "gauss"):
            hip = lambda vr=vr, ur=ur: F.excite(p, P, voiced_region=vr, unvoiced_region=ur)   # noqa: E731
            chain = lambda vr=vr, ur=ur: chain_excite(p, vr, ur)   # noqa: E731
            if ur == "zeros":
                a, b = hip(), chain()
                diffs[vr] = (float((a - b).abs().max()), int(((a != 0) != (b != 0)).sum()))
            hip_ms = alternate([hip], args.reps, args.warmup, args.inner)[0]
            for _ in range(args.warmup):
                chain()
            chain_ms = sorted(host_ms(chain, max(1, args.inner // 5)) for _ in range(max(3, args.reps // 3)))
            rows.append({"voiced": vr, "unvoiced": ur, "hip_ms": hip_ms, "hip_host_ms": sorted(host_ms(hip, args.inner) for _ in range(5))[2],
                         "chain_ms": chain_ms[len(chain_ms) // 2], "bytes_written": out_bytes, "hbm_peak_ms": floor_ms,
                         "share_of_hbm_peak": floor_ms / hip_ms})
    L, st = _lib.load(), O._stream()
    out = torch.empty(B, N * P, device=dev)
    entries = {f"dsa_excite {vr}": (lambda code=code, bip=bip: L.dsa_excite(p.data_ptr(), B, N, P, code, bip, 0.0, None, _lib.F32, out.data_ptr(), st))
               for vr, code, bip in (("pulse", _lib.EXCITE_PULSE, 0), ("sinusoidal", _lib.EXCITE_SINUSOIDAL, 1), ("sawtooth", _lib.EXCITE_SAWTOOTH, 1),
                                     ("harmonic-pulse", _lib.EXCITE_HARMONIC_PULSE, 1))}
    for fn in entries.values():
        _lib.check(fn())
    ems = alternate(list(entries.values()), args.reps, args.warmup, 5 * args.inner)
    erows = [{"entry": name, "ms": t, "bytes_written": out_bytes, "hbm_peak_ms": floor_ms, "share_of_hbm_peak": floor_ms / t}
             for name, t in zip(entries, ems)]
    # a single long utterance: one workgroup walks it
    long_p = torch.from_numpy(tracks(1, LONG, 1)).to(dev)
    long_out = torch.empty(1, LONG * P, device=dev)
    one = lambda: L.dsa_excite(long_p.data_ptr(), 1, LONG, P, _lib.EXCITE_PULSE, 0, 0.0, None, _lib.F32, long_out.data_ptr(), st)   # noqa: E731
    _lib.check(one())
    long_ms = alternate([one], args.reps, args.warmup, 3)[0]
    lines = [f"excite  utterances={B} frames={N} frame_period={P} float32  {torch.cuda.get_device_name(0)}  voiced share {voiced_share:.2f}  "
             f"(hip: device events, median of {args.reps} windows of {args.inner} calls; chain: host clock around a synchronise, it reads counts back)",
             "hip against chain with unvoiced zeros (max |difference|, samples that are non-zero in one only): "
             + "  ".join(f"{n} {v[0]:.2e} / {v[1]}" for n, v in diffs.items()),
             f"{'voiced':11s} {'unvoiced':8s} {'hip ms':>9s} {'hip host ms':>11s} {'chain ms':>9s} {'chain/hip':>9s} {'MB written':>10s} {'ms at 8 TB/s':>13s} {'share of peak':>13s}"]
    for r in rows:
        lines.append(f"{r['voiced']:11s} {r['unvoiced']:8s} {r['hip_ms']:9.4f} {r['hip_host_ms']:11.4f} {r['chain_ms']:9.3f} {r['chain_ms'] / r['hip_host_ms']:9.1f} "
                     f"{r['bytes_written'] / 1e6:10.2f} {r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f}")
    lines.append(f"{'entry alone':26s} {'ms':>9s} {'MB written':>10s} {'ms at 8 TB/s':>13s} {'share of peak':>13s}")
    for r in erows:
        lines.append(f"{r['entry']:26s} {r['ms']:9.4f} {r['bytes_written'] / 1e6:10.2f} {r['hbm_peak_ms']:13.4f} {r['share_of_hbm_peak']:13.2f}")
    lines.append(f"one utterance of {LONG} frames (dsa_excite pulse, {LONG * P} samples on one compute unit): {long_ms:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "utterances": B, "frames": N, "frame_period": P, "dtype": "float32",
                       "hbm_peak_bytes_per_s": HBM_PEAK, "reps": args.reps, "inner": args.inner, "rows": rows, "entries": erows,
                       "one_utterance": {"frames": LONG, "ms": long_ms}}, f, indent=1)


if __name__ == "__main__":
    main()
