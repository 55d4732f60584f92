#!/usr/bin/env python3
"""Golden fixtures of WorldSynthesis, by importing the REFERENCE.  Build container only (CPU; under a minute).

    python tests/golden/make_golden_world_synth.py   # writes tests/golden/world_synth.npz, world_synth_big.npz, world_synth_api.json

The cases and the formulas of their inputs, noise and cotangents are tests/world_synth_cases.py (all exact in float32; the files hold
results only, split in two so that each stays below 1 MiB).  Per case <name>, from the reference in float64: <name>_y, <name>_gsp,
<name>_gap (the gradients for the case's cotangent), <name>_index (pulses, 2: utterance and sample index), <name>_shift (the fractional
time shifts in seconds) and <name>_f0.  The reference's float32 results are kept where a test compares with them (mixed_even, whose
float32 pulse list differs: <name>_y32 and so on); elsewhere only their distance from the float64 results goes to the JSON (E_ref, E_gsp,
E_gap).  The float32 pulse list and shifts, <name>_index32 and <name>_shift32, are kept for every case.  The noise reaches the reference
through a replaced torch.randn_like for the duration of a call; the pulse list, the wrapped phase and the interpolated voicing are read
off replaced torch.nonzero / torch.fmod / interp1 the same way.

Asserted here and again in tests/test_world_synth_cpu.py from the stored numbers: every case but mixed_even has one pulse list in both
precisions, every pulse keeps min(-y1, y2) >= 1e-3 rad at its wrap, every interpolated voicing value stays 1e-3 from 1/2, no F0 lies
within 1e-3 Hz of sample_rate / fft_length + 1, and the reference's batch-wide noise_size equals the per-utterance one (0 for the last
pulse of every utterance).  D_ulp: the largest change of the float64 results, relative to max(1, max |ref|), when every value of f0, ap,
sp and the noise moves one unit in its last place at random (three draws) with the pulse list unchanged.  The JSON further holds the
signatures, buffers, state_dict keys, the exception type and text of every invalid call of world_synth_cases.ERRORS, and what the
reference does when no pulse falls anywhere (N = 1, P = 5)."""
import inspect
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402

import world_synth_cases as W  # noqa: E402


class Tap:
    """Replaces torch.randn_like, torch.nonzero, torch.fmod and the module's interp1 while a reference call runs."""

    def __init__(self, ws_module, name, noise_of=None):
        self.m, self.name, self.noise_of = ws_module, name, noise_of
        self.seen = {}

    def __enter__(self):
        self.saved = (torch.randn_like, torch.nonzero, torch.fmod, self.m.interp1)
        randn_like, nonzero, fmod, interp1 = self.saved
        calls = []

        def my_randn_like(t, **kw):
            n = W.noise(self.name, t.shape[0], t.shape[1]) if self.noise_of is None else self.noise_of(t.shape)
            self.seen["noise"] = n
            return torch.as_tensor(n).to(t.dtype)

        def my_nonzero(*a, **kw):
            out = nonzero(*a, **kw)
            self.seen["index"] = torch.stack(out, dim=1).numpy().copy()
            return out

        def my_fmod(*a, **kw):
            out = fmod(*a, **kw)
            self.seen["wrap"] = out.detach().clone()
            return out

        def my_interp1(*a, **kw):
            out = interp1(*a, **kw)
            calls.append(out.detach().clone())
            self.seen["vuv"] = calls[-1]   # the second call interpolates the voicing flag
            return out

        torch.randn_like, torch.nonzero, torch.fmod, self.m.interp1 = my_randn_like, my_nonzero, my_fmod, my_interp1
        return self

    def __exit__(self, *exc):
        torch.randn_like, torch.nonzero, torch.fmod, self.m.interp1 = self.saved


def run(diffsptk, ws_module, name, dtype, arrays=None, noise_of=None):
    """The reference on a case in `dtype`: dict of float64 arrays y, gsp, gap, index, shift, margins"""
    c = W.CASES[name]
    f0, ap, sp = (np.asarray(a, dtype=np.float64) for a in (arrays or W.inputs(name)))
    args, kw = W.options(name)
    m = diffsptk.WorldSynthesis(*args, **kw, dtype=dtype)
    t = [torch.tensor(a, dtype=dtype) for a in W.shaped(name, f0, ap, sp)]
    t[1].requires_grad_(True)
    t[2].requires_grad_(True)
    with Tap(ws_module, name, noise_of) as tap:
        y = m(*t, **({"out_length": c["out_length"]} if "out_length" in c else {}))
    y.backward(torch.tensor(W.cotangent(name, tuple(y.shape)), dtype=dtype))
    index, wrap, vuv = tap.seen["index"], tap.seen["wrap"], tap.seen["vuv"]
    b, i = torch.as_tensor(index[:, 0]), torch.as_tensor(index[:, 1])
    y1 = wrap[b, i] - math.tau
    y2 = wrap[b, i + 1]
    shift = -y1 / (y2 - y1) / c["sr"]
    # noise_size as the reference has it (diff over the flattened batch) and per utterance
    flat = torch.diff(i, append=i[-1:]).clip(min=0).numpy()
    own = np.zeros_like(flat)
    for k in range(len(flat) - 1):
        own[k] = index[k + 1, 1] - index[k, 1] if index[k + 1, 0] == index[k, 0] else 0
    return dict(y=y.detach().double().numpy(), gsp=t[2].grad.double().numpy(), gap=t[1].grad.double().numpy(), index=index,
                shift=shift.double().numpy(), wrap_margin=float(torch.minimum(-y1, y2).min()), vuv_margin=float((vuv - 0.5).abs().min()),
                noise_same=bool(np.array_equal(flat, own)), noise_size=own, noise=tap.seen["noise"])


def rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def ulp_moved(a, rng):
    a = np.asarray(a, dtype=np.float64)
    return np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def raised(f, m):
    try:
        f(m)
        return ["ok", ""]
    except Exception as e:   # noqa: BLE001
        return [type(e).__name__, str(e)]


def main():
    diffsptk = import_reference()
    import diffsptk.modules.world_synth as ws_module

    files = {stem: {} for stem in W.FILES}
    where = {name: stem for stem, names in W.FILES.items() for name in names}
    listed = []
    for name, c in W.CASES.items():
        out = files[where[name]]
        f_min = c["sr"] / c["L"] + 1
        f0 = W.inputs(name)[0]
        assert np.abs(f0.astype(np.float64) - f_min).min() >= 1e-3, name
        r64 = run(diffsptk, ws_module, name, torch.float64)
        r32 = run(diffsptk, ws_module, name, torch.float32)
        assert all(np.isfinite(r[k]).all() for r in (r64, r32) for k in ("y", "gsp", "gap")), name
        assert r64["noise_same"] and r32["noise_same"], name
        same = np.array_equal(r64["index"], r32["index"])
        rec = dict(name=name, pulses=int(len(r64["index"])), same_pulses=bool(same), wrap_margin=min(r64["wrap_margin"], r32["wrap_margin"]),
                   vuv_margin=min(r64["vuv_margin"], r32["vuv_margin"]), max_noise_size=int(r64["noise_size"].max()),
                   max_y=float(np.abs(r64["y"]).max()), max_gsp=float(np.abs(r64["gsp"]).max()), max_gap=float(np.abs(r64["gap"]).max()))
        if name != "mixed_even":
            assert same, name
            assert rec["wrap_margin"] >= 1e-3 and rec["vuv_margin"] >= 1e-3, rec
            rec.update(E_ref=float(np.abs(r32["y"] - r64["y"]).max()), E_gsp=float(np.abs(r32["gsp"] - r64["gsp"]).max()),
                       E_gap=float(np.abs(r32["gap"] - r64["gap"]).max()))
            # one unit in the last place of every input, three draws
            d = dict(y=0.0, gsp=0.0, gap=0.0)
            rng = np.random.default_rng(W.seed_of(name))
            for _ in range(3):
                moved = [ulp_moved(a, rng) for a in W.inputs(name)]
                rp = run(diffsptk, ws_module, name, torch.float64, arrays=moved,
                         noise_of=lambda shape: ulp_moved(W.noise(name, shape[0], shape[1]), rng))
                assert np.array_equal(rp["index"], r64["index"]), name
                for k in d:
                    d[k] = max(d[k], rel(rp[k], r64[k]))
            rec.update(D_ulp_y=d["y"], D_ulp_gsp=d["gsp"], D_ulp_gap=d["gap"])
        else:
            for k in ("y", "gsp", "gap"):
                out[f"{name}_{k}32"] = r32[k].astype(np.float32)
        out[f"{name}_index32"], out[f"{name}_shift32"] = r32["index"], r32["shift"].astype(np.float32)
        for k in ("y", "gsp", "gap", "index", "shift"):
            out[f"{name}_{k}"] = r64[k]
        out[f"{name}_f0"] = f0
        rec["noise_sum"] = float(np.abs(r64["noise"].astype(np.float64)).sum())   # a check that the tests inject the same numbers
        listed.append(rec)
        print(rec, flush=True)
    sizes = [c["name"] for c in listed if c["max_noise_size"] > W.CASES[c["name"]]["L"]]
    assert "sparse" in sizes, sizes

    cls = diffsptk.WorldSynthesis
    m32, m64 = cls(80, 16000, 1024), cls(80, 16000, 1024, dtype=torch.float64)
    files["world_synth"]["dc_remover64"] = m64.dc_remover.numpy()
    files["world_synth"]["dc_remover32"] = m32.dc_remover.numpy()
    for stem, arrays in files.items():
        np.savez_compressed(os.path.join(HERE, stem + ".npz"), **arrays)
        assert os.path.getsize(os.path.join(HERE, stem + ".npz")) < 1 << 20, stem

    api = {
        "signatures": {name: signature(getattr(cls, name)) for name in ("__init__", "forward")},
        "in_root": hasattr(diffsptk, "WorldSynthesis"),
        "has_functional": hasattr(diffsptk.functional, "world_synth"),
        "buffers": {key: {k: [str(v.dtype), list(v.shape)] for k, v in m.named_buffers()} for key, m in (("float32", m32), ("float64", m64))},
        "state_dict": sorted(m32.state_dict()),
        "errors": {name: raised(f, diffsptk) for name, f in W.ERRORS.items()},
        "no_pulse": raised(lambda d: d.WorldSynthesis(5, 16000, 1024)(torch.zeros(1, 1), torch.full((1, 1, 513), 0.5), torch.ones(1, 1, 513)),
                           diffsptk)[0],
        "cases": listed,
    }
    assert all(r[0] == "ValueError" for r in api["errors"].values()), api["errors"]
    with open(os.path.join(HERE, "world_synth_api.json"), "w") as f:
        json.dump(api, f, indent=1)
        f.write("\n")
    print("wrote", len(listed), "cases;", {s: os.path.getsize(os.path.join(HERE, s + ".npz")) for s in files}, "no pulse:", api["no_pulse"])


if __name__ == "__main__":
    main()
