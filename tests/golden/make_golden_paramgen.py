#!/usr/bin/env python3
"""Golden fixtures of delta / mlpg / mcpf, by importing the REFERENCE.  Build container only.

    python tests/golden/make_golden_paramgen.py     # writes tests/golden/paramgen.npz and paramgen_api.json (data)

Inputs are unit-variance noise (numpy default_rng(0), one stream in the order of the case lists), rounded to float32 so that both
precisions see the same values; for mcpf they are scaled like a cepstrum (c0 about 2, the rest decaying with the index).  Per case
`<tag>_x` the input and `<tag>_g` the cotangent (float32), `<tag>_64` the reference's float64 result and `<tag>_g64` its float64 gradient
of <result, cotangent>.  The float32 reference enters through E_ref = max |ref32 - ref64| and E_gref (the same for the gradient), recorded
per case.  The npz holds two flat arrays, `f64` and `f32`, and paramgen_api.json the index `arrays`: name -> [which, offset, shape].

The case lists cover what tests/test_paramgen_cpu.py spells out; no case is a full cross product, because no committed file may pass
1 MiB: D = 65 goes with the short sequences (and once with T = 50) and T = 193 / 257 with D = 3 or 1.

Conditions, asserted here: every input is exactly representable in float32; E_ref < 1e-4 everywhere; the reference's docstring
examples hold, and mlpg(delta(x)) == x there; the reference fails with a RuntimeError for T < 2N (recorded: the library raises
ValueError instead)."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

SEEDS = {"default": [[-0.5, 0, 0.5], [1, -2, 1]], "w23": [2, 3], "w1": [1], "asym": [[-0.5, 0], [0, 0, 0.5]], "even": [[1, -1]],
         "one": [[1.0]], "w2": [2], "w4": [4], "w5": [5]}
HALF = {"default": 1, "w23": 3, "w1": 1, "asym": 1, "even": 1, "one": 0, "w2": 2, "w4": 4, "w5": 5}   # N = (L - 1) / 2
MCPF = [(24, 0.42, 0.2, 2, 128), (3, 0.1, 0.2, 2, 128), (24, 0.42, 0.4, 0, 127), (30, 0.55, -0.1, 5, 16), (0, 0.3, 0.2, 0, 8),
        (4, 0, 0.3, 1, 9), (24, 0.42, 0.2, 40, 512)]
MCPF_LEADS = {1: (), 7: (7,), 130: (2, 65)}


def delta_cases():
    """(tag, seed name, static_out, lead or None for 2-D input, T, D)"""
    rows = []
    for name in ("default", "w23", "w1", "asym", "even"):
        N = HALF[name]
        Ts = sorted({1, 2, N, N + 1, 2 * N + 1})
        for i, T in enumerate(Ts):
            D = (1, 65, 3)[i % 3]
            lead = None if i % 2 else (3,)
            rows.append((name, bool((i // 2 + 1) % 2), lead, T, D))
        if name == "default":
            rows.append((name, True, (2,), 193, 3))
            rows.append((name, False, None, 193, 3))
        else:
            rows.append((name, name in ("w1", "even"), None, 193, 3))
        rows.append((name, False, (3,), 2 * N + 1, 65))
    return [(f"delta_{n}_{'s' if s else 'd'}_{'2d' if lead is None else 'x'.join(map(str, lead))}_t{T}_d{D}", n, s, lead, T, D)
            for n, s, lead, T, D in rows]


def mlpg_cases():
    """(tag, seed name, lead, T, D)"""
    rows = []
    leads = [(), (3,), (2, 2)]
    for name in ("default", "w23", "w1", "asym", "even", "one"):
        N = HALF[name]
        for i, T in enumerate(sorted({max(2 * N, 1), 2 * N + 1, 2 * N + 2})):
            rows.append((name, leads[i % 3], T, (65, 1, 3)[i % 3]))
        rows.append((name, (), 50, 65) if name == "default" else (name, (2, 2) if name == "one" else (3,), 50, 1))
        rows.append((name, (), 257, 3 if name in ("default", "w23", "one") else 1))
    for name in ("w2", "w4", "w5"):   # half-bandwidths 4 and 8 (the last register kernel) and 10 (the kernel that reads the column back)
        N = HALF[name]
        rows.append((name, (), 2 * N, 3))
        rows.append((name, (3,), 50, 3))
    return [(f"mlpg_{n}_{'x'.join(map(str, lead)) or '0'}_t{T}_d{D}", n, lead, T, D) for n, lead, T, D in rows]


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def main():
    d = import_reference()
    F = d.functional
    rng = np.random.default_rng(0)
    out = {}

    def noise(*shape):
        v = rng.standard_normal(shape).astype(np.float32)
        assert np.abs(v).max() < 6
        return v

    def run(fn, v, dt, cot):
        """(result, gradient of <result, cot>) of the reference in dtype dt, as float64 arrays"""
        t = torch.tensor(v, dtype=dt, requires_grad=True)
        r = fn(t)
        (r * torch.tensor(cot, dtype=dt)).sum().backward()
        return r.detach().double().numpy(), t.grad.double().numpy()

    def record(tag, fn32, fn64, x, g):
        y32, gx32 = run(fn32, x, torch.float32, g)
        y64, gx64 = run(fn64, x, torch.float64, g)
        assert y64.shape == g.shape and gx64.shape == x.shape
        e, eg = float(np.abs(y32 - y64).max()), float(np.abs(gx32 - gx64).max())
        assert e < 1e-4 and eg < 1e-4, (tag, e, eg)
        out[f"{tag}_x"], out[f"{tag}_g"], out[f"{tag}_64"], out[f"{tag}_g64"] = x, g, y64, gx64
        return {"E_ref": e, "E_gref": eg, "max_abs": float(np.abs(y64).max())}

    dcases = []
    for tag, name, static, lead, T, D in delta_cases():
        seed = SEEDS[name]
        m32, m64 = d.Delta(seed, static), d.Delta(seed, static, dtype=torch.float64)
        H = m64.window.size(0)
        shape = (T, D) if lead is None else (*lead, T, D)
        x, g = noise(*shape), noise(*shape[:-1], H * D)
        dcases.append({"tag": tag, "seed": name, "static_out": static, "lead": None if lead is None else list(lead), "T": T, "D": D, "H": H,
                       "N": HALF[name], **record(tag, m32, m64, x, g)})

    mcases = []
    for tag, name, lead, T, D in mlpg_cases():
        seed = SEEDS[name]
        m32, m64 = d.MLPG(T, seed), d.MLPG(T, seed, dtype=torch.float64)
        H = m64.M.size(1) // T
        u, g = noise(*lead, T, H * D), noise(*lead, T, D)
        mcases.append({"tag": tag, "seed": name, "lead": list(lead), "T": T, "D": D, "H": H, "N": HALF[name], **record(tag, m32, m64, u, g)})

    pcases = []
    for M, alpha, beta, onset, n in MCPF:
        for frames, lead in MCPF_LEADS.items():
            tag = f"mcpf_m{M}_a{alpha}_b{beta}_o{onset}_n{n}_f{frames}"
            m32, m64 = d.MelCepstrumPostfiltering(M, alpha, beta, onset, n), d.MelCepstrumPostfiltering(M, alpha, beta, onset, n, dtype=torch.float64)
            decay = (0.5 * np.exp(-np.arange(M + 1) / 6.0)).astype(np.float32)
            mc = noise(*lead, M + 1) * decay
            mc[..., 0] = 2 + 0.3 * mc[..., 0] / decay[0]
            mc, g = mc.astype(np.float32), noise(*lead, M + 1)
            pcases.append({"tag": tag, "M": M, "alpha": alpha, "beta": beta, "onset": onset, "ir_length": n, "frames": frames, "lead": list(lead),
                           **record(tag, m32, m64, mc, g)})

    # the docstring examples (delta.py:76-89, mlpg.py:80-100, mcpf.py:94-107)
    x = d.ramp(1, 8).view(1, -1, 2)
    y = d.Delta([[-0.5, 0], [0, 0, 0.5]])(x)
    c = d.MLPG(y.size(1), [[-0.5, 0], [0, 0, 0.5]])(y)
    assert np.allclose(y[0, 0].numpy(), [1, 2, -0.5, -1, 1.5, 2]) and np.allclose(c.numpy(), x.numpy(), atol=1e-5)
    mc1 = torch.tensor([-0.4989, 0.5941, 0.1558, -0.2130])
    mc2 = d.MelCepstrumPostfiltering(3, 0.1, 0.2)(mc1)
    assert np.allclose(mc2.numpy(), [-0.5097, 0.5941, 0.1869, -0.2556], atol=2e-4)
    doc = {"x": x.tolist(), "delta": y.tolist(), "mlpg": c.tolist(), "mc1": mc1.tolist(), "mcpf": mc2.tolist()}

    index, flat = {}, {"f64": [], "f32": []}
    for k, v in out.items():
        which = "f64" if v.dtype == np.float64 else "f32"
        assert v.dtype in (np.float64, np.float32)
        index[k] = [which, int(sum(a.size for a in flat[which])), list(v.shape)]
        flat[which].append(v.reshape(-1))
    np.savez_compressed(os.path.join(HERE, "paramgen.npz"), **{k: np.concatenate(v) for k, v in flat.items()})

    classes = ["Delta", "MaximumLikelihoodParameterGeneration", "MelCepstrumPostfiltering"]
    api = {"seeds": SEEDS, "doc": doc, "arrays": index, "delta_cases": dcases, "mlpg_cases": mcases, "mcpf_cases": pcases, "classes": {},
           "functional": {}, "aliases": {"MLPG": d.MLPG.__name__}, "state": {}, "errors": [], "departures": []}
    for cname in classes:
        cls = getattr(d, cname)
        api["classes"][cname] = {"init": sig(cls.__init__), "forward": sig(cls.forward), "func": sig(cls._func),
                                 "static": [n for n in ("_func", "_check", "_precompute", "_forward")
                                            if isinstance(inspect.getattr_static(cls, n), staticmethod)],
                                 "takes_input_size": bool(cls._takes_input_size)}
    for f in ("delta", "mlpg", "mcpf"):
        api["functional"][f] = sig(getattr(F, f))
    api["state"] = {"Delta": list(d.Delta().state_dict()), "MLPG": list(d.MLPG(8).state_dict()),
                    "MelCepstrumPostfiltering": list(d.MelCepstrumPostfiltering(4, 0.1, 0.2).state_dict())}

    def attempt(who, what, args, kw, shape):
        try:
            if what == "ctor":
                getattr(d, who)(*args, **kw)
            elif what == "call":
                getattr(d, who)(*args, **kw)(torch.zeros(shape))
            else:
                getattr(F, who)(torch.zeros(shape), *args, **kw)
            return ["ok", ""]
        except Exception as e:   # noqa: BLE001
            return [type(e).__name__, str(e)]

    errs = [("Delta", "ctor", ["x"], {}, None), ("Delta", "ctor", [3], {}, None), ("Delta", "ctor", [[0]], {}, None), ("Delta", "ctor", [[2, -1]], {}, None),
            ("Delta", "ctor", [[1, 1, 1]], {}, None), ("Delta", "call", [], {}, [2, 3, 4, 5]), ("Delta", "call", [], {}, [7]),
            ("delta", "functional", [], {"seed": "x"}, [4, 2]), ("delta", "functional", [], {"seed": [1, 2, 3]}, [4, 2]),
            ("delta", "functional", [], {}, [2, 2, 4, 2]),
            ("MLPG", "ctor", [8, [0]], {}, None), ("MLPG", "ctor", [8, [1, 1, 1]], {}, None), ("MLPG", "call", [5], {}, [4, 6]),
            ("MLPG", "call", [5], {}, [2, 6, 3]),
            ("MelCepstrumPostfiltering", "ctor", [4], {"onset": -1}, None), ("mcpf", "functional", [], {"onset": -2}, [3, 5])]
    for who, what, args, kw, shape in errs:
        got = attempt(who, what, args, kw, shape)
        assert got[0] != "ok", (who, what, args, kw)
        api["errors"].append({"who": who, "kind": what, "args": args, "kwargs": kw, "shape": shape, "raises": got})
    # where the library departs: what the reference does there, for the record
    deps = [("MLPG", "ctor", [1], {}, None), ("MLPG", "ctor", [5, [2, 3]], {}, None), ("mlpg", "functional", [], {}, [1, 3]),
            ("MelCepstrumPostfiltering", "ctor", [4], {"ir_length": 1}, None), ("MelCepstrumPostfiltering", "call", [4], {"ir_length": 1}, [5])]
    for who, what, args, kw, shape in deps:
        api["departures"].append({"who": who, "kind": what, "args": args, "kwargs": kw, "shape": shape, "raises": attempt(who, what, args, kw, shape)})
    assert api["departures"][0]["raises"][0] == api["departures"][1]["raises"][0] == "RuntimeError"
    with open(os.path.join(HERE, "paramgen_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")
    print(len(dcases), len(mcases), len(pcases), "cases;", os.path.getsize(os.path.join(HERE, "paramgen.npz")), "bytes;",
          "E_ref max", max(c["E_ref"] for c in dcases), max(c["E_ref"] for c in mcases), max(c["E_ref"] for c in pcases))
    for dep in api["departures"]:
        print(dep["who"], dep["args"], dep["kwargs"], dep["raises"][0], dep["raises"][1][:100])


if __name__ == "__main__":
    main()
