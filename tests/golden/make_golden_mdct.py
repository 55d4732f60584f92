#!/usr/bin/env python3
"""Golden fixtures of mdct / imdct / mdst / imdst, by importing the REFERENCE.  Build container only.

    python tests/golden/make_golden_mdct.py     # writes tests/golden/mdct.npz and mdct_api.json (data)

Inputs are unit-variance noise (numpy default_rng(0), one stream in the order of INPUTS), rounded to float32 so that both precisions
see the same values: per input `<name>_x` (lead..., T), the waveform; `<name>_g` (lead..., N, P), which is the cotangent of the analysis
AND the spectrum the synthesis cases start from AND, flattened to (lead..., N P), cut to its first T_out samples, the cotangent of the
synthesis (which is linear: its gradient does not depend on the spectrum it starts from).  Per case (input, direction, transform, out_length; the list is in mdct_api.json) the reference's float64 result `<tag>_64`
and float64 gradient `<tag>_g64`; the float32 results enter through E_ref = max |ref32 - ref64| and E_gref (the same for the gradient),
recorded per case, and as arrays `<tag>_32` / `<tag>_g32` only for frame lengths up to 6 -- no committed file may pass 1 MiB.  For the
same reason the npz holds two flat arrays, `f64` and `f32`, and mdct_api.json the index `arrays`: name -> [which, offset, shape] (a
thousand small members would cost 170 kB of headers).  Per input
and transform E_rt = max |imdct32(mdct32(x), out_length=T) - x|.

Conditions, asserted here:
  * every input is exactly representable in float32 and its largest magnitude is below 6;
  * the shapes are those of the closed forms: N = (T + P - 1) // P + 1 rows; T_out = (N - 1) P for out_length None, else
    min(out_length, N P);
  * the float32 reference is within 4 E_ref + 1e-6 of the float64 one by construction; E_ref itself stays below 1e-4 (a reference
    result that lost more than that would make the float32 bound meaningless);
  * the float64 round trip imdct(mdct(x), out_length=T) returns x to 1e-9 for every input and transform under the four windows of the
    reference's list ("hanning" does not satisfy the Princen-Bradley condition: no round trip is recorded as exact for it);
  * the list covers the grid of frame lengths, lengths, windows, transforms and out_length values that tests/test_mdct_cpu.py spells out."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

FAST_MIN, FAST_MAX = 16, 4096   # DSA_MDCT_FAST_MIN_LENGTH / _MAX_LENGTH of include/diffsptk_amd.h
BOTH = ["cosine", "sine"]
COS = ["cosine"]
ALL_OUT = ["none", "T", "NP", "NP+5", "(N-1)P+1"]
T_KINDS = ["1", "P-1", "P", "P+1", "3P+1"]


def t_of(kind, P):
    return {"1": 1, "P-1": max(P - 1, 1), "P": P, "P+1": P + 1, "3P+1": 3 * P + 1}[kind] if isinstance(kind, str) else kind


def inputs():
    """(name, L, window, lead, T kind, transforms, out_length kinds)"""
    rows = []
    for L in (2, 4, 6, FAST_MIN - 2, FAST_MIN):
        for kind in T_KINDS:
            rows.append((f"l{L}_t{kind}", L, "sine", (3,), kind, BOTH, ALL_OUT if kind == "3P+1" else ["T"]))
    for window in ("vorbis", "kbd", "rectangular", "hanning"):
        rows.append((f"l16_{window}", 16, window, (3,), "3P+1", BOTH, ["T", "none"]))
    rows.append(("l16_3d", 16, "sine", (2, 2), "3P+1", BOTH, ["T"]))
    for kind in T_KINDS:
        rows.append((f"l400_t{kind}", 400, "sine", (3,) if kind == "P-1" else (), kind, BOTH if kind == "3P+1" else COS, ["T"]))
        rows.append((f"l512_t{kind}", 512, "sine", (3,) if kind == "P-1" else (), kind, BOTH if kind == "3P+1" else COS,
                     ALL_OUT if kind == "1" else ["T"]))
    for window in ("vorbis", "kbd", "rectangular"):
        rows.append((f"l512_{window}", 512, window, (), "P+1", BOTH if window == "kbd" else COS, ["T"]))
    rows.append(("l512_long", 512, "sine", (), 15 * 256 + 1, COS, ["T"]))   # 17 frames: more than one tile of the fast kernels (16 frames)
    rows.append((f"l{FAST_MAX}", FAST_MAX, "sine", (), "3P+1", ["sine"], ["T"]))   # two tiles in either direction at the upper bound (the cosine
    # transform there: the leading-zeros test of tests/test_gpu_mdct.py; one more case of this size would pass the 1 MiB limit)
    rows.append((f"l{FAST_MAX + 2}", FAST_MAX + 2, "sine", (), "P-1", COS, ["T"]))
    return rows


def out_length_of(kind, T, N, P):
    return {"none": None, "T": T, "NP": N * P, "NP+5": N * P + 5, "(N-1)P+1": (N - 1) * P + 1}[kind]


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def main():
    d = import_reference()
    F = d.functional
    rng = np.random.default_rng(0)
    ana = {"cosine": d.MDCT, "sine": d.MDST}
    syn = {"cosine": d.IMDCT, "sine": d.IMDST}
    out, cases, rts = {}, [], []

    def noise(*shape):
        v = rng.standard_normal(shape).astype(np.float32)
        assert np.abs(v).max() < 6
        return v

    def run(mod, v, dt, cot, *args):
        """(result, gradient of <result, cot>) of the reference in dtype dt, as float64 arrays"""
        t = torch.tensor(v, dtype=dt, requires_grad=True)
        r = mod(t, *args)
        (r * torch.tensor(cot, dtype=dt)).sum().backward()
        return r.detach().double().numpy(), t.grad.double().numpy()

    for name, L, window, lead, kind, transforms, outs in inputs():
        P = L // 2
        T = t_of(kind, P)
        N = (T + P - 1) // P + 1
        x, g = noise(*lead, T), noise(*lead, N, P)
        out[f"{name}_x"], out[f"{name}_g"] = x, g
        small = L <= 6
        for tr in transforms:
            a32, a64 = ana[tr](L, window), ana[tr](L, window, dtype=torch.float64)
            s32, s64 = syn[tr](L, window), syn[tr](L, window, dtype=torch.float64)
            tag = f"{name}_{tr}_a"
            y32, gx32 = run(a32, x, torch.float32, g)
            y64, gx64 = run(a64, x, torch.float64, g)
            assert y64.shape == (*lead, N, P) and gx64.shape == x.shape
            e, eg = float(np.abs(y32 - y64).max()), float(np.abs(gx32 - gx64).max())
            assert e < 1e-4 and eg < 1e-4
            out[f"{tag}_64"], out[f"{tag}_g64"] = y64, gx64
            if small:
                out[f"{tag}_32"], out[f"{tag}_g32"] = y32.astype(np.float32), gx32.astype(np.float32)
            cases.append({"tag": tag, "input": name, "direction": "analysis", "transform": tr, "L": L, "window": window, "lead": list(lead),
                          "T": T, "T_kind": str(kind), "N": N, "E_ref": e, "E_gref": eg, "max_abs": float(np.abs(y64).max())})
            with torch.no_grad():
                x32 = torch.tensor(x)
                rt32 = s32(a32(x32), out_length=T)
                rt64 = s64(a64(x32.double()), out_length=T)
            assert rt64.shape == x32.shape and (window == "hanning" or float((rt64 - x32.double()).abs().max()) < 1e-9), name
            rts.append({"input": name, "transform": tr, "E_rt": float((rt32.double() - x32.double()).abs().max())})
            for ok in outs:
                ol = out_length_of(ok, T, N, P)
                T_out = (N - 1) * P if ol is None else min(ol, N * P)
                tag = f"{name}_{tr}_s_{ok}"
                cot = g.reshape(*lead, N * P)[..., :T_out]
                v32, gy32 = run(s32, g, torch.float32, cot, ol)
                v64, gy64 = run(s64, g, torch.float64, cot, ol)
                assert v64.shape == (*lead, T_out) and gy64.shape == g.shape
                e, eg = float(np.abs(v32 - v64).max()), float(np.abs(gy32 - gy64).max())
                assert e < 1e-4 and eg < 1e-4
                out[f"{tag}_64"], out[f"{tag}_g64"] = v64, gy64
                if small:
                    out[f"{tag}_32"], out[f"{tag}_g32"] = v32.astype(np.float32), gy32.astype(np.float32)
                cases.append({"tag": tag, "input": name, "direction": "synthesis", "transform": tr, "L": L, "window": window, "lead": list(lead),
                              "T": T, "T_kind": str(kind), "N": N, "out_kind": ok, "out_length": ol, "T_out": T_out, "E_ref": e, "E_gref": eg,
                              "max_abs": float(np.abs(v64).max())})

    # the docstring examples (mdct.py:82-88, mdst.py, imdct.py:83-89)
    doc = {"mdct": d.MDCT(frame_length=4)(d.ramp(3)).tolist(), "mdst": d.MDST(frame_length=4)(d.ramp(3)).tolist(),
           "imdct": d.IMDCT(frame_length=4, window="vorbis")(d.MDCT(frame_length=4, window="vorbis")(d.ramp(1, 4))).tolist()}
    assert np.allclose(doc["mdct"], [[-0.5, -0.2071], [-4.4142, -0.4142], [-1.0858, 2.6213]], atol=5e-5)
    assert np.allclose(doc["imdct"], [1, 2, 3, 4], atol=5e-5)
    index, flat = {}, {"f64": [], "f32": []}
    for k, v in out.items():
        which = "f64" if v.dtype == np.float64 else "f32"
        assert v.dtype in (np.float64, np.float32)
        index[k] = [which, int(sum(a.size for a in flat[which])), list(v.shape)]
        flat[which].append(v.reshape(-1))
    np.savez_compressed(os.path.join(HERE, "mdct.npz"), **{k: np.concatenate(v) for k, v in flat.items()})

    classes = ["ModifiedDiscreteCosineTransform", "ModifiedDiscreteSineTransform", "InverseModifiedDiscreteCosineTransform",
               "InverseModifiedDiscreteSineTransform", "ModifiedDiscreteTransform", "InverseModifiedDiscreteTransform"]
    api = {"fast_min": FAST_MIN, "fast_max": FAST_MAX, "doc": doc, "arrays": index, "cases": cases, "round_trips": rts, "classes": {}, "functional": {},
           "aliases": {a: getattr(d, a).__name__ for a in ("MDCT", "IMDCT", "MDST", "IMDST")}, "state": {}, "errors": []}
    for c in classes:
        cls = getattr(d.modules.mdct if c == "ModifiedDiscreteTransform" else d.modules.imdct if c == "InverseModifiedDiscreteTransform" else d, c)
        api["classes"][c] = {"init": sig(cls.__init__), "forward": sig(cls.forward), "func": sig(cls._func),
                             "static": [n for n in ("_func", "_check", "_precompute", "_forward")
                                        if isinstance(inspect.getattr_static(cls, n), staticmethod)]}
    for f in ("mdct", "imdct", "mdst", "imdst"):
        api["functional"][f] = sig(getattr(F, f))
    for c in ("MDCT", "MDST", "IMDCT", "IMDST"):
        for key, learnable in (("False", False), ("True", True), ("basis", ["basis"]), ("window", ["window"]), ("both", ["window", "basis"])):
            api["state"][f"{c}/{key}"] = list(getattr(d, c)(8, learnable=learnable).state_dict())
    errs = [("MDCT", "ctor", [3], {}, None), ("MDCT", "ctor", [0], {}, None), ("MDCT", "ctor", [1], {}, None), ("IMDCT", "ctor", [5], {}, None),
            ("MDST", "ctor", [7], {}, None), ("IMDST", "ctor", [-2], {}, None),
            ("MDCT", "ctor", [8], {"learnable": ["basis", "gain"]}, None), ("IMDCT", "ctor", [8], {"learnable": ["twiddle"]}, None),
            ("MDST", "ctor", [8], {"learnable": ("x",)}, None), ("MDCT", "ctor", [8], {"learnable": "basis"}, None),
            ("IMDST", "ctor", [8], {"learnable": 1}, None), ("MDCT", "ctor", [8], {"learnable": None}, None),
            ("MDCT", "ctor", [8], {"window": "triangle"}, None),
            ("IMDCT", "call", [8], {}, [4]), ("IMDST", "call", [8], {}, [4]),
            ("mdct", "functional", [], {"frame_length": 9}, [20]), ("mdst", "functional", [], {"frame_length": 0}, [20]),
            ("imdct", "functional", [], {"frame_length": 8}, [4]), ("imdst", "functional", [], {"frame_length": 8}, [4])]
    for who, what, args, kw, shape in errs:
        try:
            if what == "ctor":
                getattr(d, who)(*args, **kw)
            elif what == "call":
                getattr(d, who)(*args, **kw)(torch.zeros(shape))
            else:
                getattr(F, who)(torch.zeros(shape), *args, **kw)
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        assert got[0] != "ok", (who, what, args, kw)
        api["errors"].append({"who": who, "kind": what, "args": args, "kwargs": kw, "shape": shape, "raises": got})
    with open(os.path.join(HERE, "mdct_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases;", os.path.getsize(os.path.join(HERE, "mdct.npz")), "bytes")


if __name__ == "__main__":
    main()
