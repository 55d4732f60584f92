#!/usr/bin/env python3
"""Golden fixtures of Aperiodicity (algorithm "tandem"), by importing the REFERENCE.  Build container only (CPU; about a minute).

    python tests/golden/make_golden_ap.py   # writes tests/golden/ap.npz and ap_api.json

The cases and the formulas of their inputs and cotangents are tests/ap_cases.py (all exact in float32).  Per case <name>, from the
reference in float64: <name>_y, <name>_gx (the gradient to x for the case's cotangent), the inputs <name>_x and <name>_f0 (float32) and the
integers the reference truncated, read off a replaced Tensor.int: <name>_int64 and <name>_int32, (n_band, 3, B, N) = t0, index_bias,
curr_pos (curr_pos broadcast over the batch) in the float64 and in the float32 run.  Where the two runs chose different integers the
float32 run is not comparable with the float64 one, and the JSON says so (same_decisions); a float32 result is then judged against the
restatement (tests/ap_ref.py) run with the float32 integers.

The JSON holds per case E_ref and E_gref (the reference's float32 run against its float64 run -- or against the restatement with the
float32 integers -- relative to max(1, max |ref|)), restatement_deviation (tests/ap_ref.py against the reference, float64), D_ulp (the
largest relative change of the float64 results when x and f0 move one unit in the last place at random, three draws, the integers
unchanged), the number of cholesky_ex calls of each run (n_band when every first trial succeeds), the half-integer margin, and per sample
rate the largest E_ref / E_gref of its cases (the float32 bounds of the GPU tests are four times these).  Further the signatures,
buffers, state_dict keys, the exception type and text of every invalid call of ap_cases.ERRORS, and what the reference returns on the
silent case.

Asserted here and again in tests/test_ap_cpu.py from the stored numbers: cholesky_ex succeeds at the first trial in both dtypes for every
case but the silent one, and every pitch + 0.5 and pitch / 2 + 0.5 stays 1e-3 from an integer."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import import_reference  # noqa: E402

import ap_cases as A  # noqa: E402
import ap_ref  # noqa: E402


class Tap:
    """Replaces Tensor.int and torch.linalg.cholesky_ex while a reference call runs."""

    def __enter__(self):
        self.ints, self.cholesky = [], 0
        self.saved = (torch.Tensor.int, torch.linalg.cholesky_ex)
        to_int, cholesky_ex = self.saved

        def my_int(t, *a, **kw):
            out = to_int(t, *a, **kw)
            self.ints.append(out.numpy().copy())
            return out

        def my_cholesky_ex(*a, **kw):
            self.cholesky += 1
            return cholesky_ex(*a, **kw)

        torch.Tensor.int, torch.linalg.cholesky_ex = my_int, my_cholesky_ex
        return self

    def __exit__(self, *exc):
        torch.Tensor.int, torch.linalg.cholesky_ex = self.saved

    def decisions(self, B, N):
        """(n_band, 3, B, N)"""
        return np.stack([np.stack([np.broadcast_to(v.reshape(-1, N), (B, N)) for v in self.ints[i:i + 3]]) for i in range(0, len(self.ints), 3)])


def run(diffsptk, name, dtype, x, f0, gy):
    args, kw = A.module_args(name)
    m = diffsptk.Aperiodicity(*args, **kw, dtype=dtype)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    with Tap() as tap:
        y = m(xt, torch.tensor(f0, dtype=dtype))
    (y * torch.tensor(gy, dtype=dtype)).sum().backward()
    return y.detach().double().numpy(), xt.grad.double().numpy(), tap.decisions(*f0.shape), tap.cholesky


def rel(a, ref):
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def restate(name, x, f0, gy, dtype=np.float64):
    (P, sr, L), kw = A.module_args(name)
    fmt = A.FORMATS[kw.pop("out_format")]
    detail = {}
    y, gx = ap_ref.aperiodicity(x, f0, P, sr, L, out_format=fmt, gy=gy, dtype=dtype, detail=detail, **kw)
    dec = np.stack([np.stack([f.t0, f.bias, np.broadcast_to(f.cpos, f.t0.shape)]) for f in detail["fits"]])
    return y, gx, dec


def nudge(v, rng):
    """every value one unit in its last place up or down, float64"""
    v = np.asarray(v, np.float64)
    return np.where(rng.integers(0, 2, v.shape) == 1, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))


def raised(f, d):
    try:
        f(d)
    except Exception as e:  # noqa: BLE001
        return [type(e).__name__, str(e)]
    return None


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def main():
    diffsptk = import_reference()
    out, cases = {}, []
    for name, c in A.CASES.items():
        x, f0 = A.inputs(name)
        (P, sr, L), kw = A.module_args(name)
        y64, gx64, int64, chol64 = run(diffsptk, name, torch.float64, x, f0, A.cotangent(name, (1,)))   # the shape first
        gy = A.cotangent(name, y64.shape)
        y64, gx64, int64, chol64 = run(diffsptk, name, torch.float64, x, f0, gy)
        y32, gx32, int32, chol32 = run(diffsptk, name, torch.float32, x, f0, gy)
        same = bool(np.array_equal(int64, int32))
        n_band = int64.shape[0]
        rec = dict(name=name, sr=sr, n_band=n_band, same_decisions=same, cholesky64=chol64, cholesky32=chol32, margin=A.half_integer_margin(name))
        out.update({f"{name}_x": x, f"{name}_f0": f0, f"{name}_y": y64, f"{name}_gx": gx64, f"{name}_int64": int64.astype(np.int32),
                    f"{name}_int32": int32.astype(np.int32)})
        assert rec["margin"] >= 1e-3, (name, rec["margin"])
        if name == A.SILENT:
            rec["reference_nan_y"] = int(np.isnan(y64).sum())
            rec["reference_nan_gx"] = int(np.isnan(gx64).sum())
            rec["y_size"] = int(y64.size)
        else:
            assert chol64 == chol32 == n_band, (name, chol64, chol32)   # every first trial succeeds
            ry, rgx, rdec = restate(name, x, f0, gy)
            assert np.array_equal(rdec, int64), name
            rec["restatement_deviation"] = max(rel(ry, y64), rel(rgx, gx64))
            if same:
                rec["E_ref"], rec["E_gref"] = rel(y32, y64), rel(gx32, gx64)
            else:   # the float32 run read other samples: its error is its distance from exact arithmetic on ITS integers
                ry32, rgx32, rdec32 = restate(name, x, f0, gy, np.float32)
                assert np.array_equal(rdec32, int32), name
                rec["E_ref"], rec["E_gref"] = rel(y32, ry32), rel(gx32, rgx32)
            rng = np.random.default_rng(7)
            worst = 0.0
            for _ in range(3):
                args, kw2 = A.module_args(name)
                m = diffsptk.Aperiodicity(*args, **kw2, dtype=torch.float64)
                xt = torch.tensor(nudge(x, rng), requires_grad=True)
                with Tap() as tap:
                    y = m(xt, torch.tensor(np.where(f0 <= 32, f0.astype(np.float64), nudge(f0, rng))))
                (y * torch.tensor(gy, dtype=torch.float64)).sum().backward()
                assert np.array_equal(tap.decisions(*f0.shape), int64), name
                worst = max(worst, rel(y.detach().numpy(), y64), rel(xt.grad.numpy(), gx64))
            rec["D_ulp"] = worst
        cases.append(rec)
        print(rec)
    groups = {str(sr): dict(E_ref=max(r["E_ref"] for r in cases if r["sr"] == sr and "E_ref" in r),
                            E_gref=max(r["E_gref"] for r in cases if r["sr"] == sr and "E_gref" in r)) for sr in A.GROUPS}
    cls = diffsptk.Aperiodicity
    buffers = {}
    for key, dtype in (("float32", None), ("float64", torch.float64)):
        for tag, L in (("bins", 64), ("bands", None)):
            m = cls(80, 16000, L, dtype=dtype)
            buffers[f"{key}_{tag}"] = {k: [str(v.dtype), list(v.shape)] for k, v in m.named_buffers()}
            if L:
                out.update({f"buffer_{key}_{k.split('.')[-1]}": v.numpy() for k, v in m.named_buffers() if "ramp" not in k})
    api = {
        "cases": cases,
        "groups": groups,
        "signatures": {n: signature(getattr(cls, n)) for n in ("__init__", "forward")},
        "buffers": buffers,
        "state_dict": sorted(cls(80, 16000, 64).state_dict()),
        "in_root": hasattr(diffsptk, "Aperiodicity"),
        "in_functional": hasattr(diffsptk.functional, "ap") or hasattr(diffsptk.functional, "aperiodicity"),
        "errors": {n: raised(f, diffsptk) for n, f in A.ERRORS.items()},
        "shortest_accepted_16k": [raised(lambda d: d.Aperiodicity(7, 16000, 64)(torch.zeros(1, T), torch.zeros(1, 2)), diffsptk) is None
                                  for T in (80, 81)],
    }
    np.savez_compressed(os.path.join(HERE, "ap.npz"), **out)
    with open(os.path.join(HERE, "ap_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")
    print(groups, os.path.getsize(os.path.join(HERE, "ap.npz")))


if __name__ == "__main__":
    main()
