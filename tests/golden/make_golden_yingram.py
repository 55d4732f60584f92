#!/usr/bin/env python3
"""Golden fixtures of Yingram, by importing the REFERENCE.  Build container only (CPU; a few seconds).

    python tests/golden/make_golden_yingram.py     # writes tests/golden/yingram.npz and yingram_api.json (data)

Cases: the six option sets of yingram_ref.GRID, each with one set of noise frames and one of voiced-like frames (three harmonics of a
period inside the lag range plus 1 % noise), one silent frame, and Frame(64, 16) on a waveform of 200 samples with both `center`
values.  Inputs and cotangents are multiples of 2^-12 below 8 (stored as int16), so they are exact in float32.  Per case <name>:
<name>_xq, <name>_gq (the cotangent of y), and the reference's float64 <name>_y and <name>_gx (the gradient for that cotangent).  The JSON
holds per case E_ref = max |float32 - float64| of the reference's own y, E_gref the same of its gradient, and the deviation of the
restatement tests/yingram_ref.py from the reference's float64 (asserted <= 1e-10 here, relative to max(1, max |ref|)); further the
signatures, the root and functional names, the buffers' names and dtypes, the empty state_dict, the reference's exception type and
text for each invalid option set of yingram_ref.ERRORS, and M per option set, whose tables lags (float64 and float32 module), lags_floor
and lags_ceil are tab<k>_* of the npz.  The restatement's floor and ceiling tables are asserted equal to the reference's and its lags within
16 units in the last place (the grid of notes and the power of two round differently in NumPy and torch)."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402

import yingram_ref as R  # noqa: E402


def quantised(a):
    return np.clip(np.round(np.asarray(a) * 4096.0), -32000, 32000).astype(np.int16)


def noise(rng, F, L):
    return quantised(rng.normal(size=(F, L)) * 0.5)


def voiced(rng, F, L, lag_min, K):
    j = np.arange(L)
    rows = []
    for _ in range(F):
        period = rng.uniform(max(lag_min, 2) * 1.3, max(K * 0.6, max(lag_min, 2) * 1.4))
        phase = rng.uniform(0, 2 * np.pi, 3)
        rows.append(sum(a * np.sin(2 * np.pi * (h + 1) * j / period + phase[h]) for h, a in enumerate((0.5, 0.3, 0.2))) + 0.01 * rng.normal(size=L))
    return quantised(np.stack(rows))


def run_reference(diffsptk, x, gy, L, opts, dtype, frame=None):
    """(y, gx) of the reference in `dtype`, as float64 arrays; frame: (P, center) for a waveform input"""
    m = diffsptk.Yingram(L, dtype=dtype, **opts)
    t = torch.tensor(x, dtype=dtype, requires_grad=True)
    y = m(t if frame is None else diffsptk.Frame(L, frame[0], center=frame[1])(t))
    y.backward(torch.tensor(gy, dtype=dtype))
    return y.detach().double().numpy(), t.grad.double().numpy()


def deviation(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


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
    arrays, listed, worst, tabs = {}, [], 0.0, {}
    plan = []
    for k, (L, sr, lag_min, lag_max, n_bin, F) in enumerate(R.GRID):
        opts = dict(sample_rate=sr, lag_min=lag_min, lag_max=lag_max, n_bin=n_bin)
        plan += [(f"L{L}_{kind}", kind, L, F, opts, k, None) for kind in ("noise", "voiced")]
    fo = {q: R.FUSED[q] for q in ("sample_rate", "lag_min", "lag_max", "n_bin")}
    plan.append(("silent", "silent", 64, 1, fo, 1, None))
    plan += [(f"fused_center{int(c)}", "fused", R.FUSED["L"], 1, fo, 1, (R.FUSED["P"], c)) for c in (True, False)]
    for n, (name, kind, L, F, opts, tab, frame) in enumerate(plan):
        rng = np.random.default_rng(100 + n)
        lags, floor, ceil, K = R.tables(L, **opts)
        M = len(lags)
        if kind == "noise":
            xq = noise(rng, F, L)
        elif kind == "voiced":
            xq = voiced(rng, F, L, opts["lag_min"], K)
        elif kind == "silent":
            xq = np.zeros((1, L), dtype=np.int16)
        else:
            xq = noise(rng, 1, R.FUSED["T"])[0]
        x = xq.astype(np.float64) / 4096.0
        rows = F if frame is None else (R.FUSED["T"] - 1) // frame[0] + 1
        gq = quantised(rng.normal(size=(rows, M)))
        gy = gq.astype(np.float64) / 4096.0
        y64, g64 = run_reference(diffsptk, x, gy, L, opts, torch.float64, frame)
        y32, g32 = run_reference(diffsptk, x, gy, L, opts, torch.float32, frame)
        assert np.isfinite(y64).all() and np.isfinite(g64).all() and np.isfinite(y32).all() and np.isfinite(g32).all(), name
        if frame is None:
            mine_y, mine_g = R.forward(x, lags, floor, ceil, K), R.gradient(x, gy, lags, floor, ceil, K)
        else:
            fr = R.frames(x, L, *frame)
            mine_y = R.forward(fr, lags, floor, ceil, K)
            mine_g = R.unframe_adjoint(R.gradient(fr, gy, lags, floor, ceil, K), len(x), L, *frame)
        dev_y, dev_g = deviation(mine_y, y64), deviation(mine_g, g64)
        assert dev_y <= 1e-10 and dev_g <= 1e-10, (name, dev_y, dev_g)
        worst = max(worst, dev_y, dev_g)
        if kind == "silent":
            assert not y64.any() and not y32.any()
        ref = diffsptk.Yingram(L, dtype=torch.float64, **opts)
        ref32 = diffsptk.Yingram(L, dtype=torch.float32, **opts)
        assert np.abs(ref.lags.numpy() / lags - 1).max() <= 16 * 2.0 ** -52 and np.array_equal(ref.lags_floor.numpy(), floor) and np.array_equal(ref.lags_ceil.numpy(), ceil), name
        assert len(ref.ramp) + 1 == K
        tabs[tab] = dict(L=L, **opts, M=M)
        arrays.update({f"tab{tab}_lags64": ref.lags.numpy(), f"tab{tab}_lags32": ref32.lags.numpy(), f"tab{tab}_floor": floor, f"tab{tab}_ceil": ceil})
        arrays.update({f"{name}_xq": xq, f"{name}_gq": gq, f"{name}_y": y64, f"{name}_gx": g64})
        rec = dict(name=name, kind=kind, L=L, F=F, M=M, K=K, table=tab, **opts, frame=None if frame is None else [frame[0], bool(frame[1])],
                   E_ref=float(np.abs(y32 - y64).max()), E_gref=float(np.abs(g32 - g64).max()), dev_y=dev_y, dev_g=dev_g,
                   max_y=float(np.abs(y64).max()), max_g=float(np.abs(g64).max()))
        listed.append(rec)
        print(rec, flush=True)
    np.savez_compressed(os.path.join(HERE, "yingram.npz"), **arrays)

    cls = diffsptk.Yingram
    m32, m64 = cls(64), cls(64, dtype=torch.float64)
    api = {
        "signatures": {name: signature(getattr(cls, name)) for name in ("__init__", "forward")},
        "functional": signature(diffsptk.functional.yingram),
        "in_root": hasattr(diffsptk, "Yingram"),
        "buffers": {key: {k: str(v.dtype) for k, v in m.named_buffers()} for key, m in (("float32", m32), ("float64", m64))},
        "state_dict": sorted(m32.state_dict()),
        "errors": {name: raised(f, diffsptk) for name, f in R.ERRORS.items()},
        "index_errors": [raised(lambda d, kw=kw: d.Yingram(**kw)(torch.zeros(kw["frame_length"])), diffsptk) for kw in R.INDEX_ERRORS],
        "tables": {str(k): v for k, v in sorted(tabs.items())},
        "restatement_deviation": worst,
        "cases": listed,
    }
    assert all(r[0] != "ok" for r in api["errors"].values()), api["errors"]
    assert all(r[0] == "IndexError" for r in api["index_errors"]), api["index_errors"]
    with open(os.path.join(HERE, "yingram_api.json"), "w") as f:
        json.dump(api, f, indent=1)
        f.write("\n")
    print("wrote", len(listed), "cases;", os.path.getsize(os.path.join(HERE, "yingram.npz")), "bytes; restatement deviation", worst)


if __name__ == "__main__":
    main()
