#!/usr/bin/env python3
"""Golden fixtures of DynamicTimeWarping, by importing the REFERENCE.  Build container only (CPU; about four minutes).

    python tests/golden/make_golden_dtw.py     # writes tests/golden/dtw.npz and dtw_api.json (data)

Per case (the list, with every option and shape, is dtw_api.json["cases"]) the reference runs with B = 1 in float64 and in float32 on
the same values (every input is exact in float32).  dtw.npz holds two arrays per case:
  c<n>  float64: x (T1 D), y (T2 D), gx (T1 D), gy (T2 D), distance, E_ref, E_gref -- the float64 results with the gradient of the
        distance, E_ref = |distance32 - distance64| and E_gref = max |g32 - g64| over both gradients: the reference's own float32 error
  p<n>  int64 (T, 2): the float64 Viterbi path
An unreachable end has distance inf, zero gradients (the reference builds no graph there), the one-row path and E = 0.

Conditions, asserted here for EVERY case with a reachable end but the docstring's example, whose values are given (the seed of a case is
advanced until they hold; nothing is filtered at test time): the reference's float32 path equals its float64 path, and the smallest gap between the winning candidate and the runner-up
over the cells of the path (tests/dtw_ref.py, which must reproduce path, distance and gradients first) exceeds 1e-4 R[end] -- a float32
implementation that orders its sums differently then still takes the same path, and the gradient at softness 1e-3, which is the path's
indicator up to exp(-gap / softness), does not depend on the last place of R.

The size of the inputs: the tests bound a float32 result by 4 E_ref + 1e-6, and E_ref of one case can be small by luck.  The floor of
1e-6 has to cover what ANY float32 evaluation loses: about sqrt(N) roundings of R[end] / (T1 + T2) over the N cells of a path.  The
shapes of a hundred frames are therefore scaled to distances of order 1 and the shapes of a thousand rows to order 0.1
(sqrt(100) 2^-24 1 = 6e-7 and sqrt(1000) 2^-24 0.1 = 2e-7)."""
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

import dtw_ref  # noqa: E402

METRICS = ("manhattan", "euclidean", "squared-euclidean", "symmetric-kl")
GAMMAS = (1e-3, 0.1, 1.0)
SMALL = [(a, b) for a in (1, 2, 3) for b in (1, 2, 3, 4)] + [(7, 5), (5, 7), (4, 3)]   # (an odd count: every shape meets both D)
MARGIN = 1e-4


def cases():
    out, n = [], 0
    for p in range(7):   # every constraint x metric x softness x D, the small shapes taken in turn
        for metric in METRICS:
            for gamma in GAMMAS:
                for D in (1, 5):
                    T1, T2 = SMALL[n % len(SMALL)]
                    out.append(dict(p=p, metric=metric, gamma=gamma, D=D, T1=T1, T2=T2, lengths=None))
                    n += 1
    for p, T1, T2 in ((0, 33, 70), (1, 33, 70), (4, 33, 60), (5, 33, 60), (3, 70, 33), (6, 70, 33)):   # more columns than a wave has lanes; more rows
        for gamma in (1e-3, 0.1):
            out.append(dict(p=p, metric="euclidean", gamma=gamma, D=5, T1=T1, T2=T2, lengths=None))
    for T1 in (63, 64, 65):   # the wave route's edge
        out.append(dict(p=4, metric="euclidean", gamma=1e-3, D=5, T1=T1, T2=40, lengths=None))
        out.append(dict(p=5, metric="manhattan", gamma=0.1, D=5, T1=T1, T2=40, lengths=None))
    for T1 in (1024, 1025):   # one row per thread of the block route, and the first shape with two (p = 4 cannot reach the end of so narrow a grid)
        out.append(dict(p=1, metric="squared-euclidean", gamma=0.1, D=1, T1=T1, T2=6, lengths=None))
        out.append(dict(p=0, metric="symmetric-kl", gamma=1e-3, D=1, T1=T1, T2=6, lengths=None))
    for p, T1, T2, lengths in ((4, 7, 5, (5, 4)), (1, 5, 7, (1, 7)), (5, 33, 70, (30, 41)), (6, 65, 40, (64, 33)), (0, 3, 4, (3, 1))):   # truncating lengths
        out.append(dict(p=p, metric="euclidean", gamma=0.1, D=5, T1=T1, T2=T2, lengths=list(lengths)))
    out.append(dict(p=2, metric="euclidean", gamma=0.1, D=5, T1=3, T2=4, lengths=None, unreachable=True))
    out.append(dict(p=2, metric="manhattan", gamma=1e-3, D=1, T1=1, T2=2, lengths=None, unreachable=True))
    out.append(dict(p=5, metric="euclidean", gamma=0.1, D=5, T1=2, T2=6, lengths=None, unreachable=True))
    out.append(dict(p=5, metric="euclidean", gamma=0.1, D=5, T1=7, T2=5, lengths=[2, 5], unreachable=True))
    out.append(dict(p=1, metric="euclidean", gamma=1e-3, D=0, T1=4, T2=4, lengths=None, docstring=True))   # D = 0: (T,) inputs
    return out


def inputs(c, seed):
    if c.get("docstring"):
        return np.array([[1.0], [3.0], [6.0], [9.0]]), np.array([[2.0], [3.0], [8.0], [8.0]])
    rng = np.random.default_rng(seed)
    D = c["D"]
    if c["metric"] == "symmetric-kl":   # positive, quotients far from the clip
        x, y = rng.uniform(0.5, 2.0, (c["T1"], D)), rng.uniform(0.5, 2.0, (c["T2"], D))
    elif c["T1"] > 1000:   # a thousand accumulated cells: noise of a size that keeps R[end] of order 10 (below)
        x, y = 0.1 * rng.normal(size=(c["T1"], D)), 0.1 * rng.normal(size=(c["T2"], D))
    else:   # a slow common trend plus noise: alignments that are not the diagonal
        scale = 1.0 if c["T1"] + c["T2"] < 20 else 0.25
        x = scale * (np.cumsum(rng.normal(size=(c["T1"], D)), 0) * 0.5 + rng.normal(size=(c["T1"], D)))
        y = scale * (np.cumsum(rng.normal(size=(c["T2"], D)), 0) * 0.5 + rng.normal(size=(c["T2"], D)))
    return x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)


def run_reference(diffsptk, c, x, y, dtype):
    xt = torch.tensor(x[None] if x.ndim == 2 else x, dtype=dtype).requires_grad_()   # (B = 1, T, D), or (T,) as it is
    yt = torch.tensor(y[None] if y.ndim == 2 else y, dtype=dtype).requires_grad_()
    lengths = None if c["lengths"] is None else torch.tensor([c["lengths"]])
    dtw = diffsptk.DynamicTimeWarping(metric=c["metric"], p=c["p"], softness=c["gamma"])
    distance, indices = dtw(xt, yt, lengths, return_indices=True)
    if distance.requires_grad and bool(torch.isfinite(distance)):
        distance.sum().backward()
    gx = np.zeros_like(x) if xt.grad is None else xt.grad.double().numpy().reshape(x.shape)
    gy = np.zeros_like(y) if yt.grad is None else yt.grad.double().numpy().reshape(y.shape)
    return float(distance[0]), gx, gy, indices[0].numpy().astype(np.int64)


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
    arrays, listed = {}, []
    for n, c in enumerate(cases()):
        seed = 1000 * n
        while True:
            x, y = inputs(c, seed)
            xa, ya = (x[:, 0], y[:, 0]) if c.get("docstring") else (x, y)
            d64, gx64, gy64, path64 = run_reference(diffsptk, c, xa, ya, torch.float64)
            d32, gx32, gy32, path32 = run_reference(diffsptk, c, xa, ya, torch.float32)
            mine = dtw_ref.dtw(x, y, c["metric"], c["p"], c["gamma"], c["lengths"])
            assert not c.get("unreachable") or d64 == np.inf, c
            if d64 == np.inf:   # (many of the small shapes too: p = 2, 3, 6 with T1 < T2, p = 5 outside the 1:2 slope)
                c = dict(c, unreachable=True)
                assert d32 == np.inf and len(path64) == 1 and not gx64.any() and not gy64.any(), c
                assert mine["distance"] == np.inf and np.array_equal(mine["path"], path64), c
                e_ref = e_gref = 0.0
                break
            same = np.array_equal(path32, path64) and np.array_equal(mine["path"], path64)
            if same and (mine["margin"] > MARGIN * mine["end"] or c.get("docstring")):
                assert abs(mine["distance"] - d64) <= 1e-12 * max(1.0, abs(d64)), (c, mine["distance"], d64)
                e_ref = abs(d32 - d64)
                e_gref = max(np.abs(gx32 - gx64).max(), np.abs(gy32 - gy64).max())
                break
            assert not c.get("docstring"), "the docstring example does not meet the conditions"
            seed += 1
        gx64, gy64 = gx64.reshape(x.shape), gy64.reshape(y.shape)
        arrays[f"c{n}"] = np.concatenate([x.ravel(), y.ravel(), gx64.ravel(), gy64.ravel(), [d64, e_ref, e_gref]])
        arrays[f"p{n}"] = path64
        listed.append(dict(c, seed=seed))
        print(n, c, "seed", seed, "distance", d64, "E_ref", e_ref, "E_gref", e_gref, "margin", mine["margin"], flush=True)
    np.savez_compressed(os.path.join(HERE, "dtw.npz"), **arrays)

    api = {
        "classes": {"DynamicTimeWarping": {"init": signature(diffsptk.DynamicTimeWarping.__init__), "forward": signature(diffsptk.DynamicTimeWarping.forward),
                                           "_func": signature(diffsptk.DynamicTimeWarping._func), "merge": signature(diffsptk.DynamicTimeWarping.merge)}},
        "functional": {name: signature(getattr(diffsptk.functional, name)) for name in ("dtw", "dtw_merge")},
        "alias": diffsptk.DTW is diffsptk.DynamicTimeWarping,
        "errors": {name: raised(f, diffsptk) for name, f in dtw_ref.ERRORS.items()},
        "cases": listed,
    }
    assert all(r[0] != "ok" for r in api["errors"].values()), api["errors"]
    with open(os.path.join(HERE, "dtw_api.json"), "w") as f:
        json.dump(api, f, indent=1)
        f.write("\n")
    print("wrote", len(listed), "cases;", os.path.getsize(os.path.join(HERE, "dtw.npz")), "bytes")


if __name__ == "__main__":
    main()
