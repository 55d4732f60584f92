#!/usr/bin/env python3
"""Golden fixtures of AllPoleDigitalFilter / functional.poledf, by importing the REFERENCE.  Build container only.

The reference delegates the recursion to torchlpc.sample_wise_lpc (poledf.py:106,137), which is not installed; a stand-in module
is put into sys.modules first: the definition y[t] = x[t] - sum_k A[t, k-1] y[t - k] as a float64 torch loop, differentiated by
autograd.  Everything around it -- interpolation, gain, shape checks, error texts -- is the reference's own code.

    python tests/golden/make_golden_poledf.py     # writes tests/golden/poledf.npz and poledf_api.json (data)
"""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def sample_wise_lpc(x, A):
    """x:(B, T), A:(B, T, M) -> y:(B, T), zero initial state."""
    assert x.dim() == 2 and A.dim() == 3 and A.shape[:2] == x.shape
    M = A.size(-1)
    ys = []
    for t in range(x.size(-1)):
        v = x[:, t]
        for k in range(1, min(M, t) + 1):
            v = v - A[:, t, k - 1] * ys[t - k]
        ys.append(v)
    return torch.stack(ys, dim=-1)


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def coefficients(rng, shape, M):
    """Stable filters: sum_k |a_k| <= 0.6, gains in [0.5, 1.5]."""
    a = rng.uniform(-1.0, 1.0, shape) * (0.6 / max(M, 1))
    a[..., 0] = rng.uniform(0.5, 1.5, shape[:-1])
    return a


def main():
    stub = types.ModuleType("torchlpc")
    stub.sample_wise_lpc = sample_wise_lpc
    sys.modules["torchlpc"] = stub
    d = import_reference()
    rng = np.random.default_rng(20240901)
    out = {}
    frames = {1: 24, 7: 5, 80: 2}
    for M in (0, 1, 3, 24):
        for P in (1, 7, 80):
            N = frames[P]
            for ig in (0, 1):
                for dim in (1, 2):
                    if dim == 1 and ig:   # 1-D inputs once per (M, P)
                        continue
                    lead = () if dim == 1 else (2,)
                    x = torch.tensor(rng.standard_normal((*lead, N * P)), requires_grad=True)
                    a = torch.tensor(coefficients(rng, (*lead, N, M + 1), M), requires_grad=True)
                    gy = torch.tensor(rng.standard_normal((*lead, N * P)))
                    y = d.AllPoleDigitalFilter(M, P, ignore_gain=bool(ig))(x, a)
                    y.backward(gy)
                    key = f"M{M}_P{P}_ig{ig}_d{dim}"
                    ga = a.grad if a.grad is not None else torch.zeros_like(a)   # M = 0 with ignore_gain: y does not depend on a
                    for name, v in (("x", x), ("a", a), ("gy", gy), ("y", y), ("gx", x.grad), ("ga", ga)):
                        out[f"{key}_{name}"] = v.detach().numpy()
    # the reference's docstring example
    x = d.step(4).double()
    a = d.ramp(4).double().view(-1, 1)
    out["doc_x"], out["doc_a"] = x.numpy(), a.numpy()
    out["doc_y"] = d.AllPoleDigitalFilter(0, 1)(x, a).numpy()
    np.savez(os.path.join(HERE, "poledf.npz"), **out)

    api = {"init": sig(d.AllPoleDigitalFilter.__init__), "forward": sig(d.AllPoleDigitalFilter.forward),
           "functional": sig(d.functional.poledf), "errors": []}
    cases = [
        ("ctor", [-1, 80], {}, None),
        ("ctor", [24, 0], {}, None),
        ("call", [3, 8], {}, ((2, 16), (2, 2, 5))),       # wrong coefficient dimension
        ("call", [3, 8], {}, ((2, 17), (2, 2, 4))),       # sequence length
        ("call", [3, 8], {}, ((2, 2, 16), (2, 2, 2, 4))),   # 4-D coefficients
        ("functional", [], {"frame_period": 0}, ((16,), (2, 4))),
        ("functional", [], {"frame_period": 8}, ((15,), (2, 4))),
    ]
    for kind, args, kwargs, shapes in cases:
        try:
            if kind == "ctor":
                d.AllPoleDigitalFilter(*args, **kwargs)
            elif kind == "call":
                d.AllPoleDigitalFilter(*args, **kwargs)(torch.zeros(shapes[0], dtype=torch.float64), torch.zeros(shapes[1], dtype=torch.float64))
            else:
                d.functional.poledf(torch.zeros(shapes[0], dtype=torch.float64), torch.zeros(shapes[1], dtype=torch.float64), **kwargs)
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        api["errors"].append({"kind": kind, "args": args, "kwargs": kwargs, "shapes": shapes, "raises": got})
    with open(os.path.join(HERE, "poledf_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
