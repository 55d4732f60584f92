#!/usr/bin/env python3
"""Golden fixtures of PQMF / IPQMF / Decimation / Interpolation, by importing the REFERENCE.  Build container only.

    python tests/golden/make_golden_pqmf.py     # writes tests/golden/pqmf.npz and pqmf_api.json (data)

Inputs are closed-form (`wave` below; tests/test_gpu_pqmf.py restates it), so the files hold the reference's results only: filters
and convergence flags, float64 outputs and input gradients of sum(w * out) (w closed-form too) for the four routes, filter gradients
of learnable banks, the signatures, errors, warning and state-dict keys, and the README's subband example on data.wav."""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

BANDS = (1, 2, 3, 4, 8)
FILTER_ORDERS = (2, 3, 4, 5, 8, 11, 17, 24, 40, 62, 63)
OPTIONS = [{}, {"alpha": 50}, {"alpha": 20}, {"alpha": 40, "n_iter": 5}, {"step_size": 1e-3}, {"decay": 0.9}, {"eps": 1e-3},
           {"eps": 0.0, "n_iter": 3}]
FORMS = {"pqmf": ("1d", "2d", "3d"), "pqmf_dec": ("1d", "2d", "3d"), "ipqmf": ("2d", "3d"), "interp_ipqmf": ("2d", "3d")}


def wave(shape, seed):
    n = np.arange(int(np.prod(shape)), dtype=np.float64)
    return (np.sin(0.0123 * (seed + 1) * n + seed) + 0.3 * np.cos(0.71 * n + 0.2 * seed)).reshape(shape)


def cases():
    out = []
    for K, M in ((4, 40), (3, 7), (2, 62)):
        for T in (1, 3, 17):   # 17: shorter than the pads of M = 40 / 62
            for route, forms in FORMS.items():
                for n, form in enumerate(forms):
                    plain = route in ("pqmf", "ipqmf")
                    out.append([K, M, T, route, 1 if plain else K, 0 if plain else n % 2 + (T == 17), form, T == 17])
    for route in FORMS:
        plain = route in ("pqmf", "ipqmf")
        out.append([4, 40, 4801, route, 1 if plain else 4, 0 if plain else 2, "1d" if route.startswith("pqmf") else "2d", False])
    return out


def run(d, K, M, T, route, P, s, form, learnable):
    if route.startswith("pqmf"):
        m = d.PQMF(K, M, learnable=learnable, dtype=torch.float64)
        shape = {"1d": (T,), "2d": (2, T), "3d": (2, 1, T)}[form]
    else:
        m = d.IPQMF(K, M, learnable=learnable, dtype=torch.float64)
        shape = {"2d": (K, T), "3d": (2, K, T)}[form]
    x = torch.tensor(wave(shape, 1), requires_grad=True)
    if route == "pqmf":
        out = m(x)
    elif route == "pqmf_dec":
        out = d.Decimation(P, s)(m(x))
    elif route == "ipqmf":
        out = m(x)
    else:
        out = m(d.Interpolation(P, s)(x))
    (out * torch.tensor(wave(tuple(out.shape), 2))).sum().backward()
    return out.detach().numpy(), x.grad.numpy(), None if not learnable else m.filters.grad.numpy()


def sig(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def main():
    d = import_reference()
    from diffsptk.modules.pqmf import make_filter_banks

    out = {}
    conv = np.zeros((len(BANDS), 62, 2), dtype=np.int8)
    for a, K in enumerate(BANDS):
        for b, M in enumerate(range(2, 64)):
            for c, mode in enumerate(("analysis", "synthesis")):
                h, ok = make_filter_banks(K, M, mode)
                conv[a, b, c] = ok
                if M in FILTER_ORDERS:
                    out[f"filt_{K}_{M}_{mode}_0"] = h
    for oi, opt in enumerate(OPTIONS[1:], 1):
        for K, M in ((4, 40), (2, 11)):
            for mode in ("analysis", "synthesis"):
                h, ok = make_filter_banks(K, M, mode, **opt)
                out[f"filt_{K}_{M}_{mode}_{oi}"] = h
                out[f"conv_{K}_{M}_{mode}_{oi}"] = np.array(ok)
    out["converged"] = conv

    case_list = cases()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (K, M, T, route, P, s, form, learnable) in enumerate(case_list):
            y, gx, gf = run(d, K, M, T, route, P, s, form, learnable)
            out[f"case{i}_out"], out[f"case{i}_gin"] = y, gx
            if learnable:
                out[f"case{i}_gf"] = gf

    # README.md:269-295 of the reference, on data.wav as diffsptk.read gives it (float32 in [-1, 1))
    pcm = np.load(os.path.join(HERE, "datawav.npz"))["pcm"]
    x = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
    K, M = 4, 40
    pqmf = d.PQMF(K, M)
    decimate = d.Decimation(K)
    y = decimate(pqmf(x))
    interpolate = d.Interpolation(K)
    ipqmf = d.IPQMF(K, M)
    x_hat = ipqmf(interpolate(K * y)).reshape(-1)
    error = (x_hat - x).abs().sum()
    out["readme_x_hat"] = x_hat.numpy()
    out["readme_error"] = np.array([float(error), float((x_hat - x).abs().max())])
    print("README example: sum |x_hat - x| =", float(error), " max =", float((x_hat - x).abs().max()))
    np.savez_compressed(os.path.join(HERE, "pqmf.npz"), **out)

    classes = {"PQMF": d.PQMF, "IPQMF": d.IPQMF, "Decimation": d.Decimation, "Interpolation": d.Interpolation}
    api = {"classes": {n: {"init": sig(c.__init__), "forward": sig(c.forward)} for n, c in classes.items()},
           "functional": {"decimate": sig(d.functional.decimate), "interpolate": sig(d.functional.interpolate)},
           "bands": BANDS, "filter_orders": FILTER_ORDERS, "options": OPTIONS, "cases": case_list, "errors": [], "warnings": []}
    errors = [
        ("ctor", "PQMF", [0, 40], {}, None), ("ctor", "PQMF", [4, 1], {}, None), ("ctor", "PQMF", [4, 40], {"alpha": 0}, None),
        ("ctor", "PQMF", [4, 40], {"n_iter": 0}, None), ("ctor", "PQMF", [4, 40], {"step_size": 0}, None),
        ("ctor", "PQMF", [4, 40], {"decay": -1}, None), ("ctor", "PQMF", [4, 40], {"eps": -1e-3}, None),
        ("ctor", "PQMF", [0, 1], {"alpha": 0}, None), ("ctor", "IPQMF", [0, 40], {}, None), ("ctor", "IPQMF", [4, 1], {}, None),
        ("ctor", "IPQMF", [4, 40], {"alpha": -3}, None), ("ctor", "IPQMF", [4, 40], {"n_iter": -1}, None),
        ("ctor", "Decimation", [0], {}, None), ("ctor", "Decimation", [2, -1], {}, None), ("ctor", "Decimation", [0, -1], {}, None),
        ("ctor", "Interpolation", [0], {}, None), ("ctor", "Interpolation", [2, -1], {}, None),
        ("call", "PQMF", [4, 40], {}, [2, 1, 1, 8]), ("call", "IPQMF", [4, 40], {}, [8]), ("call", "IPQMF", [4, 40], {}, [1, 2, 4, 8]),
        ("call", "Decimation", [2, 0, 2], {}, [4, 8]), ("call", "Decimation", [2, 0, -3], {}, [4, 8]),
        ("call", "Interpolation", [2, 0, 2], {}, [4, 8]), ("call", "Interpolation", [2, 1, -3], {}, [4, 8]),
        ("functional", "decimate", [], {"period": 0}, [8]), ("functional", "decimate", [], {"period": 2, "dim": 1}, [8]),
        ("functional", "interpolate", [], {"period": 2, "start": -1}, [8]), ("functional", "interpolate", [], {"period": 0}, [8]),
    ]
    for kind, name, args, kwargs, shape in errors:
        try:
            if kind == "ctor":
                classes[name](*args, **kwargs)
            elif kind == "call":
                classes[name](*args, **kwargs)(torch.zeros(shape, dtype=torch.float64))
            else:
                getattr(d.functional, name)(torch.zeros(shape, dtype=torch.float64), *args, **kwargs)
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        assert got[0] != "ok", (kind, name, args, kwargs)
        api["errors"].append({"kind": kind, "module": name, "args": args, "kwargs": kwargs, "shape": shape, "raises": got})
    for name, args in (("PQMF", [4, 2]), ("IPQMF", [4, 2]), ("PQMF", [4, 40]), ("IPQMF", [2, 11])):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            classes[name](*args)
        api["warnings"].append({"module": name, "args": args, "messages": [str(r.message) for r in rec]})
    api["state"] = {}
    for tag, m in (("PQMF", d.PQMF(4, 40)), ("PQMF_learnable", d.PQMF(4, 40, learnable=True)), ("IPQMF", d.IPQMF(4, 40)),
                   ("IPQMF_learnable", d.IPQMF(4, 40, learnable=True))):
        api["state"][tag] = {k: list(v.shape) for k, v in m.state_dict().items()}
    api["short_input_shape"] = list(d.PQMF(4, 40)(torch.ones(1, 3)).shape)
    with open(os.path.join(HERE, "pqmf_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
