#!/usr/bin/env python3
"""Golden fixtures of GaussianMixtureModeling, by importing the REFERENCE.  Build container only (CPU; about a minute).

    python tests/golden/make_golden_gmm.py     # writes tests/golden/gmm.npz and gmm_api.json (data)

Per case (options and shapes: gmm_api.json["cases"]) the reference trains in float64 and in float32 from the same recorded initial
(w, mu, sigma), given to set_params, on the same x; x is a multiple of 2^-8 below 128 (stored as int16) and the initial parameters
are float32 values, so every input is exact in float32.  gmm.npz holds per case c<n>_<name>: xq, init_w / init_mu / init_sigma,
ubm_* for MAP, the float64 w, mu, sigma, loglik and posterior (rows ::post_stride of it for the larger cases), and per transform
t<j>: its x, y, indices and log_prob under the float64 parameters.  The JSON holds the iterations run, E_ref[quantity] = max |f32 - f64| of the
reference itself, nmax = the largest |numer| of the final E-step, and whether the components overlap.

Conditions, asserted here for EVERY case (the case's seed is advanced until they hold; nothing is filtered at test time):
  * every component keeps a posterior mass of at least 2 at every iteration, and every Cholesky succeeds in both precisions;
  * the float32 and float64 runs stop at the same iteration, and |change - eps| exceeds 8 E_ref[loglik] at every iteration but the
    first (whose change is infinite);
  * transform inputs are rows whose winning posterior leads the runner-up by more than 1e-2 (selected here, so indices compare exactly;
    the tests then require 1e-3);
  * at least half the cases have overlapping components: at least 10 % of the vectors have a largest posterior below 0.99.

The restatement tests/gmm_ref.py is compared with every float64 result here; the largest deviation, relative to max(1, max |ref|) of the
quantity, was 1.3e-13 (the posterior of the largest case, after eight iterations); tests use 16 times that, 2.1e-12.

The float32 bound of the GPU tests is 4 E_ref + floor max(1, max |ref|).  E_ref of one case can be small by luck, so the floor has to
cover what ANY float32 evaluation loses, whatever its order of summation: each of the moment sums z, px, pxx adds T products, a random
walk of sqrt(T) roundings of 2^-24 relative to the sum; each numer[t, k] is made of R products and sums (R = L (L + 3) / 2 + 4 for a
triangular factor, 3 L + 4 on the diagonal route), sqrt(R) roundings relative to its size, at most nmax, and an absolute error of
numer is a relative error of the posterior; an iteration feeds both into the next, so they are counted once per iteration run:
    floor = 2^-24 (sqrt(T) + sqrt(R) nmax) n_run.
The inputs are sized for it: |x| of a few units, variances of order 1, so that no covariance is a small difference of large moments
(pxx / z - mu mu^T with |mu|^2 of the order of the variance) and max |ref| of the parameters is of order 1.  For the largest case
(T = 4000, L = 25, 8 iterations) the floor is about 5e-4; a wrong kernel misses by orders of magnitude more."""
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

import gmm_ref  # noqa: E402


def case(L, K, T, n_iter, var_type="diag", block_size=None, alpha=0.0, weight_floor=1e-5, var_floor=1e-6, eps=0.0, spread=2.0, transforms=(),
         **extra):
    return dict(L=L, K=K, T=T, n_iter=n_iter, var_type=var_type, block_size=block_size, alpha=alpha, weight_floor=weight_floor,
                var_floor=var_floor, eps=eps, spread=spread, transforms=list(transforms), **extra)


def cases():
    return [
        # the diagonal route
        case(1, 1, 10, 1),
        case(2, 2, 63, 2, transforms=(1, 2)),
        case(3, 3, 64, 2, transforms=(1, 2, 3)),
        case(5, 8, 65, 8, spread=3.0),                                   # T a few times K
        case(25, 16, 1100, 8, spread=2.5),
        case(50, 2, 257, 2, spread=1.0),
        case(5, 3, 1100, 8, stop_early=3),                              # the fourth iteration's change is below eps
        case(2, 4, 64, 2, weight_floor=0.125, floors_a_weight=True),    # weight_floor = 1 / (2 K) floors the fourth component
        case(3, 2, 65, 2, var_floor=1e-3, constant_column=2),           # a constant column: its variance lands on var_floor
        # the general route
        case(1, 1, 10, 1, "full"),
        case(2, 2, 63, 2, "full", transforms=(1, 2)),
        case(3, 3, 64, 2, "full", transforms=(1, 2, 3)),
        case(5, 2, 65, 2, "full"),
        case(5, 8, 257, 8, "full", spread=3.0),
        case(25, 16, 4000, 8, "full", spread=2.5, transforms=(12,)),    # the largest
        case(50, 1, 257, 2, "full"),
        case(50, 2, 1100, 1, "full", spread=1.0, transforms=(25,)),
        case(4, 3, 257, 2, "diag", [2, 2]),                              # the diagonals of the cross blocks stay
        case(6, 2, 64, 2, "diag", [3, 3]),
        case(5, 3, 1100, 2, "diag", [2, 3]),
        case(5, 3, 257, 2, "full", [2, 3], transforms=(2,)),
        case(5, 3, 1100, 8, "full", stop_early=4),
        # MAP adaptation from a background model
        case(3, 3, 64, 2, alpha=0.5),
        case(5, 2, 65, 2, alpha=1.0),
        case(3, 3, 257, 2, "full", alpha=0.5),
        case(5, 2, 64, 2, "full", [2, 3], alpha=1.0),
    ]


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def inputs(c, seed):
    rng = np.random.default_rng(seed)
    L, K, T = c["L"], c["K"], c["T"]
    centres = rng.normal(size=(K, L)) * c["spread"] / np.sqrt(L)
    scales = rng.uniform(0.6, 1.2, size=(K, L))
    if c.get("floors_a_weight"):
        members = np.concatenate([rng.integers(0, K - 1, T - 5), np.full(5, K - 1)])
    else:
        members = rng.integers(0, K, T)
    mix = rng.normal(size=(L, L)) * 0.3 / np.sqrt(L) + np.eye(L) if c["var_type"] == "full" or c["block_size"] else np.eye(L)
    x = centres[members] + (rng.normal(size=(T, L)) * scales[members]) @ mix.T
    if c.get("constant_column") is not None:
        x[:, c["constant_column"]] = 0.5
    xq = np.clip(np.round(x * 256.0), -32000, 32000).astype(np.int16)
    w = rng.uniform(0.8, 1.2, K)
    init = (f32(w / w.sum()), f32(centres + 0.3 * rng.normal(size=(K, L)) / np.sqrt(L)),
            f32(np.tile(1.3 * np.eye(L) + (0.2 if gmm_ref.make_mask(L, c["var_type"], c["block_size"]).sum() > L else 0.0), (K, 1, 1))))
    ubm = None
    if c["alpha"]:
        u = rng.uniform(0.8, 1.2, K)
        ubm = (f32(u / u.sum()), f32(centres + 0.5 * rng.normal(size=(K, L)) / np.sqrt(L)), f32(np.tile(1.5 * np.eye(L) + 0.1, (K, 1, 1))))
    return xq, init, ubm


def run_reference(diffsptk, c, x, init, ubm, dtype, eps):
    t = lambda a: torch.tensor(a, dtype=dtype)   # noqa: E731
    gmm = diffsptk.GMM(c["L"] - 1, c["K"], n_iter=c["n_iter"], eps=eps, weight_floor=c["weight_floor"], var_floor=c["var_floor"],
                       var_type=c["var_type"], block_size=c["block_size"], ubm=None if ubm is None else tuple(map(t, ubm)), alpha=c["alpha"],
                       dtype=dtype)
    gmm.set_params(tuple(map(t, init)))
    seen = []
    inner = gmm._e_step

    def counted(*args, **kwargs):
        post, ll = inner(*args, **kwargs)
        seen.append((float(post.sum(0).min()), float(ll)))
        return post, ll

    gmm._e_step = counted
    (w, mu, sigma), post, ll = gmm(t(x), return_posterior=True)
    n_run = len(seen) - 1
    totals = [s[1] for s in seen[:n_run]]
    return dict(w=w.double().numpy(), mu=mu.double().numpy(), sigma=sigma.double().numpy(), posterior=post.double().numpy(), loglik=float(ll),
                n_run=n_run, mass=min(s[0] for s in seen), changes=list(np.diff(totals)))


def run_transform(diffsptk, c, dtype, params, xt):
    gmm = diffsptk.GMM(c["L"] - 1, c["K"], var_type=c["var_type"], block_size=c["block_size"], dtype=dtype)   # a fresh model: trained buffers are inference tensors
    gmm.set_params(tuple(torch.tensor(p, dtype=dtype) for p in params))
    y, idx, lp = gmm.transform(torch.tensor(xt, dtype=dtype))
    return None if y is None else y.double().numpy(), idx.numpy(), lp.double().numpy()


def deviation(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


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
    arrays, listed, worst = {}, [], (0.0, (-1, ""))
    for n, c in enumerate(cases()):
        seed = 1000 * n
        while True:
            assert seed < 1000 * n + 200, ("no seed meets the conditions", c)
            xq, init, ubm = inputs(c, seed)
            x = xq.astype(np.float64) / 256.0
            opts = dict(gmm_ref.options(c), ubm=ubm)
            eps = c["eps"]
            try:
                if c.get("stop_early"):   # a threshold between two consecutive changes of a run that does not stop
                    free = gmm_ref.train(x, *init, **dict(opts, eps=0.0))["changes"]
                    eps = float(f"{np.sqrt(free[c['stop_early'] - 1] * free[c['stop_early']]):.3g}")
                    opts["eps"] = eps
                mine = gmm_ref.train(x, *init, **opts)
                r64 = run_reference(diffsptk, c, x, init, ubm, torch.float64, eps)
                r32 = run_reference(diffsptk, c, x, init, ubm, torch.float32, eps)
            except (np.linalg.LinAlgError, torch.linalg.LinAlgError):
                seed += 1
                continue
            e_ref = {q: float(np.abs(r32[q] - r64[q]).max()) for q in gmm_ref.QUANTITIES}
            margin = min([abs(ch - eps) for ch in r64["changes"]] + [np.inf])
            ok = (min(r64["mass"], r32["mass"], mine["mass"]) >= 2.0 and r64["n_run"] == r32["n_run"] == mine["n_run"]
                  and margin > 8 * e_ref["loglik"] and np.isfinite(r32["loglik"]))
            if c.get("stop_early"):
                ok = ok and r64["n_run"] == c["stop_early"] + 1 < c["n_iter"]
            elif ok:
                assert r64["n_run"] == c["n_iter"], c
            if c.get("floors_a_weight"):
                ok = ok and mine["raw_w"] < c["weight_floor"]
            if c.get("constant_column") is not None:
                ok = ok and np.all(r64["sigma"][:, c["constant_column"], c["constant_column"]] == c["var_floor"])
            if ok:
                break
            seed += 1
        for q in gmm_ref.QUANTITIES:
            dev = deviation(mine[q], r64[q])
            worst = max(worst, (dev, (n, q)))
            assert dev <= 1e-10, (c, q, dev)
        overlap = bool((r64["posterior"].max(1) < 0.99).mean() >= 0.1)
        stride = max(1, c["T"] * c["K"] // 4096)
        arrays.update({f"c{n}_xq": xq, f"c{n}_w": r64["w"], f"c{n}_mu": r64["mu"], f"c{n}_sigma": r64["sigma"], f"c{n}_loglik": np.float64(r64["loglik"]),
                       f"c{n}_posterior": r64["posterior"][::stride]})
        arrays.update({f"c{n}_init_{q}": a.astype(np.float32) for q, a in zip(("w", "mu", "sigma"), init)})
        if ubm:
            arrays.update({f"c{n}_ubm_{q}": a.astype(np.float32) for q, a in zip(("w", "mu", "sigma"), ubm)})
        tlist = []
        params32 = tuple(f32(r64[q]) for q in ("w", "mu", "sigma"))   # the transform's model: the trained parameters, as float32 values
        diag = gmm_ref.is_diag(c["var_type"], c["block_size"])
        for j, Lx in enumerate(c["transforms"]):
            _, _, _, gap = gmm_ref.transform(x[:, :Lx], *params32, diag)
            xt = x[gap > 1e-2][:200, :Lx]
            assert len(xt) >= 20, (c, Lx, len(xt))
            my, midx, mlp, gap = gmm_ref.transform(xt, *params32, diag)
            y64, i64, l64 = run_transform(diffsptk, c, torch.float64, params32, xt)
            y32, i32, l32 = run_transform(diffsptk, c, torch.float32, params32, xt)
            assert np.array_equal(i64, i32) and np.array_equal(i64, midx) and gap.min() > 1e-2, (c, Lx)
            for a, b in ((my, y64), (mlp, l64)):
                if b is not None:
                    dev = deviation(a, b)
                    worst = max(worst, (dev, (n, f"t{j}")))
                    assert dev <= 1e-10, (c, Lx, dev)
            post, _, numer = gmm_ref.e_step(xt, *params32, diag, Lx)
            arrays.update({f"c{n}_t{j}_x": xt.astype(np.float32), f"c{n}_t{j}_indices": i64.astype(np.int64), f"c{n}_t{j}_log_prob": l64})
            if y64 is not None:
                arrays[f"c{n}_t{j}_y"] = y64
            tlist.append(dict(Lx=Lx, nmax=float(np.abs(numer).max()), e_y=0.0 if y64 is None else float(np.abs(y32 - y64).max()),
                              e_log_prob=float(np.abs(l32 - l64).max())))
        rec = dict(c, eps=eps, seed=seed, n_run=r64["n_run"], e_ref=e_ref, nmax=mine["nmax"], overlap=overlap, post_stride=stride, transforms=tlist)
        listed.append(rec)
        print(n, {k: v for k, v in rec.items() if k not in ("e_ref", "transforms")}, "E_ref", e_ref, "margin", margin, flush=True)
    assert sum(r["overlap"] for r in listed) * 2 >= len(listed), [r["overlap"] for r in listed]
    np.savez_compressed(os.path.join(HERE, "gmm.npz"), **arrays)

    cls = diffsptk.GaussianMixtureModeling
    plain, ubm = cls(2, 3), cls(2, 3, ubm=(torch.ones(3) / 3, torch.zeros(3, 3), torch.eye(3).repeat(3, 1, 1)), alpha=0.5)
    api = {
        "signatures": {name: signature(getattr(cls, name)) for name in ("__init__", "forward", "set_params", "warmup", "transform", "_e_step")},
        "alias": diffsptk.GMM is cls,
        "in_root": [hasattr(diffsptk, name) for name in ("GaussianMixtureModeling", "GMM")],
        "functional": [name for name in dir(diffsptk.functional) if "gmm" in name.lower()],
        "state_dict": {"plain": {k: list(v.shape) for k, v in plain.state_dict().items()}, "ubm": {k: list(v.shape) for k, v in ubm.state_dict().items()}},
        "buffers": {"plain": sorted(k for k, _ in plain.named_buffers()), "ubm": sorted(k for k, _ in ubm.named_buffers())},
        "errors": {name: raised(f, diffsptk) for name, f in gmm_ref.ERRORS.items()},
        "restatement_deviation": worst[0],
        "cases": listed,
    }
    assert all(r[0] != "ok" for r in api["errors"].values()), api["errors"]
    with open(os.path.join(HERE, "gmm_api.json"), "w") as f:
        json.dump(api, f, indent=1)
        f.write("\n")
    print("wrote", len(listed), "cases;", os.path.getsize(os.path.join(HERE, "gmm.npz")), "bytes; restatement deviation", worst)


if __name__ == "__main__":
    main()
