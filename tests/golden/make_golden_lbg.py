#!/usr/bin/env python3
"""Golden fixtures of LindeBuzoGrayAlgorithm and of GaussianMixtureModeling.warmup, by importing the REFERENCE.  Build container only
(CPU; a few minutes).

    python tests/golden/make_golden_lbg.py     # writes tests/golden/lbg.npz and lbg_api.json (data)

The reference's VectorQuantization imports the package vector_quantize_pytorch, which is not installed.  A stand-in written here takes
its place (as make_golden.import_reference() stands empty modules in for torchaudio and soundfile): VectorQuantize(dim, codebook_size)
with a float32 `codebook` buffer drawn by torch.randn, and forward(x) -> (codebook[idx], idx, zeros(1)), idx the first argmin of the
float64 squared distances.  The reference's LBG and GMM.warmup then run unchanged.  torch.randn is wrapped while they run, so every
draw is recorded; the tests hand the recorded draws to the module under test through its `_randn`.

Inputs that make the comparison exact: x is a multiple of 2^-8 with |x| < 8 and T <= 4096, stored as int16.  Every float32 partial sum
of the reference's scatter_add_ and sum(0) is then exact in any order (below 2^23 units of 2^-8), and a float64 quotient rounded to
float32 equals the float32 quotient (53 >= 2 * 24 + 2).  So a codebook made of float64 sums, divided and rounded once, is the
reference's bit for bit at every iteration, provided every assignment agrees -- which the first condition below secures.

Conditions, asserted here for EVERY case (the case's seed is advanced until they hold; nothing is filtered at test time):
  * at every E-step and for every vector the two nearest codewords differ by (d2 - d1) / d2 >= 2^-40, about a hundred times the
    (L + 2) 2^-53 a float64 sum of L <= 64 squares can lose;
  * the reference and the restatement tests/lbg_ref.py run the same number of iterations at every codebook size, and give the same
    codebook (bits), indices and n_data;
  * at every convergence test |ratio - eps|, ratio = change / (d + 1e-16), exceeds 8 times the larger of the reference's own error of
    that ratio (its value against the restatement's) and 2^-22, what rounding two distances to float32 can move it by;
  * a `repair` case has 1 or 2 clusters below min_data_per_cluster in some iteration and never more (r.mean(0) of one or two rows
    does not depend on the order of summation); every other case has none.  Repair cases are float32: with float64 input the
    reference repairs in float64 before rounding, the modules after;
  * `stops` "eps": every codebook size stops before n_iter; "n_iter": every size runs all n_iter iterations.

Per case c<n>: xq (int16), start (the codebook as the constructor left it, init rows included), init (if given), draw<i>, codebook,
indices, n_data; for a warmup case w, mu, sigma of the float64 model.  The JSON holds the options, per size the iteration count and the
reference's distance of every iteration, E_ref = max |reference's distance - restatement's| (for warmup cases also E_ref of w, mu,
sigma: float32 model against float64 model), the smallest gap and margin, and `restatement_deviation`, the largest |restatement's
distance - reference's| relative to max(1, d) over the float64 cases."""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402

import lbg_ref  # noqa: E402

EPOCHS = []   # one entry per call of the stand-in: (rows, live codewords, sum of squares in float32, in float64)


class VectorQuantize(torch.nn.Module):
    def __init__(self, dim, codebook_size):
        super().__init__()
        self.register_buffer("codebook", torch.randn(codebook_size, dim))

    def forward(self, x):
        cb = self.codebook
        d = (x.double().unsqueeze(1) - cb.double().unsqueeze(0)).square().sum(-1)
        idx = d.argmin(1)
        xq = cb[idx]
        EPOCHS.append((len(x), int((cb[:, 0] != 1e10).sum()), float((x - xq).square().sum()), float((x.double() - xq.double()).square().sum())))
        return xq, idx, torch.zeros(1)


def import_with_stand_in():
    stand_in = types.ModuleType("vector_quantize_pytorch")
    stand_in.VectorQuantize = VectorQuantize
    sys.modules["vector_quantize_pytorch"] = stand_in
    return import_reference()


class Recorder:
    """torch.randn, with every draw kept"""

    def __enter__(self):
        self.draws, self.inner = [], torch.randn

        def randn(*args, **kwargs):
            out = self.inner(*args, **kwargs)
            self.draws.append(out.detach().clone())
            return out

        torch.randn = randn
        return self

    def __exit__(self, *exc):
        torch.randn = self.inner


def case(L, K, T, dtype="f32", n_iter=20, eps=1e-5, perturb_factor=1e-5, min_data=1, init_rows=0, repair=False, stops=None, batch_size=None,
         warmup=None, spread=3.0):
    return dict(L=L, K=K, T=T, dtype=dtype, n_iter=n_iter, eps=eps, perturb_factor=perturb_factor, min_data=min_data, init_rows=init_rows,
                repair=repair, stops=stops, batch_size=batch_size, warmup=warmup, spread=spread)


def cases():
    return [
        case(1, 1, 10),                                         # K = 1: no split
        case(2, 2, 10),                                         # the shape of the reference's docstring example
        case(3, 4, 64, "f64"),
        case(5, 8, 257),
        case(5, 8, 65),                                         # T a few times K
        case(25, 16, 4000),
        case(25, 64, 4096),                                     # the largest
        case(3, 4, 64, init_rows=1),
        case(3, 4, 64, "f64", init_rows=2),
        case(4, 6, 200, init_rows=3),
        case(4, 12, 300, "f64", init_rows=3),
        case(5, 8, 65, min_data=5, repair=True),
        case(3, 4, 64, min_data=12, repair=True, perturb_factor=1e-2),
        case(5, 8, 257, n_iter=100, eps=1e-3, stops="eps"),
        case(5, 8, 257, "f64", n_iter=3, eps=0.0, stops="n_iter"),
        case(3, 4, 64, perturb_factor=1e-2),
        case(5, 8, 257, batch_size=100),                        # a DataLoader whose batch size does not divide T
        case(3, 4, 300, warmup=dict(var_type="diag", block_size=None)),
        case(4, 4, 400, warmup=dict(var_type="full", block_size=None)),
    ]


def inputs(c, seed):
    rng = np.random.default_rng(seed)
    L, K, T = c["L"], c["K"], c["T"]
    centres = rng.normal(size=(K, L)) * c["spread"] / np.sqrt(L)
    weights = rng.uniform(0.3, 1.0, K) if not c["repair"] else np.concatenate([np.full(K - 2, 1.0), [0.08, 0.08]])
    members = rng.choice(K, size=T, p=weights / weights.sum())
    x = centres[members] + rng.normal(size=(T, L)) * 0.5
    xq = np.clip(np.round(x * 256.0), -2047, 2047).astype(np.int16)
    init = None
    if c["init_rows"]:
        init = (centres[:c["init_rows"]] + 0.1 * rng.normal(size=(c["init_rows"], L))).astype(np.float32)
    return xq, init


def epochs_to_distances(epochs, T, dtype):
    """the reference's e_step over the stand-in's calls: per pass over the data (live codewords, distance in the reference's precision)"""
    out, rows, s32, s64 = [], 0, np.float32(0), 0.0
    for n, live, a32, a64 in epochs:
        rows, s32, s64 = rows + n, np.float32(s32 + np.float32(a32)), s64 + a64
        if rows == T:
            out.append((live, float(np.float32(s32 / np.float32(T))) if dtype == "f32" else s64 / T))
            rows, s32, s64 = 0, np.float32(0), 0.0
    assert rows == 0
    return out


def run_lbg(diffsptk, c, x, init):
    """the reference on x (float64 values): dict(start, draws, codebook, indices, distance, passes [(live, distance)])"""
    dtype = torch.float32 if c["dtype"] == "f32" else torch.float64
    xt = torch.tensor(x, dtype=dtype)
    lbg = diffsptk.LBG(c["L"] - 1, c["K"], min_data_per_cluster=c["min_data"], n_iter=c["n_iter"], eps=c["eps"], perturb_factor=c["perturb_factor"],
                       init="mean" if init is None else torch.tensor(init), batch_size=c["batch_size"])
    start = lbg.vq.codebook.clone().numpy()
    curr = lbg.curr_codebook_size
    data = xt if c["batch_size"] is None else torch.utils.data.DataLoader(torch.utils.data.TensorDataset(xt), batch_size=c["batch_size"])
    EPOCHS.clear()
    with Recorder() as rec:
        codebook, indices, distance = lbg(data, return_indices=True)
    passes = epochs_to_distances(list(EPOCHS), c["T"], c["dtype"])
    if init is None:
        passes = passes   # (the mean initialisation does not call the quantiser)
    return dict(start=start, curr=curr, draws=[d.numpy().astype(np.float32) for d in rec.draws], codebook=codebook.numpy().copy(),
                indices=indices.numpy().copy(), distance=float(distance), passes=passes[:-1])   # the last pass: return_indices


def run_warmup(diffsptk, c, x, dtype):
    gmm = diffsptk.GMM(c["L"] - 1, c["K"], dtype=dtype, **c["warmup"])
    torch.manual_seed(c["L"] * 1000 + c["T"])   # the same draws for the float64 and the float32 model
    EPOCHS.clear()
    with Recorder() as rec:
        gmm.warmup(torch.tensor(x, dtype=dtype), n_iter=c["n_iter"], eps=c["eps"], perturb_factor=c["perturb_factor"])
    return dict(w=gmm.w.double().numpy().copy(), mu=gmm.mu.double().numpy().copy(), sigma=gmm.sigma.double().numpy().copy(),
                draws=[d.numpy().astype(np.float32) for d in rec.draws])


def judge(c, ref, mine):
    """(ok, record) of one seed: the conditions of the docstring"""
    by_size = {}
    for live, d in ref["passes"]:
        by_size.setdefault(live, []).append(d)
    same = list(by_size) == mine["sizes"] and [len(v) for v in by_size.values()] == [len(v) for v in mine["distances"]]
    if not same:
        return False, dict(why="iterations differ")
    if not (np.array_equal(ref["codebook"].view(np.int32), mine["codebook"].view(np.int32)) and np.array_equal(ref["indices"], mine["indices"])):
        return False, dict(why="codebook or indices differ")
    if not mine["gap"] >= 2.0 ** -40:
        return False, dict(why=f"gap {mine['gap']}")
    real = np.float32 if c["dtype"] == "f32" else np.float64
    e_ref, margin, prev = 0.0, np.inf, None
    for (size, ref_d), my_d in zip(by_size.items(), mine["distances"]):
        for n, (a, b) in enumerate(zip(ref_d, my_d)):
            e_ref = max(e_ref, abs(a - b))
            if n:
                ratio_ref = float(np.abs(real(prev[0]) - real(a)) / (real(a) + real(1e-16)))
                ratio_mine = abs(prev[1] - b) / (b + 1e-16)
                margin = min(margin, abs(ratio_mine - c["eps"]) - 8 * max(abs(ratio_ref - ratio_mine), 2.0 ** -22))
            prev = (a, b)
    if c["eps"] > 0 and not margin > 0:
        return False, dict(why=f"margin {margin}")
    smalls = [s for per in mine["n_small"] for s in per]
    if c["repair"]:
        if not (max(smalls) in (1, 2)):
            return False, dict(why=f"clusters below the minimum: {sorted(set(smalls))}")
    elif any(smalls):
        return False, dict(why="a cluster below the minimum")
    counts = [len(v) for v in mine["distances"]]
    if c["stops"] == "eps" and not all(n < c["n_iter"] for n in counts):
        return False, dict(why=f"not stopped by eps: {counts}")
    if c["stops"] == "n_iter" and not all(n == c["n_iter"] for n in counts):
        return False, dict(why=f"stopped early: {counts}")
    return True, dict(sizes=mine["sizes"], iterations=counts, distances=list(by_size.values()), e_ref=e_ref, gap=mine["gap"],
                      margin=None if not np.isfinite(margin) else margin, n_small=mine["n_small"], distance=ref["distance"])


def signature(f):
    return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]


def raised(f, m):
    try:
        f(m)
        return ["ok", ""]
    except Exception as e:   # noqa: BLE001
        return [type(e).__name__, str(e)]


def main():
    diffsptk = import_with_stand_in()
    arrays, listed, worst = {}, [], 0.0
    for n, c in enumerate(cases()):
        seed = 1000 * n
        while True:
            assert seed < 1000 * n + 300, ("no seed meets the conditions", c)
            torch.manual_seed(seed)
            xq, init = inputs(c, seed)
            x = xq.astype(np.float64) / 256.0
            extra = {}
            if c["warmup"]:
                w64, w32 = run_warmup(diffsptk, c, x, torch.float64), run_warmup(diffsptk, c, x, torch.float32)
                assert all(np.array_equal(a, b) for a, b in zip(w64["draws"], w32["draws"]))
                start, draws = w64["draws"][0], w64["draws"][1:]   # the first draw is the constructor's codebook
                mine = lbg_ref.design(x, start, c["K"], 1, draws, min_data=c["min_data"], n_iter=c["n_iter"], eps=c["eps"],
                                      perturb_factor=c["perturb_factor"], dtype="f64")
                mask = lbg_ref.make_mask(c["L"], c["warmup"]["var_type"], c["warmup"]["block_size"])
                w, mu, sigma = lbg_ref.warmup(x, mine["codebook"], mine["indices"], mask)
                smalls = [s for per in mine["n_small"] for s in per]
                ok = (np.array_equal(w, w64["w"]) and np.array_equal(mu, w64["mu"]) and np.array_equal(w64["mu"], w32["mu"])
                      and np.array_equal(w64["w"].astype(np.float32), w32["w"].astype(np.float32)) and mine["gap"] >= 2.0 ** -40 and not any(smalls)
                      and mine["n_data"].min() >= 2)
                rec = dict(sizes=mine["sizes"], iterations=[len(v) for v in mine["distances"]], distances=mine["distances"], e_ref=0.0,
                           gap=mine["gap"], margin=None, n_small=mine["n_small"], distance=mine["distance"],
                           e_ref_w=float(np.abs(w32["w"] - w64["w"]).max()), e_ref_mu=float(np.abs(w32["mu"] - w64["mu"]).max()),
                           e_ref_sigma=float(np.abs(w32["sigma"] - w64["sigma"]).max()),
                           sigma_deviation=float(np.abs(sigma - w64["sigma"]).max())) if ok else dict(why="warmup differs")
                ref = dict(start=start, curr=1, draws=draws, codebook=mine["codebook"], indices=mine["indices"])
                extra = {q: w64[q] for q in ("w", "mu", "sigma")}
            else:
                ref = run_lbg(diffsptk, c, x, init)
                mine = lbg_ref.design(x, ref["start"], c["K"], ref["curr"], ref["draws"], init="mean" if init is None else "none",
                                      min_data=c["min_data"], n_iter=c["n_iter"], eps=c["eps"], perturb_factor=c["perturb_factor"], dtype=c["dtype"])
                ok, rec = judge(c, ref, mine)
            if ok:
                break
            print(n, "seed", seed, rec["why"], flush=True)
            seed += 1
        if c["dtype"] == "f64" and not c["warmup"]:
            worst = max(worst, max(abs(a - b) / max(1.0, b) for ra, rb in zip(rec["distances"], mine["distances"]) for a, b in zip(ra, rb)))
        arrays.update({f"c{n}_xq": xq, f"c{n}_start": ref["start"].astype(np.float32), f"c{n}_codebook": ref["codebook"].astype(np.float32),
                       f"c{n}_indices": ref["indices"].astype(np.int16 if c["K"] < 2 ** 15 else np.int64), f"c{n}_n_data": mine["n_data"].astype(np.int64)})
        arrays.update({f"c{n}_draw{i}": d for i, d in enumerate(ref["draws"])})
        arrays.update({f"c{n}_{q}": a for q, a in extra.items()})
        if init is not None:
            arrays[f"c{n}_init"] = init
        listed.append(dict(c, seed=seed, curr=int(ref["curr"]), n_draws=len(ref["draws"]), **rec))
        print(n, {k: v for k, v in listed[-1].items() if k not in ("distances", "n_small")}, flush=True)
    np.savez_compressed(os.path.join(HERE, "lbg.npz"), **arrays)

    vq, ivq, lbg = diffsptk.VectorQuantization, diffsptk.InverseVectorQuantization, diffsptk.LindeBuzoGrayAlgorithm
    api = {
        "signatures": {"VectorQuantization": {name: signature(getattr(vq, name)) for name in ("__init__", "forward")},
                       "InverseVectorQuantization": {name: signature(getattr(ivq, name)) for name in ("__init__", "forward")},
                       "LindeBuzoGrayAlgorithm": {name: signature(getattr(lbg, name)) for name in ("__init__", "forward", "transform")}},
        "alias": diffsptk.LBG is lbg,
        "in_root": [hasattr(diffsptk, name) for name in ("VectorQuantization", "InverseVectorQuantization", "LindeBuzoGrayAlgorithm", "LBG")],
        "codebook": {"shape": list(vq(2, 5).codebook.shape), "dtype": str(vq(2, 5).codebook.dtype)},
        "lbg_buffers": sorted(k for k, _ in lbg(2, 4).named_buffers()),
        "errors": {name: raised(f, diffsptk) for name, f in lbg_ref.ERRORS.items()},
        "restatement_deviation": worst,
        "cases": listed,
    }
    assert all(r[0] != "ok" for r in api["errors"].values()), api["errors"]
    with open(os.path.join(HERE, "lbg_api.json"), "w") as f:
        json.dump(api, f, indent=1)
        f.write("\n")
    print("wrote", len(listed), "cases;", os.path.getsize(os.path.join(HERE, "lbg.npz")), "bytes; restatement deviation", worst)


if __name__ == "__main__":
    main()
