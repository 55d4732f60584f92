"""NumPy restatement of LindeBuzoGrayAlgorithm.forward and of what GaussianMixtureModeling.warmup derives from it, written from the
algorithm: codebook doubling by `codebook -+ r`, nearest codeword by float64 sums of squares (first index on a tie), convergence test
in x's precision before the M-step, centroids as float64 sums divided by the count and rounded to float32, repair of clusters below
the minimum from the first largest cluster.  Every random number is taken from `draws`, a list of float32 arrays in the order the
algorithm asks for them; the codebook and the split / repair steps are float32, as in the modules.  Also: the loader of
tests/golden/lbg.npz + lbg_api.json."""
import json

import numpy as np

F32 = np.float32


def nearest(x, codebook):
    """(indices, minimal squared distances, smallest relative gap (d2 - d1) / d2 over the vectors) in float64"""
    d = ((x[:, None, :].astype(np.float64) - codebook[None, :, :].astype(np.float64)) ** 2).sum(-1)
    idx = d.argmin(1)
    best = d[np.arange(len(x)), idx]
    gap = np.inf
    if codebook.shape[0] > 1:
        rest = d.copy()
        rest[np.arange(len(x)), idx] = np.inf
        second = rest.min(1)
        gap = float(((second - best) / np.where(second > 0, second, 1.0)).min())
    return idx, best, gap


def centroids_of(x, idx, K, min_data):
    """(float32 centroids, zero where the count is below min_data; counts)"""
    counts = np.bincount(idx, minlength=K)
    sums = np.zeros((K, x.shape[1]))
    np.add.at(sums, idx, x.astype(np.float64))
    out = np.zeros((K, x.shape[1]), dtype=F32)
    keep = counts >= min_data
    out[keep] = (sums[keep] / counts[keep, None]).astype(F32)
    return out, counts


def design(x, start, K, curr, draws, *, init="mean", min_data=1, n_iter=100, eps=1e-5, perturb_factor=1e-5, dtype="f32"):
    """x:(T, L) float64 values, start:(K, L) float32 the codebook as the constructor left it (init rows included), curr: the number of
    rows the design starts from.  Returns dict(codebook float32, indices, distance, distances [[per iteration] per size], sizes, n_small
    [[...]], gap: the smallest relative gap of any E-step, ratios: [(size, iteration, ratio)] of every convergence test)."""
    real = F32 if dtype == "f32" else np.float64
    draws = list(draws)
    T, L = x.shape
    cb = np.array(start, dtype=F32)
    if init == "mean":
        cb[0] = (x.sum(0) / T).astype(F32)
    cb[curr:] = F32(1e10)
    pf = F32(perturb_factor)
    out = dict(distances=[], sizes=[], n_small=[], gap=np.inf, ratios=[])
    distance = real(np.inf)
    while True:
        if curr * 2 <= K:
            r = draws.pop(0).astype(F32).reshape(curr, L) * pf
            cb[curr:2 * curr] = cb[:curr] - r
            cb[:curr] = cb[:curr] + r
            curr *= 2
        prev = distance
        seen, smalls = [], []
        for n in range(n_iter):
            idx, best, gap = nearest(x, cb[:curr])
            out["gap"] = min(out["gap"], gap)
            d64 = float(best.sum() / T)
            distance = real(d64)
            seen.append(d64)
            with np.errstate(invalid="ignore"):
                change = np.abs(prev - distance)
                ratio = change / (distance + real(1e-16))
            if n:
                out["ratios"].append((curr, n, float(ratio)))
            if n and ratio < real(eps):
                break
            prev = distance
            cent, counts = centroids_of(x, idx, curr, min_data)
            small = counts < min_data
            smalls.append(int(small.sum()))
            if small.any():
                m = int(counts.argmax())
                r = draws.pop(0).astype(F32).reshape(int(small.sum()), L) * pf
                new = cent[m][None, :] - r
                cent[m] = cent[m] + r.sum(0, dtype=F32) / F32(len(r))
                cent[small] = new
            cb[:curr] = cent
        out["distances"].append(seen)
        out["sizes"].append(curr)
        out["n_small"].append(smalls)
        if curr == K:
            break
    assert not draws, f"{len(draws)} recorded draws were not used"
    idx, _, gap = nearest(x, cb)
    out["gap"] = min(out["gap"], gap)
    out.update(codebook=cb, indices=idx, distance=float(distance), n_data=np.bincount(idx, minlength=K))
    return out


def make_mask(L, var_type, block_size):
    block_size = block_size or [L]
    mask = np.zeros((L, L))
    edges = np.cumsum([0] + list(block_size))
    for b1, s1, e1 in zip(block_size, edges[:-1], edges[1:]):
        if var_type == "diag":
            for b2, s2, e2 in zip(block_size, edges[:-1], edges[1:]):
                if b1 == b2:
                    mask[s1:e1, s2:e2] = np.eye(b1)
        else:
            mask[s1:e1, s1:e1] = 1
    return mask


def warmup(x, codebook, indices, mask):
    """(w, mu, sigma) of gmm.py:222-238 in float64"""
    K = codebook.shape[0]
    count = np.bincount(indices, minlength=K).astype(np.float64)
    kxx = np.zeros((K, x.shape[1], x.shape[1]))
    np.add.at(kxx, indices, x[:, :, None] * x[:, None, :])
    mu = codebook.astype(np.float64)
    sigma = (kxx / count[:, None, None] - mu[:, :, None] * mu[:, None, :]) * mask
    return count / len(indices), mu, sigma


def options(c):
    return dict(min_data_per_cluster=c["min_data"], n_iter=c["n_iter"], eps=c["eps"], perturb_factor=c["perturb_factor"])


def golden_cases(directory):
    """every case of lbg_api.json with its arrays of lbg.npz: x (float64 values), start, draws (list), init (or None), codebook, indices,
    n_data, and for a warmup case w / mu / sigma of the float64 model"""
    with open(f"{directory}/lbg_api.json") as f:
        api = json.load(f)
    z = np.load(f"{directory}/lbg.npz")
    cases = []
    for n, c in enumerate(api["cases"]):
        c = dict(c, x=z[f"c{n}_xq"].astype(np.float64) / 256.0, start=z[f"c{n}_start"], draws=[z[f"c{n}_draw{i}"] for i in range(c["n_draws"])],
                 init=z[f"c{n}_init"] if f"c{n}_init" in z else None, codebook=z[f"c{n}_codebook"], indices=z[f"c{n}_indices"],
                 n_data=z[f"c{n}_n_data"])
        if c["warmup"]:
            c.update({q: z[f"c{n}_{q}"] for q in ("w", "mu", "sigma")})
        cases.append(c)
    return api, cases


def run_case(c):
    return design(c["x"], c["start"], c["K"], c["curr"], c["draws"], init="none" if c["init"] is not None else "mean",
                  min_data=c["min_data"], n_iter=c["n_iter"], eps=c["eps"], perturb_factor=c["perturb_factor"], dtype=c["dtype"])


# name -> callable(module) that must raise; the generator records what the reference raises, the tests compare
ERRORS = {
    "vq_order": lambda d: d.VectorQuantization(-1, 2),
    "vq_codebook_size": lambda d: d.VectorQuantization(1, 0),
    "lbg_order": lambda d: d.LindeBuzoGrayAlgorithm(-1, 2),
    "lbg_codebook_size": lambda d: d.LindeBuzoGrayAlgorithm(1, 0),
    "lbg_min_data_per_cluster": lambda d: d.LindeBuzoGrayAlgorithm(1, 2, min_data_per_cluster=0),
    "lbg_n_iter": lambda d: d.LindeBuzoGrayAlgorithm(1, 2, n_iter=0),
    "lbg_eps": lambda d: d.LindeBuzoGrayAlgorithm(1, 2, eps=-1.0),
    "lbg_perturb_factor": lambda d: d.LindeBuzoGrayAlgorithm(1, 2, perturb_factor=0.0),
    "lbg_init": lambda d: d.LindeBuzoGrayAlgorithm(1, 2, init="bogus")(__import__("torch").zeros(4, 2)),
    "lbg_2d": lambda d: d.LindeBuzoGrayAlgorithm(1, 2)(__import__("torch").zeros(4)),
    "lbg_init_size": lambda d: d.LindeBuzoGrayAlgorithm(1, 8, init=__import__("torch").zeros(3, 2)),
}
