"""GaussianMixtureModeling in NumPy float64, written from the formulas of EM for Gaussian mixtures (Dempster et al.; MAP adaptation:
Gauvain & Lee 1994) with the reference's conventions: the weight floor with its affine renormalisation, the variance floor, the
covariance mask, the stop on the change of the total log-likelihood.  tests/test_gmm_cpu.py pins it to the goldens of the reference
(tests/golden/gmm.npz, make_golden_gmm.py); the GPU tests lean on it where no golden exists.  Also the goldens' loader, the bounds
of the GPU tests, and the option errors the API test compares."""
import json
import os

import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))
QUANTITIES = ("w", "mu", "sigma", "posterior", "loglik")


def make_mask(L, var_type, block_size):
    """full blocks on the diagonal, or for "diag" the diagonals of every pair of blocks of equal size"""
    block_size = [L] if block_size is None else list(block_size)
    edges = np.cumsum([0] + block_size)
    mask = np.zeros((L, L))
    for b1, s1 in zip(block_size, edges):
        for b2, s2 in zip(block_size, edges):
            if var_type == "full" and s1 == s2:
                mask[s1:s1 + b1, s1:s1 + b1] = 1.0
            if var_type == "diag" and b1 == b2:
                mask[s1:s1 + b1, s2:s2 + b2] = np.eye(b1)
    return mask


def is_diag(var_type, block_size):
    return var_type == "diag" and (block_size is None or len(block_size) == 1)


def e_step(x, w, mu, sigma, diag, Lp=None):
    """(posterior (T, K), log-likelihood per vector (T), numer (T, K)) on the leading (Lp, Lp) block"""
    Lp = x.shape[1] if Lp is None else Lp
    K = len(w)
    numer = np.empty((len(x), K))
    for k in range(K):
        d = x[:, :Lp] - mu[k, :Lp]
        S = sigma[k, :Lp, :Lp]
        if diag:
            v = np.diagonal(S)
            logdet, maha = np.log(v).sum(), (d * d / v).sum(1)
        else:
            C = np.linalg.cholesky(S)
            u = np.linalg.solve(C, d.T)
            logdet, maha = 2.0 * np.log(np.diagonal(C)).sum(), (u * u).sum(0)
        numer[:, k] = np.log(w[k]) - 0.5 * (Lp * LOG_2PI + logdet + maha)
    top = numer.max(1, keepdims=True)
    lse = top + np.log(np.exp(numer - top).sum(1, keepdims=True))
    return np.exp(numer - lse), lse[:, 0], numer


def m_step(x, post, w, mu, sigma, *, diag, mask, weight_floor, var_floor, ubm, alpha):
    T, L = x.shape
    K = post.shape[1]
    y = post.sum(0)
    px = post.T @ x
    xi = alpha * ubm[0] if alpha else np.zeros(K)
    z = y + xi
    neww = np.maximum(z / (T + alpha), weight_floor)
    a = (1.0 - weight_floor * K) / (neww.sum() - weight_floor * K)
    neww = a * neww + weight_floor * (1.0 - a)
    newmu = (px + xi[:, None] * ubm[1]) / z[:, None] if alpha else px / z[:, None]
    newsigma = sigma.copy()
    for k in range(K):
        pxx = (x * post[:, k:k + 1]).T @ x
        mm = np.outer(newmu[k], newmu[k])
        if alpha:
            with np.errstate(all="ignore"):
                nu = px[k] / y[k]
                data = np.nan_to_num(pxx - y[k] * (np.outer(nu, newmu[k]) + np.outer(newmu[k], nu) - mm), nan=0.0, posinf=0.0, neginf=0.0)
            dm = ubm[1][k] - newmu[k]
            S = (data + xi[k] * ubm[2][k] + xi[k] * np.outer(dm, dm)) / z[k]
        else:
            S = pxx / z[k] - mm
        if diag:
            newsigma[k][np.diag_indices(L)] = np.maximum(np.diagonal(S), var_floor)
        else:
            S = S * mask
            S[np.diag_indices(L)] = np.maximum(np.diagonal(S), var_floor)
            newsigma[k] = S
    return neww, newmu, newsigma


def train(x, w, mu, sigma, *, n_iter, eps=1e-5, weight_floor=1e-5, var_floor=1e-6, var_type="diag", block_size=None, ubm=None, alpha=0.0):
    """dict(w, mu, sigma, loglik, posterior, n_run, changes, mass, raw_w): the parameters after the loop of gmm.py:299-386, the total
    log-likelihood of the E-step before the last update, the posterior under the final parameters, the iterations run, the change of
    every iteration, the smallest posterior mass any component had, the smallest unfloored weight"""
    L = x.shape[1]
    diag, mask = is_diag(var_type, block_size), make_mask(L, var_type, block_size)
    w, mu, sigma = w.copy(), mu.copy(), sigma.copy()
    prev, changes, mass, raw = -np.inf, [], np.inf, np.inf
    for n in range(n_iter):
        post, ll, _ = e_step(x, w, mu, sigma, diag)
        total = ll.sum()
        mass = min(mass, post.sum(0).min())
        raw = min(raw, ((post.sum(0) + (alpha * ubm[0] if alpha else 0.0)) / (len(x) + alpha)).min())
        w, mu, sigma = m_step(x, post, w, mu, sigma, diag=diag, mask=mask, weight_floor=weight_floor, var_floor=var_floor, ubm=ubm, alpha=alpha)
        changes.append(total - prev)
        if n and total - prev < eps:
            break
        prev = total
    post, _, numer = e_step(x, w, mu, sigma, diag)
    return dict(w=w, mu=mu, sigma=sigma, loglik=total, posterior=post, n_run=n + 1, changes=changes, mass=mass, raw_w=raw,
                nmax=float(np.abs(numer).max()))


def transform(x, w, mu, sigma, diag):
    """(y (T, L - Lx) or None, indices (T), log_prob (T), gap (T): the winning posterior less the runner-up, 1 for K = 1)"""
    Lx, L = x.shape[1], mu.shape[1]
    post, ll, _ = e_step(x, w, mu, sigma, diag, Lx)
    idx = post.argmax(1)
    part = np.sort(post, 1)
    gap = part[:, -1] - part[:, -2] if post.shape[1] > 1 else np.ones(len(x))
    if Lx == L:
        return None, idx, ll, gap
    M = np.stack([S[Lx:, :Lx] @ np.linalg.inv(S[:Lx, :Lx]) for S in sigma])
    y = mu[idx, Lx:] + np.einsum("tij,tj->ti", M[idx], x - mu[idx, :Lx])
    return y, idx, ll, gap


# ------------------------------------------------------------------ the goldens
def golden_cases(golden_dir):
    api = json.load(open(os.path.join(golden_dir, "gmm_api.json")))
    z = np.load(os.path.join(golden_dir, "gmm.npz"))
    out = []
    for n, c in enumerate(api["cases"]):
        c = dict(c, n=n)
        for key in z.files:
            tag, _, name = key.partition("_")
            if tag == f"c{n}":
                c[name] = z[key]
        c["x"] = c.pop("xq").astype(np.float64) / 256.0   # multiples of 2^-8 below 128: exact in float32
        c["init"] = tuple(c.pop(f"init_{q}").astype(np.float64) for q in ("w", "mu", "sigma"))
        c["ubm"] = tuple(c.pop(f"ubm_{q}").astype(np.float64) for q in ("w", "mu", "sigma")) if c["alpha"] else None
        out.append(c)
    return out


def case_id(c):
    blocks = "x".join(map(str, c["block_size"])) if c["block_size"] else "one"
    return f"{c['n']}-{c['var_type']}-{blocks}-L{c['L']}-K{c['K']}-T{c['T']}-it{c['n_iter']}" + (f"-map{c['alpha']}" if c["alpha"] else "")


def options(c):
    return dict(n_iter=c["n_iter"], eps=c["eps"], weight_floor=c["weight_floor"], var_floor=c["var_floor"], var_type=c["var_type"],
                block_size=c["block_size"], alpha=c["alpha"])


def roundings(c, Lp=None):
    """the products and sums behind one numer[t, k]: the triangular product W d and the squares, or the weighted squares"""
    L = c["L"] if Lp is None else Lp
    return 3 * L + 4 if is_diag(c["var_type"], c["block_size"]) else L * (L + 3) // 2 + 4


def floor32(c):
    """The part of the float32 bound that does not come from the reference's own error (make_golden_gmm.py derives it): per iteration
    sqrt(T) roundings of a moment sum and sqrt(roundings) of a numer of size nmax, each 2^-24, relative to max(1, max |ref|)."""
    return 2.0 ** -24 * (np.sqrt(c["T"]) + np.sqrt(roundings(c)) * c["nmax"]) * c["n_run"]


def floor32_transform(c, t):
    return 2.0 ** -24 * (np.sqrt(roundings(c, t["Lx"])) * t["nmax"] + 8 * t["Lx"])


F64_BOUND = 16 * 1.3e-13   # 16 times the restatement's largest deviation from the goldens, measured by make_golden_gmm.py


# ------------------------------------------------------------------ the option errors, name -> what raises it (m: the package)
ERRORS = {
    "order": lambda m: m.GaussianMixtureModeling(-1, 2),
    "n_mixture": lambda m: m.GaussianMixtureModeling(1, 0),
    "n_iter": lambda m: m.GaussianMixtureModeling(1, 2, n_iter=0),
    "eps": lambda m: m.GaussianMixtureModeling(1, 2, eps=-1.0),
    "weight_floor": lambda m: m.GaussianMixtureModeling(1, 2, weight_floor=0.6),
    "weight_floor_negative": lambda m: m.GaussianMixtureModeling(1, 2, weight_floor=-0.1),
    "var_floor": lambda m: m.GaussianMixtureModeling(1, 2, var_floor=-1.0),
    "alpha": lambda m: m.GaussianMixtureModeling(1, 2, alpha=1.5),
    "alpha_without_ubm": lambda m: m.GaussianMixtureModeling(1, 2, alpha=0.5),
    "block_size_sum": lambda m: m.GaussianMixtureModeling(3, 2, block_size=[2, 1]),
    "block_size_positive": lambda m: m.GaussianMixtureModeling(3, 2, block_size=[5, -1]),
    "var_type": lambda m: m.GaussianMixtureModeling(1, 2, var_type="tied"),
    "order_before_n_mixture": lambda m: m.GaussianMixtureModeling(-1, 0, n_iter=0),
    "alpha_before_block_size": lambda m: m.GaussianMixtureModeling(3, 2, alpha=0.5, block_size=[1]),
    "block_size_before_var_type": lambda m: m.GaussianMixtureModeling(3, 2, var_type="tied", block_size=[1]),
}
