"""Gaussian mixture models (csrc/gmm.hip): the E-step, the EM loop on the device with one small host read per iteration, and the
conversion of a joint-density model."""
from __future__ import annotations

import torch

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream


def gmm_lds_bytes(L: int, size: int) -> int:
    """what the E-step's workgroup holds in LDS (include/diffsptk_amd.h, section a21): a tile of vectors and of their differences from a
    mean (2 DSA_GMM_TILE_BYTES bytes per column, one column of padding), one component's matrix and mean, the reduction scratch"""
    return 2 * _lib.GMM_TILE_BYTES * (L + 1) + L * (L + 1) * size + 64


def _check_gmm(x, w, mu, sigma, Lp=None):
    """x:(T, L') against w:(K), mu:(K, L), sigma:(K, L, L); L' = L unless Lp names the leading block.  The ceiling first, the device last."""
    K, L = mu.shape
    Lp = L if Lp is None else Lp
    if x.dim() != 2 or x.size(1) != Lp or not 1 <= Lp <= L:
        raise ValueError(f"gmm: x must be (T, {Lp}), got {tuple(x.shape)}")
    if x.size(0) < 1:
        raise ValueError("gmm: x must not be empty")
    if tuple(w.shape) != (K,) or tuple(sigma.shape) != (K, L, L):
        raise ValueError(f"gmm: w, mu, sigma must be (K,), (K, L), (K, L, L), got {tuple(w.shape)}, {tuple(mu.shape)}, {tuple(sigma.shape)}")
    need = gmm_lds_bytes(Lp, x.element_size())
    if need > _lib.GMM_MAX_LDS_BYTES:
        raise ValueError(f"gmm: vectors of {Lp} elements take {need} bytes: a tile of vectors, their differences and one component's "
                         f"matrix must fit DSA_GMM_MAX_LDS_BYTES = {_lib.GMM_MAX_LDS_BYTES} bytes of LDS")
    _same_dtype(w, x, mu, sigma)
    _dtype_code(x)
    _require_device(x, w, mu, sigma)


def gmm_estep(x, w, mu, sigma, diag, Lp=None, readback=None):
    """(posterior:(T, K), loglik:(T), total:()) of gmm.py:434-486 on the leading (Lp, Lp) block.  readback: a (2,) float64 device tensor
    that receives the total and the first component + 1 whose covariance is not positive definite (0: none).  No host read."""
    _check_gmm(x, w, mu, sigma, Lp)
    xc, wc, mc, sc = x.contiguous(), w.contiguous(), mu.contiguous(), sigma.contiguous()
    K, L = mc.shape
    T, Lp = xc.shape
    dev, dt = xc.device, xc.dtype
    prec = torch.empty(K, Lp if diag else Lp * Lp, device=dev, dtype=dt)
    cst = torch.empty(K, device=dev, dtype=dt)
    failed = torch.empty(K, device=dev, dtype=torch.int32)
    post = torch.empty(T, K, device=dev, dtype=dt)
    ll = torch.empty(T, device=dev, dtype=dt)
    rows = _lib.GMM_TILE_BYTES // xc.element_size()
    partial = torch.empty((T + rows - 1) // rows, device=dev, dtype=torch.float64)
    total = torch.empty((), device=dev, dtype=dt)
    with torch.cuda.device(dev):
        _call("dsa_gmm_prepare", _p(wc), _p(sc), K, L, Lp, int(diag), _dtype_code(xc), _p(prec), _p(cst), _p(failed), _stream())
        _call("dsa_gmm_estep", _p(xc), _p(mc), _p(prec), _p(cst), _p(failed), T, K, L, Lp, int(diag), _dtype_code(xc), _p(post), _p(ll), _p(partial),
              _p(total), _p(readback), _stream())
    return post, ll, total


def gmm_em_step(x, w, mu, sigma, mask, ubm, diag, alpha, weight_floor, var_floor, readback):
    """One EM iteration in place on w, mu, sigma (contiguous): five launches, no host read.  readback as in gmm_estep; when it reports a
    failed factorisation the parameters are left as they were.  Returns the log-likelihood of the E-step, a 0-d tensor."""
    post, _, total = gmm_estep(x, w, mu, sigma, diag, None, readback)
    K, L = mu.shape
    T = x.size(0)
    code = _dtype_code(x)
    ubm_w, ubm_mu, ubm_sigma = ubm if ubm is not None else (None, None, None)
    with torch.cuda.device(x.device):
        size = _lib.load().dsa_gmm_accum_workspace_bytes(T, K, L, int(diag), code)
        if size < 0:
            _lib.check(_lib.ERR_INVALID_ARGUMENT, "dsa_gmm_accum_workspace_bytes")
        ws = torch.empty(size // x.element_size(), device=x.device, dtype=x.dtype)
        _call("dsa_gmm_accum", _p(x), _p(post), T, K, L, int(diag), code, _p(ws), _stream())
        _call("dsa_gmm_update", _p(ws), _p(readback), _p(ubm_w), _p(ubm_mu), _p(ubm_sigma), _p(mask), T, K, L, int(diag), float(alpha),
              float(weight_floor), float(var_floor), code, _p(w), _p(mu), _p(sigma), _stream())
    return total


def gmm_cluster_moments(x, indices, K):
    """(count:(K), kxx:(K, L, L)) of a hard assignment indices:(T) in 0 .. K - 1: the number of vectors of every cluster and the sum of
    their x x^T (gmm.py:222-233), by dsa_gmm_accum on the one-hot posterior -- K times the work of a direct sum, for a one-off
    initialisation.  No host read."""
    if x.dim() != 2 or x.size(0) < 1 or tuple(indices.shape) != (x.size(0),):
        raise ValueError(f"gmm: x must be (T, L) and indices (T,), got {tuple(x.shape)} and {tuple(indices.shape)}")
    code = _dtype_code(x)
    _require_device(x, indices)
    xc = x.contiguous()
    T, L = xc.shape
    post = torch.zeros(T, K, device=xc.device, dtype=xc.dtype).scatter_(1, indices.view(-1, 1), 1)
    with torch.cuda.device(xc.device):
        size = _lib.load().dsa_gmm_accum_workspace_bytes(T, K, L, 0, code)
        if size < 0:
            _lib.check(_lib.ERR_INVALID_ARGUMENT, "dsa_gmm_accum_workspace_bytes")
        ws = torch.zeros(size // xc.element_size(), device=xc.device, dtype=xc.dtype)   # (the tiles above the diagonal stay unwritten)
        _call("dsa_gmm_accum", _p(xc), _p(post), T, K, L, 0, code, _p(ws), _stream())
    low = torch.tril(ws.view(-1, K, L + 1, L + 1).sum(0))   # the lower triangle of sum [x, 1] [x, 1]^T per cluster
    full = low + torch.tril(low, -1).transpose(-1, -2)
    count = torch.bincount(indices, minlength=K).to(xc.dtype)
    return count, full[:, :L, :L]


def gmm_transform(x, post, mu, sigma, Lx):
    """(y:(T, L - Lx) or None, indices:(T) int64): gmm.py:418-432 from the posterior of the leading block.  No host read."""
    xc, pc, mc, sc = x.contiguous(), post.contiguous(), mu.contiguous(), sigma.contiguous()
    K, L = mc.shape
    T = xc.size(0)
    code = _dtype_code(xc)
    indices = torch.empty(T, device=xc.device, dtype=torch.int64)
    y = M = None
    with torch.cuda.device(xc.device):
        if Lx < L:
            M = torch.empty(K, L - Lx, Lx, device=xc.device, dtype=xc.dtype)
            y = torch.empty(T, L - Lx, device=xc.device, dtype=xc.dtype)
            _call("dsa_gmm_regress", _p(sc), K, L, Lx, code, _p(M), _stream())
        _call("dsa_gmm_transform", _p(xc), _p(pc), _p(mc), _p(M), T, K, L, Lx, code, _p(indices), _p(y), _stream())
    return y, indices
