"""Gaussian mixture models (reference: gmm.py): EM training of a K-component model on (T, L) vectors, diagonal, block-wise or full
covariance, optionally MAP-adapted from a universal background model, and the conversion of a joint-density model (`transform`).  One EM
iteration is five launches of csrc/gmm.hip -- factorisation, E-step, its total, weighted moment sums, M-step -- with the parameters,
the posterior and the moments on the device throughout; outer(x), the (B, K, L, 1) intermediates and the einsum of the reference never
exist.

What differs from the reference (include/diffsptk_amd.h, section a21):
  * the input is a (T, L) tensor of the module's dtype on the module's device, or a DataLoader whose batches are moved to the device and
    concatenated there ONCE; `batch_size` is accepted for parity and does not change the launches (a launch covers all T vectors);
  * `forward` reads two numbers back per iteration, in one copy: the log-likelihood, which the convergence test needs (the reference
    synchronises there too), and the status of the factorisation.  Because of that read `forward` cannot be captured in a graph;
    `transform` and `_e_step(reduction="none")` read nothing back;
  * a covariance that is not positive definite raises torch.linalg.LinAlgError from `forward`, naming the component, after the iteration's
    launches have finished (the M-step of that iteration is skipped on the device: the parameters stay as they were).  `transform` and
    `_e_step` do not read the status: there such a component has posterior 0 and, if every component fails, the result is NaN;
  * `transform` forms sigma_yx sigma_xx^-1 in a kernel of its own (Gauss-Jordan with partial pivoting on the block as it is), not with
    torch.inverse; a singular block gives inf / NaN instead of an error;
  * `warmup` still raises NotImplementedError; what it computes in the reference -- K-means clustering by LindeBuzoGrayAlgorithm, then
    weights, means and covariances of the clusters -- is `init_by_lbg(x, **lbg_params)` here, on the device (modules/lbg.py);
  * L is bounded by the E-step's LDS: 2048 (L + 1) + L (L + 1) sizeof(dtype) + 64 <= DSA_GMM_MAX_LDS_BYTES (float32: L <= 69,
    float64: L <= 63).

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py."""
from __future__ import annotations

import logging

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader

from .. import ops
from ..utils.private import to

Params = tuple[torch.Tensor, torch.Tensor, torch.Tensor]


class GaussianMixtureModeling(nn.Module):
    """order M >= 0 (L = M + 1), n_mixture K >= 1; n_iter, eps: the iteration count and the convergence threshold on the change of the total
    log-likelihood; weight_floor in [0, 1 / K], var_floor >= 0; var_type "diag" or "full" with block_size (summing to L): the structure
    of the covariance; ubm = (w, mu, sigma) and alpha in [0, 1]: MAP adaptation (gmm.py:87-177)."""

    def __init__(self, order: int, n_mixture: int, *, n_iter: int = 100, eps: float = 1e-5, weight_floor: float = 1e-5, var_floor: float = 1e-6,
                 var_type: str = "diag", block_size=None, ubm: Params | None = None, alpha: float = 0, batch_size: int | None = None,
                 verbose: bool | int = False, device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()

        if order < 0:
            raise ValueError("order must be non-negative.")
        if n_mixture <= 0:
            raise ValueError("n_mixture must be positive.")
        if n_iter <= 0:
            raise ValueError("n_iter must be positive.")
        if eps < 0:
            raise ValueError("eps must be non-negative.")
        if not 0 <= weight_floor <= 1 / n_mixture:
            raise ValueError("weight_floor must be in [0, 1 / K].")
        if var_floor < 0:
            raise ValueError("var_floor must be non-negative.")
        if not 0 <= alpha <= 1:
            raise ValueError("alpha must be in [0, 1].")

        self.order = order
        self.n_mixture = n_mixture
        self.n_iter = n_iter
        self.eps = eps
        self.weight_floor = weight_floor
        self.var_floor = var_floor
        self.alpha = alpha
        self.batch_size = batch_size
        self.verbose = verbose
        self.logger = logging.getLogger("gmm")

        if self.alpha != 0 and ubm is None:
            raise ValueError("ubm must be provided when alpha is not 0.")

        L = self.order + 1
        if block_size is None:
            block_size = [L]
        block_size = list(block_size)
        if sum(block_size) != L:
            raise ValueError("The sum of block_size must be equal to order + 1.")
        if not all(0 < b for b in block_size):
            raise ValueError("All elements of block_size must be positive.")

        self.is_diag = var_type == "diag" and len(block_size) == 1

        # the mask of the covariance: full blocks, or for "diag" the diagonals of every pair of blocks of equal size (gmm.py:150-162)
        mask = torch.zeros((L, L), device=device, dtype=dtype)
        edges = np.cumsum([0] + block_size)
        for b1, s1, e1 in zip(block_size, edges[:-1], edges[1:]):
            if var_type == "diag":
                for b2, s2, e2 in zip(block_size, edges[:-1], edges[1:]):
                    if b1 == b2:
                        mask[s1:e1, s2:e2] = torch.eye(b1)
            elif var_type == "full":
                mask[s1:e1, s1:e1] = 1
            else:
                raise ValueError(f"var_type {var_type} is not supported.")
        self.register_buffer("mask", mask, persistent=False)

        params = {"device": device, "dtype": dtype}
        K = self.n_mixture
        self.register_buffer("w", torch.ones(K, **params) / K)
        self.register_buffer("mu", torch.randn(K, L, **params))
        self.register_buffer("sigma", torch.eye(L, **params).repeat(K, 1, 1))

        if ubm is not None:
            self.set_params(ubm)
            ubm_w, ubm_mu, ubm_sigma = ubm
            self.register_buffer("ubm_w", to(ubm_w, **params))
            self.register_buffer("ubm_mu", to(ubm_mu, **params))
            self.register_buffer("ubm_sigma", to(ubm_sigma, **params))

    def set_params(self, params: tuple[torch.Tensor | None, torch.Tensor | None, torch.Tensor | None]) -> None:
        """params: (w:(K,), mu:(K, M+1), sigma:(K, M+1, M+1)), each a tensor or None: copied into the model's buffers."""
        w, mu, sigma = params
        if w is not None:
            self.w[:] = w
        if mu is not None:
            self.mu[:] = mu
        if sigma is not None:
            self.sigma[:] = sigma

    def warmup(self, x: torch.Tensor | DataLoader, **lbg_params) -> None:
        """The reference initialises the model by K-means clustering here (gmm.py:199-239); this backend does that in `init_by_lbg`."""
        raise NotImplementedError("GaussianMixtureModeling.warmup is not implemented: call init_by_lbg(x, **lbg_params), which initialises "
                                  "the model with LindeBuzoGrayAlgorithm on the device, or set_params")

    @torch.no_grad()
    def init_by_lbg(self, x: torch.Tensor | DataLoader, **lbg_params) -> None:
        """x:(T, M+1) of the module's dtype, or a DataLoader: the parameters from K-means clustering, as gmm.py:199-239 computes them --
        w = count / T, mu = the codebook of LindeBuzoGrayAlgorithm(order, n_mixture, **lbg_params), sigma = (sum of x x^T of the cluster /
        count - mu mu^T) * mask -- and `set_params`.  A cluster without data gives the reference's 0 / 0."""
        from .lbg import LindeBuzoGrayAlgorithm

        x = self._gather(x)
        lbg = LindeBuzoGrayAlgorithm(self.order, self.n_mixture, device=self.w.device, **lbg_params)
        codebook, indices, _ = lbg(x, return_indices=True)
        count, kxx = ops.gmm_cluster_moments(x.to(self.w.dtype), indices, self.n_mixture)
        mm = codebook.unsqueeze(-1) * codebook.unsqueeze(-2)   # (K, L, L), in the codebook's float32 as the reference forms it
        sigma = (kxx / count.view(-1, 1, 1) - mm) * self.mask
        w = count / torch.full_like(count, len(indices))   # a true division (by a Python number torch multiplies by the reciprocal)
        self.set_params((w, codebook, sigma))

    def _gather(self, x: torch.Tensor | DataLoader) -> torch.Tensor:
        if isinstance(x, DataLoader):   # the batches on the device, once
            return torch.cat([batch[0].to(self.w.device) for batch in x])
        if isinstance(x, torch.Tensor):
            return x
        raise ValueError(f"Unsupported input type: {type(x)}.")

    def _ubm(self):
        if self.alpha == 0:
            return None
        return tuple(t.contiguous() for t in (self.ubm_w, self.ubm_mu, self.ubm_sigma))

    @torch.inference_mode()
    def forward(self, x: torch.Tensor | DataLoader, return_posterior: bool = False):
        """x:(T, M+1) or a DataLoader -> ((w, mu, sigma), log_likelihood), or ((w, mu, sigma), posterior:(T, K), log_likelihood): the
        parameters after at most n_iter EM iterations and the total log-likelihood of the E-step before the last update
        (gmm.py:241-392).  Not differentiable."""
        x = self._gather(x)
        ops._check_gmm(x, self.w, self.mu, self.sigma)
        x = x.contiguous()
        # the iteration works on fresh tensors and the buffers are rebound at the end, as the reference rebinds them per iteration
        w, mu, sigma = (t.clone(memory_format=torch.contiguous_format) for t in (self.w, self.mu, self.sigma))
        mask, ubm = self.mask.contiguous(), self._ubm()
        readback = torch.empty(2, device=x.device, dtype=torch.float64)
        T = x.size(0)

        prev = torch.tensor(-torch.inf, dtype=x.dtype)
        log_likelihood = None
        for n in range(self.n_iter):
            log_likelihood = ops.gmm_em_step(x, w, mu, sigma, mask, ubm, self.is_diag, self.alpha, self.weight_floor, self.var_floor, readback)
            total, status = readback.tolist()   # the one host read of the iteration
            if status:
                self.w, self.mu, self.sigma = w, mu, sigma
                raise torch.linalg.LinAlgError(f"gmm: the covariance of component {int(status) - 1} is not positive-definite "
                                               f"(iteration {n + 1}): its Cholesky factorisation could not be completed")
            if self.verbose:
                self.logger.info(f"iter {n + 1:5d}: average = {total / T:g}")
            current = torch.tensor(total, dtype=x.dtype)   # the reference compares in the module's precision
            change = current - prev
            if n and change < self.eps:
                break
            prev = current
        self.w, self.mu, self.sigma = w, mu, sigma

        params = (self.w, self.mu, self.sigma)
        if return_posterior:
            posterior, _, _ = ops.gmm_estep(x, w, mu, sigma, self.is_diag)
            return params, posterior, log_likelihood
        return params, log_likelihood

    def transform(self, x: torch.Tensor):
        """x:(T, N+1) -> (y:(T, M-N) or None when N = M, indices:(T,) int64, log_prob:(T,)): the component with the largest posterior
        given the leading N+1 elements, and y = mu_y[k] + sigma_yx[k] sigma_xx[k]^-1 (x - mu_x[k]) (gmm.py:394-432).  No host read."""
        N = x.size(-1) - 1
        posterior, log_prob = self._e_step(x, reduction="none", in_order=N)
        y, indices = ops.gmm_transform(x, posterior, self.mu, self.sigma, N + 1)
        return y, indices, log_prob

    def _e_step(self, x: torch.Tensor | DataLoader, reduction: str = "sum", in_order: int | None = None):
        """(posterior:(T, K), log-likelihood: (T,) for reduction "none", their sum for "sum") on the leading in_order + 1 elements."""
        if reduction not in ("none", "sum"):
            raise ValueError(f"reduction {reduction} is not supported.")
        x = self._gather(x)
        Lp = self.order + 1 if in_order is None else in_order + 1
        posterior, ll, total = ops.gmm_estep(x, self.w, self.mu, self.sigma, self.is_diag, Lp)
        return posterior, (ll if reduction == "none" else total)
