"""Codebook design by the Linde-Buzo-Gray algorithm (reference: lbg.py): the codebook is doubled by splitting every codeword and refined
by K-means until the target size.  One iteration is three calls into csrc/vq.hip (four launches) -- the nearest-codeword search on float64 sums, the
per-codeword counts and float64 sums in fixed-order segments, the centroids with the iteration's three scalars -- on data that stays on
the device; the (B, K) distance matrix, histc and scatter_add_ of the reference never exist.  The order of operations is that of
lbg.py:192-331: initialisation, unused rows at 1e10, split `codebook -+ r`, E-step, convergence test before the M-step, M-step, repair of
clusters below min_data_per_cluster from the largest cluster, the optional last E-step.

What differs from the reference (include/diffsptk_amd.h, section a23):
  * the input is a (T, M+1) float32 or float64 tensor on the module's device, or a DataLoader whose batches are moved to the device and
    concatenated there ONCE; `batch_size` is accepted for parity and changes nothing (a launch covers all T vectors);
  * `forward` reads three numbers back per iteration, in one copy: the distance, which the convergence test needs (the reference
    synchronises there too), the number of clusters below the minimum and the largest cluster.  The M-step of an iteration is launched
    BEFORE that read, into a pending buffer; the host adopts the buffer after the read, or drops it when the iteration converged (the
    reference breaks before its M-step).  Because of the read `forward` cannot be captured in a graph;
  * the search forms its sums of squares in float64 from the values as stored, so the assignment is that of exact arithmetic apart from
    ties closer than float64 rounding; the centroids are float64 sums divided by the count and rounded to float32 once, in one fixed
    order: two runs give the same bits;
  * the repair of small clusters and the split are float32 element-wise steps of torch on at most K rows, and all their random numbers
    come from `self._randn(rows, cols)`: torch.randn with a torch.Generator of the MODULE'S DEVICE seeded with `seed`.  For the same seed
    these numbers differ from those of the reference's generator on another device (the CPU's, say), and so does the codebook, by about
    perturb_factor before the iterations pull it back.  With float64 input the reference repairs in float64 and rounds afterwards;
    here the centroids are float32 by then;
  * `metric` "aic" / "bic" evaluates a GaussianMixtureModeling of the module's device and x's dtype (the reference builds it on the CPU);
  * `verbose` logs the reference's lines through logging.getLogger("lbg"); there are no progress bars (no tqdm), whatever its value;
  * M + 1 <= DSA_VQ_MAX_LENGTH (64).

A quirk kept as it is: for a `codebook_size` that is no power of two and init="mean", the design starts from c = codebook_size / 2^n
codewords of which only row 0 is the mean; rows 1 .. c - 1 are whatever the constructor drew (torch.randn), here and in the reference.

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py."""
from __future__ import annotations

import logging
import math

import torch
from torch import nn
from torch.utils.data import DataLoader

from .. import ops
from .vq import VectorQuantization


class LindeBuzoGrayAlgorithm(nn.Module):
    """order M >= 0, codebook_size K >= 1; min_data_per_cluster >= 1; n_iter, eps: the iterations per codebook size and the threshold on
    the relative change of the distance; perturb_factor > 0; init "mean" or a (1~K, M+1) tensor whose row count times a power of two is K;
    metric "none", "aic" or "bic"; seed: of the random draws (lbg.py:79-144)."""

    def __init__(self, order: int, codebook_size: int, *, min_data_per_cluster: int = 1, n_iter: int = 100, eps: float = 1e-5,
                 perturb_factor: float = 1e-5, init: str | torch.Tensor = "mean", metric: str = "none", batch_size: int | None = None,
                 seed: int | None = None, verbose: bool | int = False, device: torch.device | None = None) -> None:
        super().__init__()

        if order < 0:
            raise ValueError("order must be non-negative.")
        if codebook_size <= 0:
            raise ValueError("codebook_size must be positive.")
        if min_data_per_cluster <= 0:
            raise ValueError("min_data_per_cluster must be positive.")
        if n_iter <= 0:
            raise ValueError("n_iter must be positive.")
        if eps < 0:
            raise ValueError("eps must be non-negative.")
        if perturb_factor <= 0:
            raise ValueError("perturb_factor must be positive.")

        self.order = order
        self.codebook_size = codebook_size
        self.min_data_per_cluster = min_data_per_cluster
        self.n_iter = n_iter
        self.eps = eps
        self.perturb_factor = perturb_factor
        self.metric = metric
        self.batch_size = batch_size
        self.seed = seed
        self.verbose = verbose
        self.logger = logging.getLogger("lbg")
        self._generator = None
        self.distances: list[list[float]] = []

        self.vq = VectorQuantization(order, codebook_size, device=device).eval()

        if isinstance(init, torch.Tensor):
            given_codebook_size = init.size(0)
            c = codebook_size
            while c % 2 == 0 and c != given_codebook_size:
                c //= 2
            if c != given_codebook_size:
                raise ValueError("Codebook size must be a power-of-two muptiple of the initial codebook size.")
            self.curr_codebook_size = given_codebook_size
            self.init = "none"
            self.vq.codebook[:given_codebook_size] = init
        else:
            c = codebook_size
            while c % 2 == 0:
                c //= 2
            self.curr_codebook_size = c
            self.init = init

    def _randn(self, rows: int, cols: int) -> torch.Tensor:
        """Every random draw of `forward`: (rows, cols) float32 standard normal numbers on the module's device."""
        return torch.randn(rows, cols, device=self.vq.codebook.device, dtype=torch.float32, generator=self._generator)

    @staticmethod
    def _read(readback: torch.Tensor) -> list[float]:
        """The one host read of an iteration: [distance, clusters below the minimum, first largest cluster]."""
        return readback.tolist()

    def _gather(self, x: torch.Tensor | DataLoader) -> torch.Tensor:
        if isinstance(x, DataLoader):   # the batches on the device, once
            return torch.cat([batch[0].to(self.vq.codebook.device) for batch in x])
        if isinstance(x, torch.Tensor):
            return x
        raise ValueError(f"Unsupported input type: {type(x)}.")

    @torch.inference_mode()
    def forward(self, x: torch.Tensor | DataLoader, return_indices: bool = False) -> list[torch.Tensor]:
        """x:(T, M+1) or a DataLoader -> [codebook:(K, M+1) float32, indices:(T,) int64 if return_indices, distance: 0-d in x's dtype]
        (lbg.py:146-331).  Not differentiable.

        >>> lbg = diffsptk.LBG(1, 2, seed=22, device="cuda")   # which optimum ten points reach depends on the split's draw
        >>> x = torch.tensor([[-0.5, 0.3], [0.0, 0.7], [0.2, -0.1], [3.4, 2.0], [-2.8, 1.0],
        ...                   [2.9, -3.0], [2.2, -2.5], [1.5, -1.6], [1.8, 0.5], [1.3, 0.0]], device="cuda")
        >>> codebook, indices, distance = lbg(x, return_indices=True)   # [[1.6250, 0.8000], [0.5833, -0.9833]], ..., 4.2804
        """
        x = self._gather(x)
        if x.dim() != 2:
            raise ValueError("Input vectors must be 2D.")
        if self.init not in ("none", "mean"):
            raise ValueError(f"init {self.init} is not supported.")
        codebook = self.vq.codebook
        ops._check_vq(x, codebook)
        x = x.contiguous()
        device = codebook.device
        T, L = x.shape
        readback = torch.empty(3, device=device, dtype=torch.float64)
        self._generator = torch.Generator(device)
        if self.seed is not None:
            self._generator.manual_seed(self.seed)

        # Initialize codebook.
        if self.init == "mean":
            if self.verbose:
                self.logger.info("K = 1")
            mean, _ = ops.vq_accum_update(x, torch.zeros(T, device=device, dtype=torch.int64), None, 1, 1, readback)
            codebook[0] = mean[0]
        codebook[self.curr_codebook_size:] = 1e10

        indices = None
        distance = torch.inf
        self.distances = []   # per codebook size, the distance of every E-step, as read
        while True:
            next_codebook_size = self.curr_codebook_size * 2
            if next_codebook_size <= self.codebook_size:
                # Double codebook.
                r = self._randn(self.curr_codebook_size, L) * self.perturb_factor
                codebook[self.curr_codebook_size:next_codebook_size] = codebook[:self.curr_codebook_size] - r
                codebook[:self.curr_codebook_size] += r
                self.curr_codebook_size = next_codebook_size
            K = self.curr_codebook_size

            if self.verbose:
                self.logger.info(f"K = {K}")

            prev_distance = distance
            self.distances.append([])
            for n in range(self.n_iter):
                # E-step and, into the pending buffer, the M-step; then the one host read of the iteration.
                indices, pending, n_data = ops.lbg_step(x, codebook[:K], self.min_data_per_cluster, readback)
                d, n_small, largest = self._read(readback)
                self.distances[-1].append(d)
                distance = torch.tensor(d, dtype=x.dtype)   # the reference tests convergence in x's precision
                if self.verbose:
                    self.logger.info(f"  iter {n + 1:5d}: distance = {distance:g}")

                # Check convergence.
                change = (prev_distance - distance).abs()
                if n and change / (distance + 1e-16) < self.eps:
                    break   # before the M-step: the pending centroids are dropped
                prev_distance = distance

                centroids = pending
                if n_small:
                    m, small = int(largest), int(n_small)
                    r = self._randn(small, L) * self.perturb_factor
                    centroids[n_data < self.min_data_per_cluster] = centroids[m:m + 1].expand(small, -1) - r
                    centroids[m] += r.mean(0)
                codebook[:K] = centroids

            if self.metric != "none":
                from .gmm import GaussianMixtureModeling

                gmm = GaussianMixtureModeling(self.order, K, device=device, dtype=x.dtype)
                gmm.set_params((None, codebook[:K], None))
                _, log_likelihood = gmm._e_step(x)
                n_param = K * L
                if self.metric == "aic":
                    metric = -2 * log_likelihood + n_param * 2
                elif self.metric == "bic":
                    metric = -2 * log_likelihood + n_param * math.log(T)
                else:
                    raise ValueError(f"metric {self.metric} is not supported.")
                if self.verbose:
                    self.logger.info(f"  {self.metric.upper()} = {metric:g}")

            if K == self.codebook_size:
                break

        ret = [codebook]
        if return_indices:
            indices, _, _, _ = ops.vq_search(x, codebook, False)
            ret.append(indices)
        ret.append(distance.to(device) if isinstance(distance, torch.Tensor) else distance)
        return ret

    def transform(self, x: torch.Tensor):
        """x:(T, M+1) -> (xq:(T, M+1), indices:(T,)) with the designed codebook (lbg.py:333-351)."""
        xq, indices, _ = self.vq(x)
        return xq, indices
