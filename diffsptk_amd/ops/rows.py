"""Row products and the element-wise ends of the untuned mel-cepstral step: csrc/rows_gemm.hip, dsa_freqt_* of csrc/mcep.hip."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream

ROWS_PRO_LOG, ROWS_EPI_EXPSUB, ROWS_TRANS = _lib.ROWS_PRO_LOG, _lib.ROWS_EPI_EXPSUB, _lib.ROWS_TRANS   # DSA_ROWS_* of the header


def rows_gemm(c, A, flags=0, aux=None):
    """out = op_out(op_in(c) @ B), B = A or (ROWS_TRANS) A^T: the library's general float32 row product on the matrix instruction
    (dsa_rows_gemm, csrc/rows_gemm.hip) with the fused log prologue / exp(aux - 2 .) epilogue of the untuned mel-cepstral step."""
    cc, Ac = c.contiguous(), A.contiguous()
    K = cc.size(-1)
    N = Ac.size(0) if flags & ROWS_TRANS else Ac.size(1)
    F = cc.numel() // K
    out = torch.empty(*cc.shape[:-1], N, device=c.device, dtype=c.dtype)
    auxc = None if aux is None else aux.contiguous()
    with torch.cuda.device(c.device):
        _call("dsa_rows_gemm", _p(cc), F, K, _p(Ac), Ac.size(1), N, flags, _p(auxc), N, _dtype_code(cc), _p(out), N, _stream())
    return out


def _row_product_is_long(Lin, Lout, elt) -> bool:
    """True where the library's row-product entry (csrc/mcep.hip:dsa_freqt_fwd / _bwd) would fall to its one-workgroup-per-row
    kernel: the matrix does not fit the LDS-resident kernel's 48 KB and the shape is outside the 257-bin matrix-core kernel's
    range -- the 1025-bin products of the 48 kHz set-ups.  Those run on the general matrix-core row product (rows_gemm).  The
    choice is a function of the GEOMETRY only (never of the number of rows): a frame's result does not depend on how many frames
    share its batch (tests/test_gpu_parity.py::test_row_products_are_batch_invariant)."""
    lds_fits = elt * (Lin * Lout + 64 * (Lin + 1)) <= 48 * 1024
    return _lib.env_int("DSA_FREQT_GEMM", 1) != 0 and not lds_fits and max(Lin, Lout) >= 512


class MatmulRowsFn(torch.autograd.Function):
    """out = c @ A for a fixed (non-learnable) matrix A (freqt.py:141-143, mcep.py:286-288)."""

    @staticmethod
    def forward(ctx, c, A):
        _require_device(c, A)
        _same_dtype(c, A)
        cc, Ac = c.contiguous(), A.contiguous()
        L1, L2 = Ac.shape
        F = cc.numel() // L1
        ctx.save_for_backward(Ac)
        mfma = cc.dtype == torch.float32 and 48 < L1 <= 320 and L2 <= 192   # (the library picks its 257-bin matrix-core kernel)
        if not mfma and cc.dtype == torch.float32 and _row_product_is_long(L1, L2, cc.element_size()):
            return rows_gemm(cc, Ac)
        out = torch.empty(*cc.shape[:-1], L2, device=c.device, dtype=c.dtype)
        with torch.cuda.device(c.device):
            _call("dsa_freqt_fwd", _p(cc), F, L1, _p(Ac), L2, _dtype_code(cc), _p(out), _stream())
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (Ac,) = ctx.saved_tensors
        g = g.contiguous()
        L1, L2 = Ac.shape
        F = g.numel() // L2
        if g.dtype == torch.float32 and _row_product_is_long(L2, L1, g.element_size()):
            return rows_gemm(g, Ac, ROWS_TRANS), None
        gc = torch.empty(*g.shape[:-1], L1, device=g.device, dtype=g.dtype)
        with torch.cuda.device(g.device):
            _call("dsa_freqt_bwd", _p(g), F, L1, _p(Ac), L2, _dtype_code(g), _p(gc), _stream())
        return gc, None


class RowsLogFn(torch.autograd.Function):
    """y = log(x) (mcep.py:203) as the library's own element-wise launch, differentiable (dsa_rows_ew op 0)."""

    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous()
        y = torch.empty_like(xc)
        with torch.cuda.device(x.device):
            _call("dsa_rows_ew", 0, 0, _p(xc), None, None, xc.numel(), _dtype_code(xc), _p(y), None, _stream())
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (xc,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(xc)
        with torch.cuda.device(gy.device):
            _call("dsa_rows_ew", 0, 1, _p(xc), None, _p(gy), xc.numel(), _dtype_code(xc), _p(gx), None, _stream())
        return gx


class RowsExpSubFn(torch.autograd.Function):
    """y = exp(a - 2 b) (mcep.py:210-212), differentiable (dsa_rows_ew op 1; the backward needs the output only)."""

    @staticmethod
    def forward(ctx, a, b):
        ac, bc = a.contiguous(), b.contiguous()
        y = torch.empty_like(ac)
        with torch.cuda.device(a.device):
            _call("dsa_rows_ew", 1, 0, _p(ac), _p(bc), None, ac.numel(), _dtype_code(ac), _p(y), None, _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = gy.contiguous()
        ga, gb = torch.empty_like(y), torch.empty_like(y)
        with torch.cuda.device(gy.device):
            _call("dsa_rows_ew", 1, 1, _p(y), None, _p(gy), y.numel(), _dtype_code(y), _p(ga), _p(gb), _stream())
        return ga, gb
