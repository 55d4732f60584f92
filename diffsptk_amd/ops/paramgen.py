"""Parameter generation (csrc/paramgen.hip): delta features, maximum likelihood parameter generation, mel-cepstrum postfiltering."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream


def _check_window(op, t, window):
    _require_device(t, window)
    _same_dtype(t, window)
    if window.dim() != 2 or window.size(1) % 2 != 1 or not window.is_contiguous():
        raise ValueError(f"{op}: the window must be a contiguous (H, L) tensor with L odd, got {tuple(window.shape)}")


def _delta(name, t, B, T, D, window, out):
    if out.numel():
        with torch.cuda.device(t.device):
            _call(name, _p(t), B, T, D, _p(window), window.size(0), window.size(1), _dtype_code(t), _p(out), _stream())
    return out


class DeltaFn(torch.autograd.Function):
    """x:(B, T, D) -> (B, T, H D), h-major (delta.py:181-201).  window:(H, L).  The backward is one gather launch; nothing is saved."""

    @staticmethod
    def forward(ctx, x, window):
        _check_window("delta", x, window)
        xc = x.contiguous()
        B, T, D = xc.shape
        ctx.window = window
        return _delta("dsa_delta", xc, B, T, D, window, torch.empty(B, T, window.size(0) * D, device=xc.device, dtype=xc.dtype))

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        window = ctx.window
        gc = gy.contiguous()
        B, T, HD = gc.shape
        D = HD // window.size(0)
        return _delta("dsa_delta_vjp", gc, B, T, D, window, torch.empty(B, T, D, device=gc.device, dtype=gc.dtype)), None


def _mlpg(t, lead, T, D, window, th, factor, adjoint):
    H = window.size(0)
    B = 1
    for n in lead:
        B *= n
    tc = t.contiguous()
    out = torch.empty(*lead, T, H * D if adjoint else D, device=tc.device, dtype=tc.dtype)
    if out.numel():
        work = torch.empty(B, T, D, device=tc.device, dtype=tc.dtype) if adjoint else None
        with torch.cuda.device(tc.device):
            _call("dsa_mlpg", _p(tc), B, T, D, _p(window), _p(th), H, window.size(1), _p(factor), _lib.MLPG_ADJOINT if adjoint else _lib.MLPG_FORWARD,
                  _dtype_code(tc), _p(work), _p(out), _stream())
    return out


class MlpgFn(torch.autograd.Function):
    """u:(..., T, D H), h-major -> (..., T, D): the solution of W^T W c = W^T u (mlpg.py:165-171).  window:(H, L); th:(H) int32;
    factor:(T, L) the banded Cholesky factor of W^T W (utils.tables.mlpg_factor).  The operator is linear: the backward is the adjoint
    entry on the cotangent, with one (B, T, D) workspace, and nothing is saved."""

    @staticmethod
    def forward(ctx, u, window, th, factor):
        _check_window("mlpg", u, window)
        _require_device(th, factor)
        _same_dtype(u, factor)
        H, L = window.shape
        if u.dim() < 2:
            raise ValueError("mlpg: the input must be at least 2D.")
        T = u.size(-2)
        if u.size(-1) % H:
            raise ValueError(f"mlpg: the last dimension {u.size(-1)} is no multiple of the {H} windows.")
        if tuple(factor.shape) != (T, L) or not factor.is_contiguous() or th.dtype != torch.int32 or tuple(th.shape) != (H,):
            raise ValueError(f"mlpg: factor {tuple(factor.shape)} / th {tuple(th.shape)} do not fit {T} frames and a window {tuple(window.shape)}")
        ctx.cfg = (window, th, factor)
        return _mlpg(u, u.shape[:-2], T, u.size(-1) // H, window, th, factor, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, gc):
        window, th, factor = ctx.cfg
        return _mlpg(gc, gc.shape[:-2], gc.size(-2), gc.size(-1), window, th, factor, True), None, None, None


def _check_mcpf(mc, table, table_t):
    _require_device(mc, table, table_t)
    _dtype_code(mc)
    M1 = mc.size(-1)
    bins = table.size(0)
    if table.dtype != torch.float64 or table_t.dtype != torch.float64 or tuple(table.shape) != (bins, M1) or tuple(table_t.shape) != (M1, bins) \
            or not (table.is_contiguous() and table_t.is_contiguous()):
        raise ValueError(f"mcpf: the float64 tables {tuple(table.shape)}, {tuple(table_t.shape)} do not fit {M1} coefficients")
    if bins > _lib.MCPF_MAX_BINS:
        raise ValueError(f"ir_length must be at most {2 * (_lib.MCPF_MAX_BINS - 1)}.")
    return M1, bins


class McpfFn(torch.autograd.Function):
    """mc:(..., M+1) -> the postfiltered mel-cepstrum (mcpf.py:191-209 in closed form).  table:(bins, M+1) and table_t, its transpose,
    float64 (utils.tables.mcpf_table); scale = 1 + beta.  The backward is one launch on (mc, cotangent); only mc is saved."""

    @staticmethod
    def forward(ctx, mc, table, table_t, scale, onset):
        M1, bins = _check_mcpf(mc, table, table_t)
        mcc = mc.contiguous()
        out = torch.empty_like(mcc)
        if mcc.numel():
            with torch.cuda.device(mcc.device):
                _call("dsa_mcpf", _p(mcc), mcc.numel() // M1, M1, _p(table_t), bins, float(scale), int(onset), _dtype_code(mcc), _p(out), _stream())
        ctx.save_for_backward(mcc)
        ctx.cfg = (table, table_t, float(scale), int(onset))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (mcc,) = ctx.saved_tensors
        table, table_t, scale, onset = ctx.cfg
        gc = g.contiguous()
        gmc = torch.empty_like(mcc)
        if mcc.numel():
            M1 = mcc.size(-1)
            with torch.cuda.device(mcc.device):
                _call("dsa_mcpf_vjp", _p(mcc), _p(gc), mcc.numel() // M1, M1, _p(table), _p(table_t), table.size(0), scale, onset, _dtype_code(mcc),
                      _p(gmc), _stream())
        return gmc, None, None, None, None
