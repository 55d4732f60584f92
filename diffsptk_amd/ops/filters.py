"""All-zero (csrc/zerodf.hip) and all-pole (poledf.hip) time-variant filters, pseudo-QMF banks and interpolation (pqmf.hip), and the
excitation that drives the synthesis filters (excite.hip)."""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream


class ZerodfFn(torch.autograd.Function):
    """Time-variant all-zero filter (zerodf.py:207-243): x:(..., T), b:(..., T/P, M+1) -> y:(..., T)."""

    @staticmethod
    def forward(ctx, x, b, P, zeroth_index, ignore_gain):
        _require_device(x, b)
        _same_dtype(x, b)
        xc, bc = x.contiguous(), b.contiguous()
        T = xc.size(-1)
        M = bc.size(-1) - 1
        B = xc.numel() // max(T, 1)
        # the kernels index the coefficient rows by (utterance, frame): the leading dimensions must agree (zerodf() below
        # broadcasts them the way the reference's tensor arithmetic does before it gets here)
        if bc.dim() < 2 or bc.shape[:-2] != xc.shape[:-1] or bc.size(-2) * P != T:
            raise ValueError(f"zerodf: coefficients {tuple(bc.shape)} do not match the signal {tuple(xc.shape)} at frame period {P}")
        y = torch.empty_like(xc)
        with torch.cuda.device(x.device):
            _call("dsa_zerodf_fwd", _p(xc), _p(bc), B, T, M, P, zeroth_index, int(bool(ignore_gain)), _dtype_code(xc), _p(y), _stream())
        ctx.save_for_backward(xc, bc, y)
        ctx.cfg = (P, zeroth_index, int(bool(ignore_gain)))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, bc, y = ctx.saved_tensors
        P, z0, ig = ctx.cfg
        T = xc.size(-1)
        M = bc.size(-1) - 1
        B = xc.numel() // max(T, 1)
        gyc = gy.contiguous()
        gx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(bc) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(gy.device):
            _call("dsa_zerodf_bwd", _p(gyc), _p(xc), _p(bc), _p(y), B, T, M, P, z0, ig, _dtype_code(xc), _p(gx), _p(gb), _stream())
        return gx, gb, None, None, None


def _broadcast_leading(op, x, c, c_name):
    """x:(..., T) and the coefficients c:(..., T/P, M+1) with their leading dimensions broadcast against each other, as the
    reference's tensor arithmetic does (zerodf.py:207-243 accepts e.g. a batch of signals with one unbatched coefficient
    matrix).  expand() is an autograd operation, so the gradient of a broadcast operand is summed back by autograd."""
    if c.dim() < 2:
        raise ValueError(f"{op}: {c_name} must have at least two dimensions (frames, coefficients).")
    try:
        batch = torch.broadcast_shapes(x.shape[:-1], c.shape[:-2])
    except RuntimeError as e:
        raise ValueError(f"{op}: leading dimensions of x {tuple(x.shape)} and {c_name} {tuple(c.shape)} do not broadcast") from e
    if tuple(x.shape[:-1]) != tuple(batch):
        x = x.expand(*batch, x.size(-1))
    if tuple(c.shape[:-2]) != tuple(batch):
        c = c.expand(*batch, *c.shape[-2:])
    return x, c


def zerodf(x, b, P, zeroth_index, ignore_gain):
    """ZerodfFn with the leading dimensions of x:(..., T) and b:(..., T/P, M+1) broadcast against each other first."""
    x, b = _broadcast_leading("zerodf", x, b, "b")
    return ZerodfFn.apply(x, b, P, zeroth_index, ignore_gain)


class PoledfFn(torch.autograd.Function):
    """Time-variant all-pole filter (poledf.py:117-140, the recursion of torchlpc.sample_wise_lpc): x:(..., T),
    a:(..., T/P, M+1) -> y:(..., T).  Forward one launch (dsa_poledf_fwd); backward the adjoint recursion, then ga in a
    second launch when a needs a gradient (dsa_poledf_bwd)."""

    @staticmethod
    def forward(ctx, x, a, P, ignore_gain):
        _require_device(x, a)
        _same_dtype(x, a)
        xc, ac = x.contiguous(), a.contiguous()
        T = xc.size(-1)
        M = ac.size(-1) - 1
        B = xc.numel() // max(T, 1)
        if ac.dim() < 2 or ac.shape[:-2] != xc.shape[:-1] or ac.size(-2) * P != T:
            raise ValueError(f"poledf: coefficients {tuple(ac.shape)} do not match the signal {tuple(xc.shape)} at frame period {P}")
        y = torch.empty_like(xc)
        with torch.cuda.device(x.device):
            _call("dsa_poledf_fwd", _p(xc), _p(ac), B, T, M, P, int(bool(ignore_gain)), _dtype_code(xc), _p(y), _stream())
        ctx.save_for_backward(xc, ac, y)
        ctx.cfg = (P, int(bool(ignore_gain)))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, ac, y = ctx.saved_tensors
        P, ig = ctx.cfg
        T = xc.size(-1)
        M = ac.size(-1) - 1
        B = xc.numel() // max(T, 1)
        gyc = gy.contiguous()
        u = torch.empty_like(xc)   # the adjoint state (the library owns no device memory)
        gx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        ga = torch.empty_like(ac) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(gy.device):
            _call("dsa_poledf_bwd", _p(gyc), _p(xc), _p(ac), _p(y), B, T, M, P, ig, _dtype_code(xc), _p(u), _p(gx), _p(ga), _stream())
        return gx, ga, None, None


def poledf(x, a, P, ignore_gain):
    """PoledfFn with the leading dimensions of x:(..., T) and a:(..., T/P, M+1) broadcast against each other first."""
    x, a = _broadcast_leading("poledf", x, a, "a")
    return PoledfFn.apply(x, a, P, ignore_gain)


def pqmf_out_length(T: int, period: int, start: int) -> int:
    """len(range(start, T, period)): the samples Decimation(period, start) keeps (decimate.py:92)."""
    return (T - start + period - 1) // period if T > start else 0


class PqmfFn(torch.autograd.Function):
    """Pseudo-QMF analysis (pqmf.py:250-258: conv1d over the zero / replicate padded signal) with the Decimation(period, start)
    that may follow it folded in: x:(B, T), f:(K, M+1) the stored (time-flipped) filters -> y:(B, K, len(range(start, T, period))).
    (1, 0) is the plain analysis.  Backward (dsa_pqmf_bwd): gx, the replicate pad's copies summed into x[T-1], and for learnable
    filters gf from per-utterance partials in a workspace, summed in a fixed order."""

    @staticmethod
    def forward(ctx, x, f, period, start):
        _require_device(x, f)
        _same_dtype(x, f)
        xc, fc = x.contiguous(), f.contiguous()
        B, T = xc.shape
        K, M1 = fc.shape
        y = torch.empty(B, K, pqmf_out_length(T, period, start), device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_pqmf_fwd", _p(xc), _p(fc), B, T, K, M1 - 1, period, start, _dtype_code(xc), _p(y), _stream())
        ctx.save_for_backward(xc if ctx.needs_input_grad[1] else None, fc)
        ctx.cfg = (B, T, period, start)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xc, fc = ctx.saved_tensors
        B, T, period, start = ctx.cfg
        K, M1 = fc.shape
        gx = torch.empty(B, T, device=fc.device, dtype=fc.dtype) if ctx.needs_input_grad[0] else None
        gf = torch.zeros_like(fc) if ctx.needs_input_grad[1] else None   # (an empty batch leaves it zero)
        if gx is None and gf is None:
            return None, None, None, None
        work = torch.empty(B * K * M1, device=fc.device, dtype=fc.dtype) if gf is not None else None
        gyc = gy.contiguous()
        with torch.cuda.device(fc.device):
            _call("dsa_pqmf_bwd", _p(gyc), _p(xc), _p(fc), B, T, K, M1 - 1, period, start, _dtype_code(fc), _p(gx), _p(gf), _p(work),
                  _stream())
        return gx, gf, None, None


class IpqmfFn(torch.autograd.Function):
    """Pseudo-QMF synthesis (ipqmf.py:132-141) with the Interpolation(up, start) that may precede it folded in: y:(B, K, T),
    f:(K, M+1) the stored (time-flipped) filters -> x:(B, T up + start).  (1, 0) is the plain synthesis; otherwise only the taps on
    the interpolated samples are evaluated and the zero-stuffed signal is never written.  Backward (dsa_ipqmf_bwd): gy at the kept
    positions, and gf for learnable filters."""

    @staticmethod
    def forward(ctx, y, f, up, start):
        _require_device(y, f)
        _same_dtype(y, f)
        yc, fc = y.contiguous(), f.contiguous()
        B, K, T = yc.shape
        x = torch.empty(B, T * up + start, device=y.device, dtype=y.dtype)
        with torch.cuda.device(y.device):
            _call("dsa_ipqmf_fwd", _p(yc), _p(fc), B, T, K, fc.size(1) - 1, up, start, _dtype_code(yc), _p(x), _stream())
        ctx.save_for_backward(yc if ctx.needs_input_grad[1] else None, fc)
        ctx.cfg = (B, T, up, start)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        yc, fc = ctx.saved_tensors
        B, T, up, start = ctx.cfg
        K, M1 = fc.shape
        gy = torch.empty(B, K, T, device=fc.device, dtype=fc.dtype) if ctx.needs_input_grad[0] else None
        gf = torch.zeros_like(fc) if ctx.needs_input_grad[1] else None
        if gy is None and gf is None:
            return None, None, None, None
        work = torch.empty(B * K * M1, device=fc.device, dtype=fc.dtype) if gf is not None else None
        gxc = gx.contiguous()
        with torch.cuda.device(fc.device):
            _call("dsa_ipqmf_bwd", _p(gxc), _p(yc), _p(fc), B, T, K, M1 - 1, up, start, _dtype_code(fc), _p(gy), _p(gf), _p(work),
                  _stream())
        return gy, gf, None, None


class InterpolateFn(torch.autograd.Function):
    """Interpolation._forward (interpolate.py:85-96): zeros with x[..., n, ...] at start + n period along dim, one launch that
    writes every output element (dsa_interpolate_fwd); backward the strided gather (dsa_interpolate_bwd)."""

    @staticmethod
    def forward(ctx, x, period, start, dim):
        _require_device(x)
        d = dim % x.dim()
        xc = x.contiguous()
        shape = tuple(xc.shape)
        outer, T, inner = math.prod(shape[:d]), shape[d], math.prod(shape[d + 1:])
        out_shape = list(shape)
        out_shape[d] = T * period + start
        y = torch.empty(out_shape, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_interpolate_fwd", _p(xc), outer, T, inner, period, start, _dtype_code(xc), _p(y), _stream())
        ctx.cfg = (shape, outer, T, inner, period, start)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        shape, outer, T, inner, period, start = ctx.cfg
        gyc = gy.contiguous()
        gx = torch.empty(shape, device=gy.device, dtype=gy.dtype)
        with torch.cuda.device(gy.device):
            _call("dsa_interpolate_bwd", _p(gyc), outer, T, inner, period, start, _dtype_code(gyc), _p(gx), _stream())
        return gx, None, None, None


def zerodf_taylor_shapes_ok(x, b, P) -> bool:
    """Shapes the fused Taylor-stage launches cover, forward and backward (csrc/zerodf.hip:zerodf_rows_plan, zerodf_launch_bwd)."""
    return (P % 4 == 0 and 16 <= P <= 256 and b.size(-1) - 1 >= 16 and b.dim() >= 2 and tuple(b.shape[:-2]) == tuple(x.shape[:-1])
            and b.size(-2) * P == x.size(-1) and x.is_cuda and x.dtype == b.dtype and x.dtype in (torch.float32, torch.float64))


def zerodf_taylor_supported(x, b, P) -> bool:
    """zerodf_taylor_shapes_ok and no graph is being recorded."""
    return zerodf_taylor_shapes_ok(x, b, P) and not (torch.is_grad_enabled() and (x.requires_grad or b.requires_grad))


class ZerodfTaylorFn(torch.autograd.Function):
    """y = sum_{i=0}^{order} F^i x / i!  (mglsadf.py:356-365) with a graph: one launch per stage forward (filter, 1 / i, running
    sum: dsa_zerodf_taylor_fwd), one call per stage backward (dsa_zerodf_taylor_bwd: G_{i-1} = gy + F^T G_i / i and
    gb += dF(x_{i-1})^T G_i / i) -- instead of the differentiable filter + two element-wise operations per stage and autograd's
    accumulations.  x:(..., T), b:(..., T/P, M+1), shapes as zerodf_taylor_shapes_ok."""

    @staticmethod
    def forward(ctx, x, b, P, zeroth_index, order):
        xc, bc = x.contiguous(), b.contiguous()
        y = xc.clone()
        cur = xc
        stages = [xc]
        for i in range(1, order + 1):
            cur, y = zerodf_taylor(cur, bc, P, zeroth_index, 1.0 / i, y, want_y=i < order)
            if i < order:
                stages.append(cur)
        ctx.save_for_backward(bc, *stages)
        ctx.cfg = (P, zeroth_index, order)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        bc, *stages = ctx.saved_tensors
        P, z0, order = ctx.cfg
        gy = gy.contiguous()
        T = gy.size(-1)
        M = bc.size(-1) - 1
        B = gy.numel() // max(T, 1)
        gb = torch.zeros_like(bc) if ctx.needs_input_grad[1] else None
        G = gy
        with torch.cuda.device(gy.device):
            for i in range(order, 0, -1):
                G_out = torch.empty_like(gy)
                _call("dsa_zerodf_taylor_bwd", _p(G), _p(stages[i - 1]), _p(bc), B, T, M, P, z0, 1.0 / i, _p(gy), _dtype_code(gy),
                      _p(G_out), _p(gb), _stream())
                G = G_out
        return (G if ctx.needs_input_grad[0] else None), gb, None, None, None


def zerodf_taylor(x, b, P, zeroth_index, scale, acc, want_y=True):
    """One Taylor stage of the multi-stage MLSA filter without a graph (mglsadf.py:356-365): returns
    (scale * zerodf(x; b) or None, acc + scale * zerodf(x; b)) from one launch; `acc` is updated in place."""
    _require_device(x, b, acc)
    _same_dtype(x, b)
    _same_dtype(x, acc)
    xc, bc = x.contiguous(), b.contiguous()
    if not acc.is_contiguous() or acc.shape != xc.shape:
        raise ValueError("zerodf_taylor: acc must be a contiguous tensor of the signal's shape")
    if bc.dim() < 2 or bc.shape[:-2] != xc.shape[:-1] or bc.size(-2) * P != xc.size(-1):
        raise ValueError(f"zerodf_taylor: coefficients {tuple(bc.shape)} do not match the signal {tuple(xc.shape)} at frame period {P}")
    T = xc.size(-1)
    M = bc.size(-1) - 1
    B = xc.numel() // max(T, 1)
    y = torch.empty_like(xc) if want_y else None
    with torch.cuda.device(x.device):
        _call("dsa_zerodf_taylor_fwd", _p(xc), _p(bc), B, T, M, P, zeroth_index, float(scale), _p(acc), _dtype_code(xc),
              _p(y), _p(acc), _stream())
    return y, acc


EXCITE_TYPES = {"pulse": _lib.EXCITE_PULSE, "harmonic-pulse": _lib.EXCITE_HARMONIC_PULSE, "sinusoidal": _lib.EXCITE_SINUSOIDAL,
                "sawtooth": _lib.EXCITE_SAWTOOTH, "inverted-sawtooth": _lib.EXCITE_INVERTED_SAWTOOTH, "triangle": _lib.EXCITE_TRIANGLE,
                "square": _lib.EXCITE_SQUARE}


def excite(p, P, voiced_region, bipolar, shift=0.0):
    """The voiced part of ExcitationGeneration._forward (excite.py:222-310) in one launch (dsa_excite): pitch p:(..., N) in samples,
    0 = unvoiced -> (..., N P) with zeros in the unvoiced samples.  `shift`: the initial phase / 2 pi, a float or a tensor with one value
    per utterance.  Forward only: the result carries no gradient, and p is not modified."""
    _require_device(p)
    pc = p.detach().contiguous()
    N = pc.size(-1)
    B = math.prod(pc.shape[:-1])
    out = torch.empty(*pc.shape[:-1], N * P, device=pc.device, dtype=pc.dtype)
    per_utterance = None
    if isinstance(shift, torch.Tensor):
        _require_device(shift)
        _same_dtype(pc, shift)
        per_utterance = shift.detach().contiguous()
        if per_utterance.numel() != B:
            raise ValueError(f"excite: {per_utterance.numel()} shifts for {B} utterances")
    with torch.cuda.device(pc.device):
        _call("dsa_excite", _p(pc), B, N, int(P), EXCITE_TYPES[voiced_region], int(bool(bipolar)),
              0.0 if per_utterance is not None else float(shift), _p(per_utterance), _dtype_code(pc), _p(out), _stream())
    return out
