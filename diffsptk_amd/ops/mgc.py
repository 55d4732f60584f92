"""Mel-generalized cepstra: gnorm, the mgcep Newton step and its solve (csrc/mgc.hip, thsolve.hip, thsolve_quad.hip), gc2gc (mgc.hip),
the MLSA filter's stability check (mlsacheck.hip)."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream


def gnorm(x, gamma, inverse=False):
    """Gain normalisation (gnorm.py:102-112) / its inverse (ignorm.py:99-109) of (..., M + 1) rows in one launch (dsa_gnorm_fwd);
    forward only -- the modules keep the stock composition when a gradient is wanted."""
    xc = x.contiguous()
    n = xc.size(-1)
    out = torch.empty_like(xc)
    with torch.cuda.device(x.device):
        _call("dsa_gnorm_fwd", _p(xc), xc.numel() // n, n, float(gamma), int(bool(inverse)), _dtype_code(xc), _p(out), _stream())
    return out


def gnorm_applies(x) -> bool:
    """dsa_gnorm_fwd takes this call: a device tensor in float32 / float64 and no gradient wanted."""
    return x.is_cuda and x.dtype in (torch.float32, torch.float64) and not (torch.is_grad_enabled() and x.requires_grad) and x.numel() > 0


def mgcep_gain(r, b_eps, gamma, b_join):
    """(sqrt(r_0 + gamma sum_m r_{m+1} b_eps_m), b_join) as one (..., M + 1) tensor (mgcep.py:213-215, 221, 231-233; dsa_mgcep_gain),
    forward only."""
    rc, bc, jc = r.contiguous(), b_eps.contiguous(), b_join.contiguous()
    M = bc.size(-1)
    out = torch.empty(*bc.shape[:-1], M + 1, device=bc.device, dtype=bc.dtype)
    with torch.cuda.device(bc.device):
        _call("dsa_mgcep_gain", _p(rc), _p(bc), _p(jc), bc.numel() // M, M, float(gamma), _dtype_code(bc), _p(out), _stream())
    return out


def gc2gc_fused(c1, out_order, in_gamma, out_gamma, n_fft, twiddle, flags=0):
    """GeneralizedCepstrumToGeneralizedCepstrum._forward (mgc2mgc.py:333-361) in one launch (dsa_gc2gc_fwd): c1:(..., M1+1)
    -> (..., M2+1); forward only.  `flags` folds the scalar steps around it (1 gnorm before, 2 ignorm after, 4 tail * out_gamma,
    8 zeroth * out_gamma + 1).  None when the configuration has no fused kernel (n_fft not a power of two / too long)."""
    _require_device(c1, twiddle)
    _same_dtype(c1, twiddle)
    esz = 8 if c1.dtype == torch.float32 else 16
    if n_fft < 4 or n_fft & (n_fft - 1) or n_fft * esz > 150 * 1024 or out_order + 1 > n_fft:
        return None
    cc = c1.contiguous()
    n_in = cc.size(-1)
    F = cc.numel() // n_in
    out = torch.empty(*cc.shape[:-1], out_order + 1, device=c1.device, dtype=c1.dtype)
    with torch.cuda.device(c1.device):
        _call("dsa_gc2gc_fwd", _p(cc), F, n_in, out_order, float(in_gamma), float(out_gamma), n_fft, _p(twiddle), int(flags),
              _dtype_code(cc), _p(out), _stream())
    return out


class Gc2gcFn(torch.autograd.Function):
    """GeneralizedCepstrumToGeneralizedCepstrum._forward (mgc2mgc.py:333-361) with a graph: dsa_gc2gc_fwd forward, dsa_gc2gc_bwd
    backward -- one launch each, the n_fft-point spectra never in memory.  Use gc2gc_fn(): None when there is no fused kernel."""

    @staticmethod
    def forward(ctx, c1, out_order, in_gamma, out_gamma, n_fft, twiddle):
        y = gc2gc_fused(c1, out_order, in_gamma, out_gamma, n_fft, twiddle)
        ctx.save_for_backward(c1, twiddle)
        ctx.cfg = (out_order, float(in_gamma), float(out_gamma), n_fft)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g2):
        c1, tw = ctx.saved_tensors
        out_order, ig, og, n_fft = ctx.cfg
        cc, gc = c1.contiguous(), g2.contiguous()
        n_in = cc.size(-1)
        F = cc.numel() // n_in
        gc1 = torch.empty_like(cc)
        with torch.cuda.device(cc.device):
            _call("dsa_gc2gc_bwd", _p(cc), _p(gc), F, n_in, out_order, ig, og, n_fft, _p(tw), _dtype_code(cc), _p(gc1), _stream())
        return gc1, None, None, None, None, None


def gc2gc_fn(c1, out_order, in_gamma, out_gamma, n_fft, twiddle):
    """Gc2gcFn.apply where the fused kernels cover the configuration (n_fft a power of two whose five half-length arrays fit LDS),
    else None."""
    esz = 10 if c1.dtype == torch.float32 else 20
    if n_fft < 4 or n_fft & (n_fft - 1) or n_fft * esz + 64 > 150 * 1024 or out_order + 1 > n_fft or not c1.is_cuda:
        return None
    return Gc2gcFn.apply(c1, out_order, in_gamma, out_gamma, n_fft, twiddle)


def mgcep_step(x, b1, images, gamma):
    """(pt, qt, r) of one Newton step of mgcep.py:199-220 in one launch (dsa_mgcep_step: spectrum arithmetic + the five row
    products, float32 / fft_length 512 / cep_order <= 24); forward only."""
    _require_device(x, b1, images)
    _same_dtype(x, b1, images)
    xc, bc = x.contiguous(), b1.contiguous()
    K, M = xc.size(-1), bc.size(-1)
    F = xc.numel() // K
    lead = xc.shape[:-1]
    pt = torch.empty(*lead, M, device=x.device, dtype=x.dtype)
    qt = torch.empty(*lead, 2 * M - 1, device=x.device, dtype=x.dtype)
    r = torch.empty(*lead, M + 1, device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        _call("dsa_mgcep_step", _p(xc), _p(bc), F, 2 * (K - 1), M, float(gamma), _p(images), _dtype_code(xc), _p(pt), _p(qt), _p(r),
              _stream())
    return pt, qt, r


def _step_bwd_entry(images_bwd):
    """The step's adjoint: binary16 images (tables.mgcep_step_bwd_h_images, kept as int16 bit patterns so that Module.float() cannot
    cast them; float16 accepted too) select the binary16 kernel, float32 ones the round-3 kernel.  Anything else is a cast image."""
    if images_bwd.dtype in (torch.int16, torch.float16):
        if images_bwd.numel() != 9 * 22528:
            raise ValueError("mgcep step adjoint: the binary16 operand images must have 9 x 22528 entries")
        return "dsa_mgcep_step_bwd_h"
    if images_bwd.dtype != torch.float32:
        raise ValueError(f"mgcep step adjoint: operand images of dtype {images_bwd.dtype} (expected int16 / float16 or float32)")
    return "dsa_mgcep_step_bwd"


class MgcepStepFn(torch.autograd.Function):
    """(pt, qt, r) of one Newton step of mgcep.py:199-220 with a graph: forward dsa_mgcep_step, backward dsa_mgcep_step_bwd (one
    launch each; float32 / fft_length 512 / cep_order <= 24).  x:(..., 257), b1:(..., M)."""

    @staticmethod
    def forward(ctx, x, b1, images, images_bwd, gamma):
        pt, qt, r = mgcep_step(x, b1, images, gamma)
        ctx.save_for_backward(x, b1, images_bwd)
        ctx.gamma = float(gamma)
        return pt, qt, r

    @staticmethod
    @once_differentiable
    def backward(ctx, gpt, gqt, gr):
        x, b1, images_bwd = ctx.saved_tensors
        xc, bc = x.contiguous(), b1.contiguous()
        K, M = xc.size(-1), bc.size(-1)
        F = xc.numel() // K
        lead = xc.shape[:-1]

        def cot(g, n):
            return torch.zeros(*lead, n, device=xc.device, dtype=xc.dtype) if g is None else g.contiguous()

        gpt, gqt, gr = cot(gpt, M), cot(gqt, 2 * M - 1), cot(gr, M + 1)
        gx = torch.empty_like(xc)
        gb = torch.empty_like(bc)
        with torch.cuda.device(xc.device):
            _call(_step_bwd_entry(images_bwd), _p(xc), _p(bc), _p(gpt), _p(gqt), _p(gr), F, 2 * (K - 1), M, ctx.gamma, _p(images_bwd),
                  _dtype_code(xc), None, _p(gx), _p(gb), _stream())
        return gx, gb, None, None, None


def thsolve_update(pt, qt, r, b1):
    """b1 + solve(symmetric_toeplitz(pt) + hankel(qt), r[..., 1:])  (mgcep.py:226-230) in one call, the right-hand side read
    in place from the step's (.., M + 1) vector (dsa_thsolve_update_fwd: order 24, float32); forward only.  None: not covered."""
    M = pt.size(-1)
    if M != 24 or pt.dtype != torch.float32 or r.size(-1) != M + 1 or not (pt.is_contiguous() and qt.is_contiguous() and r.is_contiguous()):
        return None
    _require_device(pt, qt, r, b1)
    _same_dtype(pt, qt, r, b1)
    lead = tuple(pt.shape[:-1])
    if tuple(qt.shape) != lead + (2 * M - 1,) or tuple(r.shape) != lead + (M + 1,) or tuple(b1.shape) != lead + (M,):
        raise ValueError(f"thsolve_update: shapes {tuple(pt.shape)}, {tuple(qt.shape)}, {tuple(r.shape)}, {tuple(b1.shape)} do not "
                         "describe one batch of order-M systems")
    bc = b1.contiguous()
    F = pt.numel() // M
    out = torch.empty_like(bc)
    with torch.cuda.device(pt.device):
        _call("dsa_thsolve_update_fwd", _p(pt), _p(qt), _p(r), M + 1, 1, F, M, _dtype_code(pt), _p(bc), _p(out), _stream())
    return out


def mgcep_step_solve(x, b1, images_h, gamma, out=None, n_steps=1, want_prev=False):
    """(b1 + solve(toeplitz(pt) + hankel(qt), r[1:]), r) of one WHOLE Newton step of mgcep.py:199-230 in one launch
    (dsa_mgcep_step_solve: binary16-split matrix chains + the block elimination; float32 / fft_length 512 / cep_order 24 /
    gamma in (-1, 0)); forward only.  `images_h`: tables.mgcep_step_h_buffer as a byte tensor; `out`: where the updated coefficients
    go (may be `b1` itself when that is contiguous); `n_steps` Newton steps in the one launch (r is the last step's); `want_prev`: also
    return the last step's input coefficients (what the gain of mgcep.py:221 multiplies r with)."""
    _require_device(x, b1, images_h)
    _same_dtype(x, b1)
    xc, bc = x.contiguous(), b1.contiguous()
    K, M = xc.size(-1), bc.size(-1)
    F = xc.numel() // K
    lead = xc.shape[:-1]
    if out is None:
        out = torch.empty_like(bc)
    elif not (out.is_contiguous() and out.shape == bc.shape and out.dtype == bc.dtype and out.device == bc.device):
        raise ValueError("mgcep_step_solve: `out` must be a contiguous tensor like b1")
    r = torch.empty(*lead, M + 1, device=x.device, dtype=x.dtype)
    prev = torch.empty_like(bc) if want_prev else None
    with torch.cuda.device(x.device):
        _call("dsa_mgcep_step_solve", _p(xc), _p(bc), F, 2 * (K - 1), M, float(gamma), _p(images_h), _dtype_code(xc), _p(out), _p(r), None, None,
              int(n_steps), _p(prev), _stream())
    return (out, r, prev) if want_prev else (out, r)


class MgcepStepSolveFn(torch.autograd.Function):
    """(b1 + solve(toeplitz(pt) + hankel(qt), r[1:]), r) of one Newton step of mgcep.py:199-230 with a graph: forward ONE launch
    (dsa_mgcep_step_solve, which also leaves pt and qt behind), backward the adjoint solve (dsa_thsolve_bwd on the kept system and
    the step's solution) followed by the step's adjoint (dsa_mgcep_step_bwd) -- what autograd composes from MgcepStepFn, ThSolveFn
    and the additions around them, without their intermediate tensors.  float32 / fft_length 512 / cep_order 24."""

    @staticmethod
    def forward(ctx, x, b1, images_h, images_bwd, gamma):
        _require_device(x, b1, images_h)
        _same_dtype(x, b1)
        xc, bc = x.contiguous(), b1.contiguous()
        K, M = xc.size(-1), bc.size(-1)
        F = xc.numel() // K
        lead = xc.shape[:-1]
        out = torch.empty_like(bc)
        r = torch.empty(*lead, M + 1, device=x.device, dtype=x.dtype)
        pt = torch.empty(*lead, M, device=x.device, dtype=x.dtype)
        qt = torch.empty(*lead, 2 * M - 1, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_mgcep_step_solve", _p(xc), _p(bc), F, 2 * (K - 1), M, float(gamma), _p(images_h), _dtype_code(xc), _p(out), _p(r), _p(pt),
                  _p(qt), 1, None, _stream())
        ctx.save_for_backward(xc, bc, out, pt, qt, images_bwd)
        ctx.gamma = float(gamma)
        return out, r

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, gr):
        xc, bc, out, pt, qt, images_bwd = ctx.saved_tensors
        K, M = xc.size(-1), bc.size(-1)
        F = xc.numel() // K
        gout = torch.zeros_like(out) if gout is None else gout.contiguous()
        sol = out - bc
        gp, gq, grhs = torch.empty_like(pt), torch.empty_like(qt), torch.empty_like(sol)
        grf = torch.zeros(*xc.shape[:-1], M + 1, device=xc.device, dtype=xc.dtype) if gr is None else gr.contiguous().clone()
        gx, gb1 = torch.empty_like(xc), torch.empty_like(bc)
        with torch.cuda.device(xc.device):
            _call("dsa_thsolve_bwd", _p(gout), _p(pt), _p(qt), _p(sol), F, M, _dtype_code(pt), _p(gp), _p(gq), _p(grhs), _stream())
            grf[..., 1:] += grhs                                         # the right-hand side is r[1:]
            _call(_step_bwd_entry(images_bwd), _p(xc), _p(bc), _p(gp), _p(gq), _p(grf), F, 2 * (K - 1), M, ctx.gamma, _p(images_bwd), _dtype_code(xc),
                  None, _p(gx), _p(gb1), _stream())
        return gx, gb1 + gout, None, None, None


def mgcep_spectra(x, b1, Cr, Ci, gamma):
    """(5, ..., K): pp, qq (X^2 - Y^2), qq 2XY, pp X, pp Y of one Newton step of mgcep.py:199-209 in one launch
    (dsa_mgcep_spectra); forward only."""
    _require_device(x, b1, Cr, Ci)
    _same_dtype(x, b1, Cr, Ci)
    xc, bc = x.contiguous(), b1.contiguous()
    K, M = xc.size(-1), bc.size(-1)
    F = xc.numel() // K
    out = torch.empty((5, *xc.shape), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        _call("dsa_mgcep_spectra", _p(xc), _p(bc), F, 2 * (K - 1), M, _p(Cr.contiguous()), _p(Ci.contiguous()), float(gamma),
              _dtype_code(xc), _p(out), _stream())
    return out


class ThSolveFn(torch.autograd.Function):
    """g = solve(symmetric_toeplitz(p) + hankel(q), r) per row (mgcep.py:226-229): p:(..., n), q:(..., 2n-1), r:(..., n)."""

    @staticmethod
    def forward(ctx, p, q, r):
        _require_device(p, q, r)
        _same_dtype(p, q, r)
        pc, qc, rc = p.contiguous(), q.contiguous(), r.contiguous()
        n = pc.size(-1)
        if qc.size(-1) != 2 * n - 1 or rc.size(-1) != n:
            raise ValueError("thsolve: expected p:(..., n), q:(..., 2n-1), r:(..., n)")
        if qc.shape[:-1] != pc.shape[:-1] or rc.shape[:-1] != pc.shape[:-1]:   # the kernels index q and r by p's row number
            raise ValueError(f"thsolve: leading dimensions differ (p {tuple(pc.shape)}, q {tuple(qc.shape)}, r {tuple(rc.shape)})")
        F = pc.numel() // n
        g = torch.empty_like(rc)
        with torch.cuda.device(p.device):
            _call("dsa_thsolve_fwd", _p(pc), _p(qc), _p(rc), F, n, _dtype_code(pc), _p(g), _stream())
        ctx.save_for_backward(pc, qc, g)
        return g

    @staticmethod
    @once_differentiable
    def backward(ctx, gg):
        pc, qc, g = ctx.saved_tensors
        n = pc.size(-1)
        F = pc.numel() // n
        ggc = gg.contiguous()
        gp, gq, gr = torch.empty_like(pc), torch.empty_like(qc), torch.empty_like(ggc)
        with torch.cuda.device(gg.device):
            _call("dsa_thsolve_bwd", _p(ggc), _p(pc), _p(qc), _p(g), F, n, _dtype_code(pc), _p(gp), _p(gq), _p(gr), _stream())
        return gp, gq, gr


MLSACHECK_MODES = {"fast": _lib.MLSACHECK_FAST, "scale": _lib.MLSACHECK_SCALE, "clip": _lib.MLSACHECK_CLIP}


class MlsaCheckFn(torch.autograd.Function):
    """mlsacheck.py:181-230 in one launch (dsa_mlsacheck).  `unstable`: a zeroed int32 tensor of one element that the kernel sets when
    the threshold is below a frame's amplitude, or None.  The backward (dsa_mlsacheck_vjp) recomputes everything from the input mc:
    nothing but mc is saved."""

    @staticmethod
    def forward(ctx, mc, alpha, threshold, mode, n_fft, unstable):
        _require_device(mc)
        mcc = mc.contiguous()
        M1 = mcc.size(-1)
        out = torch.empty_like(mcc)
        with torch.cuda.device(mc.device):
            _call("dsa_mlsacheck", _p(mcc), mcc.numel() // M1, M1 - 1, float(alpha), float(threshold), int(mode), int(n_fft), _dtype_code(mcc),
                  _p(out), _p(unstable), _stream())
        ctx.save_for_backward(mcc)
        ctx.cfg = (float(alpha), float(threshold), int(mode), int(n_fft))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (mcc,) = ctx.saved_tensors
        gout = gout.contiguous()
        M1 = mcc.size(-1)
        gmc = torch.empty_like(mcc)
        with torch.cuda.device(gout.device):
            _call("dsa_mlsacheck_vjp", _p(gout), _p(mcc), mcc.numel() // M1, M1 - 1, *ctx.cfg, _dtype_code(mcc), _p(gmc), _stream())
        return gmc, None, None, None, None, None


def mlsacheck(mc, alpha, threshold, mode, n_fft, detect=False):
    """(out, unstable) of the MLSA filter's stability check on mc:(..., M+1); mode: "fast", "scale" or "clip" (MLSACHECK_MODES).
    unstable is None unless detect, else a one-element int32 tensor (non-zero: the threshold is below some frame's amplitude) that the
    caller reads back -- the only synchronisation, and only when asked for."""
    unstable = torch.zeros(1, dtype=torch.int32, device=mc.device) if detect else None
    return MlsaCheckFn.apply(mc, alpha, threshold, MLSACHECK_MODES[mode], n_fft, unstable), unstable
