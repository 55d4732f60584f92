"""The LPC branch: autocorrelation, Levinson-Durbin, LPC, and frame + window + LPC in one launch (csrc/lpc.hip; the kernels tuned for
float32 and lpc_order 24: csrc/lpc24.hip, csrc/lpc24_bwd.hip)."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _mcep_scratch, _p, _require_device, _same_dtype, _scratch, _stream, num_frames, pad_mode_code


class AcorrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, M, fmt):
        _require_device(x)
        xc = x.contiguous()
        L = xc.size(-1)
        F = xc.numel() // L
        r = torch.empty(*xc.shape[:-1], M + 1, device=x.device, dtype=x.dtype)
        with torch.cuda.device(x.device):
            _call("dsa_acorr_fwd", _p(xc), F, L, M, fmt, _dtype_code(xc), _p(r), _stream())
        ctx.save_for_backward(xc)
        ctx.cfg = (M, fmt)
        return r

    @staticmethod
    @once_differentiable
    def backward(ctx, gr):
        (xc,) = ctx.saved_tensors
        M, fmt = ctx.cfg
        gr = gr.contiguous()
        L = xc.size(-1)
        F = xc.numel() // L
        gx = torch.empty_like(xc)
        with torch.cuda.device(gr.device):
            _call("dsa_acorr_bwd", _p(gr), _p(xc), F, L, M, fmt, _dtype_code(xc), _p(gx), _stream())
        return gx, None, None


class LevdurFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, eps):
        _require_device(r)
        rc = r.contiguous()
        M = rc.size(-1) - 1
        F = rc.numel() // (M + 1)
        out = torch.empty_like(rc)
        with torch.cuda.device(r.device):
            _call("dsa_levdur_fwd", _p(rc), F, M, float(eps), _dtype_code(rc), _p(out), _stream())
        ctx.save_for_backward(rc, out)
        ctx.eps = eps
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rc, out = ctx.saved_tensors
        g = g.contiguous()
        M = rc.size(-1) - 1
        F = rc.numel() // (M + 1)
        gr = torch.empty_like(rc)
        with torch.cuda.device(g.device):
            _call("dsa_levdur_bwd", _p(g), _p(rc), _p(out), F, M, float(ctx.eps), _dtype_code(rc), _p(gr),
                  _stream())
        return gr, None


class LpcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, M, eps):
        _require_device(x)
        xc = x.contiguous()
        L = xc.size(-1)
        F = xc.numel() // L
        out = torch.empty(*xc.shape[:-1], M + 1, device=x.device, dtype=x.dtype)
        scratch = _scratch(x.device)
        with torch.cuda.device(x.device):
            _call("dsa_lpc_fwd", _p(xc), F, L, M, float(eps), _dtype_code(xc), _p(scratch), _p(out), _stream())
        ctx.save_for_backward(xc, out)
        ctx.cfg = (M, eps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xc, out = ctx.saved_tensors
        M, eps = ctx.cfg
        g = g.contiguous()
        L = xc.size(-1)
        F = xc.numel() // L
        gx = torch.empty_like(xc)
        with torch.cuda.device(g.device):
            _call("dsa_lpc_bwd", _p(g), _p(xc), _p(out), F, L, M, float(eps), _dtype_code(xc), _p(gx), _stream())
        return gx, None, None


def frame_window_lpc(x, window, L, P, M, eps, center=True, mode="constant", exact_lag_sums=False):
    """Fused LPC branch, forward: LPC(Window(Frame(x))), README.md:198-201 of the reference.  exact_lag_sums: float64 lag sums on
    the vector unit instead of binary16 splits on the matrix pipe (DSA_LPC_EXACT_LAGSUMS; for near-singular frames)."""
    _require_device(x, window)
    _same_dtype(x, window)
    xc, wc = x.contiguous(), window.contiguous()
    T = xc.size(-1)
    B = xc.numel() // T
    out = torch.empty(*xc.shape[:-1], num_frames(T, P), M + 1, device=x.device, dtype=x.dtype)
    # the kept-zero per-(device, stream) counters of the persistent kernels (the kernel hands them back zeroed: no fill launch per call;
    # under graph capture a private block and the library's own reset, see _mcep_scratch).  The mel-cepstral launch bits
    # (overlapped launches, reserved CUs) are not the LPC entry's: only its own flags go with the pad mode.
    scratch, clean = _mcep_scratch(x.device)
    flag = _lib.LPC_SCRATCH_IS_CLEAN if clean else 0
    if exact_lag_sums:
        flag |= _lib.LPC_EXACT_LAGSUMS
    with torch.cuda.device(x.device):
        _call("dsa_frame_window_lpc_fwd", _p(xc), B, T, L, P, _p(wc), int(center), pad_mode_code(mode) | flag, M,
              float(eps), _dtype_code(xc), _p(scratch), _p(out), _stream())
    return out


def frame_window_lpc_bwd_supported(x, L, P, M, center, mode) -> bool:
    """dsa_frame_window_lpc_bwd takes this configuration (the conditions of its launcher, csrc/lpc24_bwd.hip): float32, lpc_order 24,
    25 <= frame_length <= 512, constant padding, and a (frame_length, frame_period) pair whose overlap fits the wave's stretch."""
    if not (x.is_cuda and x.dtype == torch.float32 and M == 24 and 25 <= L <= 512 and mode == "constant" and P >= 1 and x.size(-1) >= 1):
        return False
    left = L // 2 if center else 0
    halo = (left - 1) // P - (left - L) // P          # (Python's floor division, as lb_floordiv)
    return L + P <= 1024 and halo <= 48 and min(64 - halo, num_frames(x.size(-1), P)) >= 1


class FrameWindowLpcFn(torch.autograd.Function):
    """LPC(Window(Frame(x))) (README.md:198-201 of the reference; frame.py:120-141, window.py:185-193, lpc.py:137-139) as ONE launch
    forward (dsa_frame_window_lpc_fwd) and ONE launch backward (dsa_frame_window_lpc_bwd): no (B N, L) tensor in memory either
    way.  A fixed window; callers check frame_window_lpc_bwd_supported first."""

    @staticmethod
    def forward(ctx, x, window, L, P, M, eps, center, exact_lag_sums):
        out = frame_window_lpc(x, window, L, P, M, eps, center, "constant", exact_lag_sums)
        ctx.save_for_backward(x.contiguous(), window.contiguous())
        ctx.cfg = (L, P, M, eps, center)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xc, wc = ctx.saved_tensors
        L, P, M, eps, center = ctx.cfg
        gc = g.contiguous()
        T = xc.size(-1)
        gx = torch.empty_like(xc)
        with torch.cuda.device(g.device):
            _call("dsa_frame_window_lpc_bwd", _p(gc), _p(xc), xc.numel() // T, T, L, P, _p(wc), int(center), pad_mode_code("constant"),
                  M, float(eps), _dtype_code(xc), _p(gx), _stream())
        return gx, None, None, None, None, None, None, None


def _rows(t):
    """(contiguous tensor, F, M) of a (..., M+1) tensor of coefficient rows."""
    tc = t.contiguous()
    M1 = tc.size(-1)
    return tc, tc.numel() // M1, M1 - 1


class Lpc2ParFn(torch.autograd.Function):
    """lpc2par.py:103-120 (the step-down recursion) in one launch; the backward works from the output k alone."""

    @staticmethod
    def forward(ctx, a, gamma):
        _require_device(a)
        ac, F, M = _rows(a)
        k = torch.empty_like(ac)
        with torch.cuda.device(a.device):
            _call("dsa_lpc2par_fwd", _p(ac), F, M, float(gamma), _dtype_code(ac), _p(k), _stream())
        ctx.save_for_backward(k)
        ctx.gamma = gamma
        return k

    @staticmethod
    @once_differentiable
    def backward(ctx, gk):
        (k,) = ctx.saved_tensors
        gk, F, M = _rows(gk)
        ga = torch.empty_like(k)
        with torch.cuda.device(gk.device):
            _call("dsa_lpc2par_bwd", _p(gk), _p(k), F, M, float(ctx.gamma), _dtype_code(k), _p(ga), _stream())
        return ga, None


class Par2LpcFn(torch.autograd.Function):
    """par2lpc.py:101-107 (the step-up recursion) in one launch; the backward recomputes from the input k."""

    @staticmethod
    def forward(ctx, k, gamma):
        _require_device(k)
        kc, F, M = _rows(k)
        a = torch.empty_like(kc)
        with torch.cuda.device(k.device):
            _call("dsa_par2lpc_fwd", _p(kc), F, M, float(gamma), _dtype_code(kc), _p(a), _stream())
        ctx.save_for_backward(kc)
        ctx.gamma = gamma
        return a

    @staticmethod
    @once_differentiable
    def backward(ctx, ga):
        (kc,) = ctx.saved_tensors
        ga, F, M = _rows(ga)
        gk = torch.empty_like(kc)
        with torch.cuda.device(ga.device):
            _call("dsa_par2lpc_bwd", _p(ga), _p(kc), F, M, float(ctx.gamma), _dtype_code(kc), _p(gk), _stream())
        return gk, None


class LpcCheckFn(torch.autograd.Function):
    """lpccheck.py:104-121 (step-down, clip, step-up) in one launch.  `unstable`: a zeroed int32 tensor of one element that the
    kernel sets when any |k_m| >= 1, or None.  Saves the unclipped PARCOR, and only when a gradient is wanted."""

    @staticmethod
    def forward(ctx, a, bound, unstable):
        _require_device(a)
        ac, F, M = _rows(a)
        out = torch.empty_like(ac)
        k = torch.empty_like(ac) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(a.device):
            _call("dsa_lpccheck_fwd", _p(ac), F, M, float(bound), _dtype_code(ac), _p(out), _p(k), _p(unstable), _stream())
        if k is not None:
            ctx.save_for_backward(k)
        ctx.bound = bound
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (k,) = ctx.saved_tensors
        gout, F, M = _rows(gout)
        ga = torch.empty_like(k)
        with torch.cuda.device(gout.device):
            _call("dsa_lpccheck_bwd", _p(gout), _p(k), F, M, float(ctx.bound), _dtype_code(k), _p(ga), _stream())
        return ga, None, None


def lpc2par(a, gamma=1.0):
    return Lpc2ParFn.apply(a, gamma)


def par2lpc(k, gamma=1.0):
    return Par2LpcFn.apply(k, gamma)


def lpccheck(a, bound, detect=False):
    """(out, unstable): unstable is None unless detect, else a one-element int32 tensor (non-zero: some |k_m| >= 1) that the
    caller reads back -- the only synchronisation, and only when asked for."""
    unstable = torch.zeros(1, dtype=torch.int32, device=a.device) if detect else None
    return LpcCheckFn.apply(a, bound, unstable), unstable


def _lsp_rows(t):
    """_rows for the line-spectral-pair entries, whose order is bounded (csrc/lsp.hip: one root per lane of a wave)."""
    tc, F, M = _rows(t)
    if M > _lib.LSP_MAX_ORDER:
        raise ValueError(f"the order of the line spectral pairs is {M}: at most {_lib.LSP_MAX_ORDER} (DSA_LSP_MAX_ORDER) is supported.")
    return tc, F, M


class Lpc2LspFn(torch.autograd.Function):
    """lpc2lsp.py:169-197 in one launch: a root search on two Chebyshev series, no eigen-solver.  `unit`: radians per unit of the
    output format.  `failed`: a zeroed int32 tensor of one element that the kernel sets when a row's roots were not found (that row is
    NaN), or None.  The backward works from the input a and the output w, without a root finder."""

    @staticmethod
    def forward(ctx, a, log_gain, unit, failed):
        ac, F, M = _lsp_rows(a)   # (the order first: that error needs no device)
        _require_device(a)
        w = torch.empty_like(ac)
        with torch.cuda.device(a.device):
            _call("dsa_lpc2lsp_fwd", _p(ac), F, M, int(log_gain), float(unit), _dtype_code(ac), _p(w), _p(failed), _stream())
        ctx.save_for_backward(ac, w)
        ctx.cfg = (log_gain, unit)
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, gw):
        ac, w = ctx.saved_tensors
        log_gain, unit = ctx.cfg
        gw, F, M = _rows(gw)
        ga = torch.empty_like(ac)
        with torch.cuda.device(gw.device):
            _call("dsa_lpc2lsp_bwd", _p(gw), _p(ac), _p(w), F, M, int(log_gain), float(unit), _dtype_code(ac), _p(ga), _stream())
        return ga, None, None, None


class Lsp2LpcFn(torch.autograd.Function):
    """lsp2lpc.py:171-195 in one launch: products of real second-order sections; the backward recomputes from the input w."""

    @staticmethod
    def forward(ctx, w, log_gain, unit):
        wc, F, M = _lsp_rows(w)   # (the order first: that error needs no device)
        _require_device(w)
        a = torch.empty_like(wc)
        with torch.cuda.device(w.device):
            _call("dsa_lsp2lpc_fwd", _p(wc), F, M, int(log_gain), float(unit), _dtype_code(wc), _p(a), _stream())
        ctx.save_for_backward(wc)
        ctx.cfg = (log_gain, unit)
        return a

    @staticmethod
    @once_differentiable
    def backward(ctx, ga):
        (wc,) = ctx.saved_tensors
        log_gain, unit = ctx.cfg
        ga, F, M = _rows(ga)
        gw = torch.empty_like(wc)
        with torch.cuda.device(ga.device):
            _call("dsa_lsp2lpc_bwd", _p(ga), _p(wc), F, M, int(log_gain), float(unit), _dtype_code(wc), _p(gw), _stream())
        return gw, None, None


class LspCheckFn(torch.autograd.Function):
    """lspcheck.py:115-145 in one launch, each row stopping on its own distances.  `unstable`: a zeroed int32 tensor of one element
    that the kernel sets by the test of lspcheck.py:121, or None.  The backward replays the forward from the input w."""

    @staticmethod
    def forward(ctx, w, min_distance, n_iter, unstable):
        wc, F, M = _lsp_rows(w)   # (the order first: that error needs no device)
        _require_device(w)
        out = torch.empty_like(wc)
        with torch.cuda.device(w.device):
            _call("dsa_lspcheck_fwd", _p(wc), F, M, float(min_distance), int(n_iter), _dtype_code(wc), _p(out), _p(unstable), _stream())
        ctx.save_for_backward(wc)
        ctx.cfg = (min_distance, n_iter)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (wc,) = ctx.saved_tensors
        min_distance, n_iter = ctx.cfg
        gout, F, M = _rows(gout)
        gw = torch.empty_like(wc)
        with torch.cuda.device(gout.device):
            _call("dsa_lspcheck_bwd", _p(gout), _p(wc), F, M, float(min_distance), int(n_iter), _dtype_code(wc), _p(gw), _stream())
        return gw, None, None, None


def lpc2lsp(a, log_gain=False, unit=1.0, detect=False):
    """(w, failed): failed is None unless detect, else a one-element int32 tensor (non-zero: some row's roots were not found and that
    row is NaN) for the caller to read back."""
    failed = torch.zeros(1, dtype=torch.int32, device=a.device) if detect else None
    return Lpc2LspFn.apply(a, log_gain, unit, failed), failed


def lsp2lpc(w, log_gain=False, unit=1.0):
    return Lsp2LpcFn.apply(w, log_gain, unit)


def lspcheck(w, min_distance, n_iter, detect=False):
    """(out, unstable): unstable is None unless detect, else a one-element int32 tensor (non-zero: the test of lspcheck.py:121 fired)
    that the caller reads back -- the only synchronisation, and only when asked for."""
    unstable = torch.zeros(1, dtype=torch.int32, device=w.device) if detect else None
    return LspCheckFn.apply(w, min_distance, n_iter, unstable), unstable
