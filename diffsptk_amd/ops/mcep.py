"""Mel-cepstral analysis: the tuned kernels (csrc/mcep.hip, mcep_mfma.hip, mcep_mfma_bwd.hip), the composed Newton paths (rows_gemm.hip, thsolve.hip)."""
from __future__ import annotations

import weakref

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _mcep_scratch, _p, _require_device, _same_dtype, _stream, num_frames, pad_mode_code
from .rows import MatmulRowsFn, ROWS_EPI_EXPSUB, RowsExpSubFn, RowsLogFn, rows_gemm
from .mgc import ThSolveFn

_IMAGES: dict = {}   # id(G) -> (weakref to G, versions, images): prepared operand images, made once per set of matrices


def mcep_images(G: torch.Tensor, D: torch.Tensor, E: torch.Tensor, fft_length: int, M: int):
    """The per-configuration constants of the tuned mel-cepstral kernels (dsa_mcep_prepare): binary16 hi/lo
    operand images of G, D, E, prepared once per set of matrices and reused by every call (None when the
    configuration has no tuned kernel).  Keyed by the tensors themselves (weakly) and their version counters, so
    moving a module to another device or editing a matrix in place prepares new images."""
    if G.device.type != "cuda" or G.dtype != torch.float32:
        return None
    lib = _lib.load()
    nbytes = lib.dsa_mcep_images_bytes(fft_length, M, _lib.F32)
    if nbytes <= 0:
        return None
    ver = (G._version, D._version, E._version, G.data_ptr(), D.data_ptr(), E.data_ptr())
    hit = _IMAGES.get(id(G))
    if hit is not None and hit[0]() is G and hit[1] == ver:
        if not hit[3].query():   # prepared on another stream and possibly not done yet
            with torch.cuda.device(G.device):
                torch.cuda.current_stream().wait_event(hit[3])
        return hit[2]
    Gc, Dc, Ec = G.contiguous(), D.contiguous(), E.contiguous()
    img = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
    with torch.cuda.device(G.device):
        _call("dsa_mcep_prepare", _p(Gc), _p(Dc), _p(Ec), fft_length, M, _lib.F32, _p(img), _stream())
        # once per configuration; later calls may come from any stream, so they wait for this event on THEIR stream (no host
        # synchronisation: the preparation can sit inside a stream capture)
        ready = torch.cuda.Event()
        ready.record()
    if hit is None or hit[0]() is not G:
        weakref.finalize(G, _IMAGES.pop, id(G), None)   # the images go when the matrices go
    _IMAGES[id(G)] = (weakref.ref(G), ver, img, ready)
    return img


def _mcep_composed_applies(Xc, M) -> bool:
    """Geometries without a tuned kernel (48 kHz set-ups: fft_length 1024 / 2048, orders 34 .. 60).  A function of the geometry
    and the dtype only -- never of the number of frames: a frame's mel-cepstrum does not depend on how many frames share its
    batch.  Short spectra (fft_length < 256: the reference's own test grids) keep the generic kernel pair."""
    return (Xc.dtype == torch.float32 and M + 1 <= 64 and M >= 1 and Xc.size(-1) >= 129
            and _lib.env_int("DSA_MCEP_COMPOSED", 1) != 0)   # float64 keeps the generic kernel pair


def mcep_composed(X, G, D, E, av, fft_length, M, n_iter, algo):
    """The mel-cepstral analysis for a geometry without a tuned kernel, WITH a graph when one is wanted: the whole-batch
    launches of _mcep_composed_fwd are differentiable operations (GEMMs, element-wise, ThSolveFn), so autograd runs the
    backward as whole-batch launches too (the generic kernel pair keeps one workgroup per frame in both directions).
    None: not applicable (a tuned kernel exists, the generic family was asked for, or the spectrum is short)."""
    if algo == _lib.ALGO_GENERIC or X.device.type != "cuda":
        return None
    K = fft_length // 2 + 1
    F = X.numel() // K
    if not _mcep_composed_applies(X, M) or mcep_images(G, D, E, fft_length, M) is not None:
        return None
    _require_device(X, G, D, E, av)
    _same_dtype(X, G, D, E, av)
    return _mcep_composed_fwd(X.contiguous(), G, D, E, av, M, n_iter)


def mcep_newton_update(rt, av, mc):
    """mc + solve(T(rt[:, :n]) + H(rt), rt[:, :n] - av) (mcep.py:216-222; dsa_mcep_newton_update, float32, n <= 55)."""
    n = mc.size(-1)
    out = torch.empty_like(mc)
    with torch.cuda.device(mc.device):
        _call("dsa_mcep_newton_update", _p(rt), mc.numel() // n, n, _p(av), _dtype_code(mc), _p(mc), _p(out), _stream())
    return out


class McepNewtonUpdateFn(torch.autograd.Function):
    """mc + solve(T(rt[:, :n]) + H(rt), rt[:, :n] - av) with a gradient (mcep.py:216-222): forward = the batched solve (the solution is
    kept), backward = the same solve on the cotangent and one launch of diagonal sums (dsa_mcep_newton_update_bwd).  As a slice, a
    subtraction, ThSolveFn and an addition the step was nine small stock launches around the two kernels, in each direction."""

    @staticmethod
    def forward(ctx, rt, av, mc):
        rtc = rt.contiguous()
        n = mc.size(-1)
        sol = torch.empty_like(mc)
        with torch.cuda.device(mc.device):
            _call("dsa_mcep_newton_update", _p(rtc), mc.numel() // n, n, _p(av), _dtype_code(mc), None, _p(sol), _stream())
        ctx.save_for_backward(rtc, sol)
        return mc + sol

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rtc, sol = ctx.saved_tensors
        n = sol.size(-1)
        gc = g.contiguous()
        u, grt = torch.empty_like(sol), torch.empty_like(rtc)
        with torch.cuda.device(g.device):
            _call("dsa_mcep_newton_update_bwd", _p(gc), _p(rtc), _p(sol), sol.numel() // n, n, _dtype_code(sol), _p(u), _p(grt), _stream())
        return grt, None, g


def mcep_newton_resid(logx, mc, D, E):
    """rt = exp(logx - 2 mc D) E (mcep.py:210-215) in one launch (dsa_mcep_newton_resid: float32, 3 <= M + 1 <= 55): e is formed
    chunk by chunk in the operand layout of the second product and never reaches memory."""
    n, K = mc.size(-1), logx.size(-1)
    Dc, Ec = D.contiguous(), E.contiguous()
    rt = torch.empty(*mc.shape[:-1], 2 * n - 1, device=mc.device, dtype=mc.dtype)
    with torch.cuda.device(mc.device):
        _call("dsa_mcep_newton_resid", _p(logx), mc.numel() // n, K, _p(mc), n, _p(Dc), Dc.size(1), _p(Ec), Ec.size(1),
              _dtype_code(mc), _p(rt), _stream())
    return rt


_RESID_IMAGES: dict = {}   # id(D) -> (weakref to D, versions, images, ready event): the binary16 operand images of dsa_mcep_newton_resid_h


def mcep_resid_images(D, E):
    """The binary16 hi / lo operand images dsa_mcep_newton_resid_h consumes (dsa_mcep_resid_prepare: one small launch), made once per
    pair of tables and kept as long as the tables live (keyed like mcep_images: weakly by the tensors and their version counters; a call
    from another stream waits for the preparation's event on ITS stream)."""
    if D.device.type != "cuda" or D.dtype != torch.float32 or E.dtype != torch.float32:
        return None
    n, K = D.size(0), D.size(1)
    nbytes = _lib.load().dsa_mcep_resid_images_bytes(K, n)
    if nbytes <= 0:
        return None
    ver = (D._version, E._version, D.data_ptr(), E.data_ptr(), tuple(D.shape), tuple(E.shape))
    hit = _RESID_IMAGES.get(id(D))
    if hit is not None and hit[0]() is D and hit[1] == ver:
        if not hit[3].query():
            with torch.cuda.device(D.device):
                torch.cuda.current_stream().wait_event(hit[3])
        return hit[2]
    Dc, Ec = D.contiguous(), E.contiguous()
    images = torch.empty(nbytes, dtype=torch.uint8, device=D.device)
    with torch.cuda.device(D.device):
        _call("dsa_mcep_resid_prepare", _p(Dc), Dc.size(1), _p(Ec), Ec.size(1), K, n, _dtype_code(Dc), _p(images), _stream())
        ready = torch.cuda.Event()
        ready.record()
    if hit is None or hit[0]() is not D:
        weakref.finalize(D, _RESID_IMAGES.pop, id(D), None)
    _RESID_IMAGES[id(D)] = (weakref.ref(D), ver, images, ready)
    return images


_RESID_BWD_IMAGES: dict = {}   # id(D) -> (weakref to D, versions, images, ready event): the operand images of dsa_mcep_newton_resid_h_bwd


def mcep_resid_bwd_images(D, E):
    """The binary16 hi / lo operand images dsa_mcep_newton_resid_h_bwd consumes (dsa_mcep_resid_bwd_prepare), made once per pair of
    tables and kept as long as the tables live (as mcep_resid_images); None where no kernel covers the order."""
    if D.device.type != "cuda" or D.dtype != torch.float32 or E.dtype != torch.float32:
        return None
    n, K = D.size(0), D.size(1)
    nbytes = _lib.load().dsa_mcep_resid_bwd_images_bytes(K, n)
    if nbytes <= 0:
        return None
    ver = (D._version, E._version, D.data_ptr(), E.data_ptr(), tuple(D.shape), tuple(E.shape))
    hit = _RESID_BWD_IMAGES.get(id(D))
    if hit is not None and hit[0]() is D and hit[1] == ver:
        if not hit[3].query():
            with torch.cuda.device(D.device):
                torch.cuda.current_stream().wait_event(hit[3])
        return hit[2]
    Dc, Ec = D.contiguous(), E.contiguous()
    images = torch.empty(nbytes, dtype=torch.uint8, device=D.device)
    with torch.cuda.device(D.device):
        _call("dsa_mcep_resid_bwd_prepare", _p(Dc), Dc.size(1), _p(Ec), Ec.size(1), K, n, _dtype_code(Dc), _p(images), _stream())
        ready = torch.cuda.Event()
        ready.record()
    if hit is None or hit[0]() is not D:
        weakref.finalize(D, _RESID_BWD_IMAGES.pop, id(D), None)
    _RESID_BWD_IMAGES[id(D)] = (weakref.ref(D), ver, images, ready)
    return images


MCEP_GLOGX_MIN_FRAMES = 20480   # (tools/sweep_glogx_threshold.py: 16 384 frames 2.55 against 2.53 ms accumulating, 24 576: 3.40 against 3.73)


class McepNewtonStepsHFn(torch.autograd.Function):
    """mcep.py:208-222 at the 48 kHz set-ups (orders 32 .. 54) WITH a gradient, as one node (round 6): forward = per Newton step
    dsa_mcep_newton_resid_h + dsa_mcep_newton_update, the iterates, rt rows and solutions kept ((3 n + ...) floats per frame and step
    -- not e:(F, K)); backward = per step, in reverse, dsa_mcep_newton_update_bwd (the solve on the cotangent, the diagonal sums) and
    dsa_mcep_newton_resid_h_bwd (e recomputed from the iterate; glogx accumulated in place).  Inputs: logx (natural logarithms of the
    spectrum) and the start mc0 = logx G; the tables D, E, alpha_vec carry no gradient here (a learnable basis takes the composed
    path).  Replaces, per step and 102 400 frames at 2048 / 49, 2.0 ms of differentiable pieces by 0.5 + 0.7 ms."""

    @staticmethod
    def forward(ctx, logx, mc0, D, E, av, n_iter):
        images = mcep_resid_images(D, E)
        F, n = mc0.numel() // mc0.size(-1), mc0.size(-1)
        K = logx.size(-1)
        lx = logx.contiguous()
        mcs = torch.empty(n_iter + 1, F, n, device=mc0.device, dtype=mc0.dtype)   # the iterates
        rts = torch.empty(n_iter, F, 2 * n - 1, device=mc0.device, dtype=mc0.dtype)
        sols = torch.empty(n_iter, F, n, device=mc0.device, dtype=mc0.dtype)
        mcs[0].copy_(mc0.reshape(F, n))
        with torch.cuda.device(mc0.device):
            for i in range(n_iter):
                _call("dsa_mcep_newton_resid_h", _p(lx), F, K, _p(mcs[i]), n, _p(images), _dtype_code(lx), _p(rts[i]), _stream())
                _call("dsa_mcep_newton_update", _p(rts[i]), F, n, _p(av), _dtype_code(lx), None, _p(sols[i]), _stream())
                torch.add(mcs[i], sols[i], out=mcs[i + 1])
        ctx.save_for_backward(lx, mcs, rts, sols, D, E)
        ctx.n_iter = n_iter
        return mcs[n_iter].reshape(mc0.shape).clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lx, mcs, rts, sols, D, E = ctx.saved_tensors
        n_iter = ctx.n_iter
        F, n = mcs.size(1), mcs.size(2)
        K = lx.size(-1)
        images_b = mcep_resid_bwd_images(D, E)
        gbar = g.reshape(F, n).contiguous().clone()
        u, gmc = torch.empty_like(gbar), torch.empty_like(gbar)
        # 0.2.2: the sum over the steps that lands in glogx is formed AFTER the sweep, in one pass over the bins from the iterates and the
        # steps' cotangents grt (kept: 4 (2 n - 1) bytes per frame and step) -- dsa_mcep_newton_glogx_h; the sweep's launches then leave
        # glogx alone (a step moves the (F, K) array once instead of three times).  Same values summed in the same order: the same bits
        # as the in-place accumulation (DSA_MCEP_GLOGX_PASS=0, and n_iter beyond what the pass holds on chip).
        # (from MCEP_GLOGX_MIN_FRAMES frames on: below, the pass's one-tile workgroups leave CUs idle -- 12 800 frames at 2048 / 49: 2.42 ms
        #  accumulating, 2.48 with the pass; DSA_MCEP_GLOGX_PASS=1 forces it, =0 forbids it.  The bits do not depend on the choice.)
        env = _lib.env_int("DSA_MCEP_GLOGX_PASS", -1)
        one_pass = (env != 0 and (F >= MCEP_GLOGX_MIN_FRAMES or env == 1)
                    and n_iter * ((4 + 2 * ((2 * n - 1 + 31) // 32)) * 1024 + 128) <= 156 * 1024)
        with torch.cuda.device(g.device):
            if one_pass:
                grts = torch.empty_like(rts)
                for i in range(n_iter - 1, -1, -1):
                    _call("dsa_mcep_newton_update_bwd", _p(gbar), _p(rts[i]), _p(sols[i]), F, n, _dtype_code(lx), _p(u), _p(grts[i]), _stream())
                    _call("dsa_mcep_newton_resid_h_bwd", _p(lx), F, K, _p(mcs[i]), n, _p(grts[i]), _p(images_b), _dtype_code(lx), None, _p(gmc),
                          _stream())
                    gbar.add_(gmc)
                glogx = torch.empty_like(lx)
                rc = getattr(_lib.load(), "dsa_mcep_newton_glogx_h")(_p(lx), F, K, _p(mcs), n, _p(grts), int(n_iter), _p(images_b),
                                                                       _dtype_code(lx), _p(glogx), _stream())
                if rc == _lib.ERR_UNSUPPORTED:   # (cannot happen for what mcep_newton_steps_grad_applies admits; kept as the contract says)
                    glogx.zero_()
                    for i in range(n_iter):
                        _call("dsa_mcep_newton_resid_h_bwd", _p(lx), F, K, _p(mcs[i]), n, _p(grts[i]), _p(images_b), _dtype_code(lx), _p(glogx),
                              _p(gmc), _stream())
                else:
                    _lib.check(rc, "dsa_mcep_newton_glogx_h")
            else:
                glogx = torch.zeros_like(lx)
                grt = torch.empty_like(rts[0])
                for i in range(n_iter - 1, -1, -1):
                    _call("dsa_mcep_newton_update_bwd", _p(gbar), _p(rts[i]), _p(sols[i]), F, n, _dtype_code(lx), _p(u), _p(grt), _stream())
                    _call("dsa_mcep_newton_resid_h_bwd", _p(lx), F, K, _p(mcs[i]), n, _p(grt), _p(images_b), _dtype_code(lx), _p(glogx), _p(gmc),
                          _stream())
                    gbar.add_(gmc)
        return glogx.reshape(lx.shape), gbar.reshape(g.shape), None, None, None, None


def mcep_newton_steps_grad_applies(M1, D, E, av):
    """McepNewtonStepsHFn takes the analysis: orders 32 .. 54, float32 tables without a gradient of their own
    (DSA_MCEP_GRAD_H=0: the composed path, for A/B runs)."""
    return (33 <= M1 <= 55 and _lib.env_int("DSA_MCEP_GRAD_H", 1) != 0 and D.dtype == torch.float32 and E.dtype == torch.float32
            and av.dtype == torch.float32 and not (D.requires_grad or E.requires_grad or av.requires_grad)
            and D.device.type == "cuda" and _lib.load().dsa_mcep_resid_bwd_images_bytes(D.size(1), D.size(0)) > 0
            and _lib.load().dsa_mcep_resid_images_bytes(D.size(1), D.size(0)) > 0)


def mcep_newton_resid_h(logx, mc, images):
    """rt = exp(logx - 2 mc D) E (mcep.py:210-215) in one launch with both products as 3-term binary16 splits on the matrix pipe
    (dsa_mcep_newton_resid_h: float32, 3 <= M + 1 <= 55); `images` from mcep_resid_images(D, E)."""
    n, K = mc.size(-1), logx.size(-1)
    rt = torch.empty(*mc.shape[:-1], 2 * n - 1, device=mc.device, dtype=mc.dtype)
    with torch.cuda.device(mc.device):
        _call("dsa_mcep_newton_resid_h", _p(logx), mc.numel() // n, K, _p(mc), n, _p(images), _dtype_code(mc), _p(rt), _stream())
    return rt


def mcep_newton_steps_applies(M1: int) -> bool:
    """dsa_mcep_newton_steps has an instantiation for this order (32 .. 54, among them the 48 kHz set-ups fft_length 2048 / order 49
    and 1024 / order 34).  DSA_MCEP_BIG=0 (the two-launch step, for A/B runs) is the library's to read: the entry then refuses."""
    return 33 <= M1 <= 55


def mcep_newton_steps(logx, mc0, images, av, n_iter):
    """ALL n_iter Newton steps of mcep.py:208-222 in ONE persistent launch (dsa_mcep_newton_steps, csrc/mcep_big_f16.h): per step the
    products of mcep_newton_resid_h and the solve-and-update of mcep_newton_update, rt and mc staying on chip; forward only.
    None: the library has no instantiation for this order after all, or DSA_MCEP_BIG=0 (the caller runs the two launches per step)."""
    n, K = mc0.size(-1), logx.size(-1)
    mcc = mc0.contiguous()
    out = torch.empty_like(mcc)
    with torch.cuda.device(mcc.device):
        rc = getattr(_lib.load(), "dsa_mcep_newton_steps")(_p(logx), mcc.numel() // n, K, _p(mcc), n, _p(images), _p(av), int(n_iter),
                                                            _dtype_code(mcc), _p(out), _stream())
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "dsa_mcep_newton_steps")
    return out


def _mcep_composed_fwd(Xc, G, D, E, av, M, n_iter):
    """mcep.py:203-222 for the geometries the tuned kernel does not cover, as whole-batch launches of the library's own kernels
    instead of the one-workgroup-per-frame generic kernel: per Newton step the two row products (F, M+1) x (M+1, K) and
    (F, K) x (K, 2M+1) with exp(log X - 2 .) between them as ONE matrix-core launch (dsa_mcep_newton_resid; orders above 54: two
    launches of dsa_rows_gemm) and the batched Toeplitz-plus-Hankel solve-and-update (dsa_mcep_newton_update).  With a
    graph wanted the same composition runs on differentiable pieces (RowsLogFn, MatmulRowsFn, RowsExpSubFn, ThSolveFn).  Same
    arithmetic order per frame as the reference's formulation; float32 products accumulate in float32."""
    M1 = M + 1
    lead = Xc.shape[:-1]
    X2 = Xc.reshape(-1, Xc.size(-1))
    want_grad = torch.is_grad_enabled() and X2.requires_grad
    if X2.dtype != torch.float32:
        raise _lib.BackendError("mcep (whole-batch composition): float32 only")
    if want_grad:
        logx = RowsLogFn.apply(X2)                                        # mcep.py:203
        mc = MatmulRowsFn.apply(logx, G)                                  # :204-207
    else:
        logx = RowsLogFn.apply(X2)                                        # kept: every step's epilogue reads it
        mc = rows_gemm(logx, G)
    one_launch_resid = _lib.env_int("DSA_MCEP_RESID", 1) != 0 and Xc.size(-1) >= 4
    # round 5: the step's two products as binary16 splits (DSA_MCEP_RESID_H=0: the float32 matrix instructions of round 4, for A/B runs)
    images_h = None
    if not want_grad and 3 <= M1 <= 55 and one_launch_resid and _lib.env_int("DSA_MCEP_RESID_H", 1) != 0 \
            and D.dtype == torch.float32 and E.dtype == torch.float32:
        images_h = mcep_resid_images(D, E)
    if images_h is not None and n_iter >= 1 and mcep_newton_steps_applies(M1) and av.dtype == torch.float32:
        # round 6: every step in one persistent launch (22 launches -> 3 for the analysis)
        out_ = mcep_newton_steps(logx, mc, images_h, av, n_iter)
        if out_ is not None:
            return out_.reshape(*lead, M1)
    if want_grad and n_iter >= 1 and Xc.size(-1) >= 4 and mcep_newton_steps_grad_applies(M1, D, E, av):
        # round 6: the steps as ONE node whose backward is two launches per step (dsa_mcep_newton_update_bwd, dsa_mcep_newton_resid_h_bwd)
        return McepNewtonStepsHFn.apply(logx, mc, D, E, av, n_iter).reshape(*lead, M1)
    for _ in range(n_iter):
        if want_grad:
            e = RowsExpSubFn.apply(logx, MatmulRowsFn.apply(mc, D))       # :210-212
            rt = MatmulRowsFn.apply(e, E)                                 # :214-215
        elif images_h is not None:
            rt = mcep_newton_resid_h(logx, mc.contiguous(), images_h)     # :210-215 in one launch on the binary16 matrix pipe
        elif 3 <= M1 <= 55 and one_launch_resid:
            rt = mcep_newton_resid(logx, mc, D, E)                        # :210-215 in one launch, e never stored
        else:
            e = rows_gemm(mc, D, ROWS_EPI_EXPSUB, aux=logx)               # product and exp(log X - 2 .) in one launch
            rt = rows_gemm(e, E)
        if want_grad and 2 <= M1 <= 55:
            mc = McepNewtonUpdateFn.apply(rt, av, mc)                     # :216-222, one node
        elif want_grad or M1 > 55:
            p = rt[:, :M1].contiguous()
            mc = mc + ThSolveFn.apply(p, rt, p - av)                      # :216-222
        else:
            mc = mcep_newton_update(rt, av, mc)                           # the same in one launch: 16 systems per wave
    return mc.reshape(*lead, M1)


# The tuned mel-cepstral forward can keep every Newton step's (2 M + 1)-entry row of rt behind the iterates a gradient needs anyway:
# the backward then skips its second forward chain (1.56 -> 1.09-1.18 ms per 204 800 frames).  Cost: n_iter F (2 M + 1) floats on top
# of the (n_iter + 1) F (M + 1) of the iterates -- at 204 800 frames and 10 steps 401 MB on top of 225 MB, alive from the forward to
# the backward.  Above this many EXTRA bytes per call the rows are not kept and the backward recomputes them (same gradient to
# rounding; slower); set it to 0 to never keep them, or DSA_MCEP_HIST_RT=0 in the environment.
MCEP_HIST_RT_MAX_BYTES = 4 << 30


def _keep_rt_rows(n_iter, F, M, like):
    return _lib.env_int("DSA_MCEP_HIST_RT", 1) != 0 and n_iter * F * (2 * M + 1) * like.element_size() <= MCEP_HIST_RT_MAX_BYTES


def _mcep_history(n_iter, F, M, like, with_rt):
    """The Newton history a gradient needs: (n_iter + 1, F, M + 1) iterates, followed -- for the tuned kernels (with_rt) -- by the
    (n_iter, F, 2 M + 1) rows of rt that let the backward skip its second forward chain (DSA_ALGO_HIST_HAS_RT).  One flat buffer."""
    n = (n_iter + 1) * F * (M + 1) + (n_iter * F * (2 * M + 1) if with_rt else 0)
    return torch.empty(n, device=like.device, dtype=like.dtype)


_overlapped = [False]


class overlapped_launches:
    """``with ops.overlapped_launches():`` -- the caller alternates consecutive, independent analysis calls between two streams
    (bench.py --streams 2, dist.analyze_chunked_overlap(alternate_streams=True)).  The tuned mel-cepstral forward launches then pack
    their short last round of tiles onto a few workgroups and release every other CU to the next launch, which waits on the other
    stream (DSA_ALGO_OVERLAPPED_LAUNCHES, include/diffsptk_amd.h): 6.25 rounds per 204 800 frames in the steady state instead of
    6.8.  Results are bit-identical either way; a lone launch is slower with it, so it is never the default."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _overlapped[0]
        _overlapped[0] = self.on
        return self

    def __exit__(self, *exc):
        _overlapped[0] = self.prev
        return False


_fixed_steps = [False]


class fixed_newton_steps:
    """``with ops.fixed_newton_steps():`` -- the tuned mel-cepstral forward launches (STFT -> mel-cepstrum in one launch, mcep alone;
    float32, fft_length 512, cep_order 24) run every one of their ``n_iter`` Newton steps (DSA_ALGO_FIXED_STEPS,
    include/diffsptk_amd.h).  By default ``n_iter`` is the LARGEST number of steps: a frame stops at the first step whose update is at
    most 2^-20 max(1, |mc|_inf), which is where float32 steps stop improving it, or at most 2^-16 max(1, |mc|_inf) and a sixteenth of
    the update before it -- the quadratic phase, in which the next update would be below 2^-20 (never at step 1).  The difference between the two is a small
    fraction of the tolerance the results are tested to; inside the context the results are those of the fixed-step kernels bit for
    bit.  Every other kernel family runs exactly ``n_iter`` steps either way."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _fixed_steps[0]
        _fixed_steps[0] = self.on
        return self

    def __exit__(self, *exc):
        _fixed_steps[0] = self.prev
        return False


_full_chains = [False]


class full_precision_chains:
    """``with ops.full_precision_chains():`` -- the tuned mel-cepstral forward launches run every Newton step on three-term binary16
    chains (DSA_ALGO_FULL_CHAINS, include/diffsptk_amd.h; the environment form is DSA_MCEP_FULL_CHAINS=1).  By default step k is coarse
    when k <= clamp(n_iter - 6, 0, 2): one product per chain instead of three, operands good to 2^-11, with at least six full steps
    behind it -- Newton's method removes an early step's rounding error.  Inside the context the results are those of the kernels
    before the coarse steps bit for bit; together with fixed_newton_steps(), those of the fixed-step kernels."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _full_chains[0]
        _full_chains[0] = self.on
        return self

    def __exit__(self, *exc):
        _full_chains[0] = self.prev
        return False


_reserved_cus = [0]


class reserve_cus:
    """``with ops.reserve_cus(n):`` -- the tuned mel-cepstral forward launches (STFT -> mel-cepstrum in one launch, mcep alone) leave
    ``n`` of the 256 CUs free (DSA_ALGO_RESERVE_CUS, include/diffsptk_amd.h).  A persistent workgroup fills its CU, so a kernel of
    another stream -- RCCL's all-gather of the previous batch's features -- otherwise starts only in the launch's tail and the next
    launch queues behind it.  dist.analyze_chunked_overlap sets it in a world of more than one rank.  Same bits; the launch itself
    takes 256 / (256 - n) as long."""

    def __init__(self, n: int):
        self.n = max(0, min(63, int(n)))

    def __enter__(self):
        self.prev = _reserved_cus[0]
        _reserved_cus[0] = self.n
        return self

    def __exit__(self, *exc):
        _reserved_cus[0] = self.prev
        return False


def _mcep_algo(clean: bool) -> int:
    """The algo bits of a tuned mel-cepstral forward launch: DSA_ALGO_SCRATCH_IS_CLEAN with DSA_ALGO_OVERLAPPED_LAUNCHES
    (overlapped_launches()) on the kept-zero scratch, DSA_ALGO_RESERVE_CUS (reserve_cus()), DSA_ALGO_FIXED_STEPS
    (fixed_newton_steps()) and DSA_ALGO_FULL_CHAINS (full_precision_chains())."""
    flag = _lib.algo_reserve_cus(_reserved_cus[0]) | (_lib.ALGO_FIXED_STEPS if _fixed_steps[0] else 0) | (_lib.ALGO_FULL_CHAINS if _full_chains[0] else 0)
    if clean:
        flag |= _lib.ALGO_SCRATCH_IS_CLEAN | (_lib.ALGO_OVERLAPPED_LAUNCHES if _overlapped[0] else 0)
    return flag


def stft_mcep_fusable(x, window, G, L, P, fft_length, M) -> bool:
    """Configurations dsa_stft_mcep_fwd covers (include/diffsptk_amd.h): float32 device tensors, frame_length 400, fft_length 512,
    cep_order 24 (the caller checks power format / constant padding / no zmean / no relative floor)."""
    if not (x.is_cuda and x.dtype == torch.float32 and window.dtype == torch.float32 and G.dtype == torch.float32):
        return False
    T = x.size(-1)
    if T < 1 or T >= 2 ** 31 or L != 400 or fft_length != 512 or M != 24 or P < 1:
        return False
    B = x.numel() // T
    return B * num_frames(T, P) < 2 ** 31


class StftMcepFn(torch.autograd.Function):
    """MelCepstralAnalysis(STFT(x)) in ONE launch (dsa_stft_mcep_fwd; stft.py:237-241 -> mcep.py:189-224): the (B, N, 257) power
    spectrogram is neither written nor re-read -- unless a gradient is wanted: then the same launch also leaves the spectrogram
    and the Newton history behind, and the backward is the two stages' own (dsa_mcep_bwd, then dsa_stft_bwd)."""

    @staticmethod
    def forward(ctx, x, window, twiddle, G, D, E, av, L, P, fft_length, center, eps, M, n_iter, mode="constant", zmean=False,
                relative_floor_db=None):
        _require_device(x, window, twiddle, G, D, E, av)
        _same_dtype(x, window, twiddle, G, D, E, av)
        xc, wc = x.contiguous(), window.contiguous()
        T = xc.size(-1)
        B = xc.numel() // T
        N = num_frames(T, P)
        K = fft_length // 2 + 1
        F = B * N
        need_grad = ctx.needs_input_grad[0]
        mc = torch.empty(*xc.shape[:-1], N, M + 1, device=x.device, dtype=x.dtype)
        with_rt = need_grad and _keep_rt_rows(n_iter, F, M, xc)
        hist = _mcep_history(n_iter, F, M, x, with_rt) if need_grad else None
        X = torch.empty(*xc.shape[:-1], N, K, device=x.device, dtype=x.dtype) if need_grad else None
        images = mcep_images(G, D, E, fft_length, M)
        if images is None:
            raise _lib.BackendError("stft_mcep: no tuned kernel for this configuration (check stft_mcep_fusable first)")
        scratch, clean = _mcep_scratch(x.device)
        flag = _mcep_algo(clean)
        if with_rt:
            flag |= _lib.ALGO_HIST_HAS_RT
        with torch.cuda.device(x.device):
            _call("dsa_stft_mcep_opts_fwd", _p(xc), B, T, L, P, fft_length, _p(wc), _p(twiddle), int(center), int(bool(zmean)),
                  pad_mode_code(mode), float(eps), int(relative_floor_db is not None),
                  0.0 if relative_floor_db is None else float(relative_floor_db), M, n_iter, _p(G), _p(D), _p(E), _p(av), _dtype_code(xc),
                  _lib.ALGO_AUTO | flag, _p(images), _p(scratch), _p(mc), _p(hist), _p(X), _stream())
        if need_grad:
            ctx.save_for_backward(xc, wc, twiddle, X, hist, G, D, E, av)
        ctx.cfg = (L, P, fft_length, center, eps, M, n_iter)
        ctx.mode = mode
        ctx.zmean = bool(zmean)
        ctx.floor_db = relative_floor_db
        ctx.images = images
        ctx.with_rt = with_rt
        return mc

    @staticmethod
    @once_differentiable
    def backward(ctx, gmc):
        xc, wc, twiddle, X, hist, G, D, E, av = ctx.saved_tensors
        L, P, fft_length, center, eps, M, n_iter = ctx.cfg
        gmc = gmc.contiguous()
        K = fft_length // 2 + 1
        F = X.numel() // K
        T = xc.size(-1)
        B = xc.numel() // T
        gX = torch.empty_like(X)
        gx = torch.empty_like(xc)
        scratch = torch.empty(_lib.MCEP_BWD_WORKSPACE_BYTES, dtype=torch.uint8, device=gmc.device)
        with torch.cuda.device(gmc.device):
            _call("dsa_mcep_bwd", _p(gmc), _p(X), _p(hist), F, fft_length, M, n_iter, _p(G), _p(D), _p(E), _p(av),
                  _dtype_code(X), _lib.ALGO_AUTO | _lib.ALGO_SCRATCH_HAS_WORKSPACE | (_lib.ALGO_HIST_HAS_RT if ctx.with_rt else 0),
                  _p(ctx.images), _p(scratch), _p(gX), _stream())
            _call("dsa_stft_bwd", _p(gX), _p(xc), B, T, L, P, fft_length, _p(wc), _p(twiddle), int(center), int(ctx.zmean),
                  pad_mode_code(ctx.mode), float(eps), int(ctx.floor_db is not None), 0.0 if ctx.floor_db is None else float(ctx.floor_db), 3,
                  _dtype_code(xc), _lib.ALGO_AUTO, _p(gx), None, _stream())
        return (gx,) + (None,) * 16


class McepFn(torch.autograd.Function):
    """MelCepstralAnalysis._forward (mcep.py:189-224) with composed linear stages."""

    @staticmethod
    def forward(ctx, X, G, D, E, av, fft_length, M, n_iter, algo):
        _require_device(X, G, D, E, av)
        _same_dtype(X, G, D, E, av)
        Xc = X.contiguous()
        K = fft_length // 2 + 1
        F = Xc.numel() // K
        mc = torch.empty(*Xc.shape[:-1], M + 1, device=X.device, dtype=X.dtype)
        need_hist = ctx.needs_input_grad[0]
        images = mcep_images(G, D, E, fft_length, M) if algo != _lib.ALGO_GENERIC else None
        if images is None and not need_hist and algo != _lib.ALGO_GENERIC and _mcep_composed_applies(Xc, M):
            return _mcep_composed_fwd(Xc, G, D, E, av, M, n_iter)
        # the tuned kernels keep every step's rt row next to the iterates (DSA_ALGO_HIST_HAS_RT): the backward skips a chain
        with_rt = need_hist and images is not None and _keep_rt_rows(n_iter, F, M, Xc)
        hist = _mcep_history(n_iter, F, M, X, with_rt) if need_hist else None
        # the tile queue's counters: a per-(device, stream) scratch that the kernel leaves zeroed (no fill launch per call)
        scratch = None
        flag = 0
        if images is not None:
            scratch, clean = _mcep_scratch(X.device)
            flag = _mcep_algo(clean)
        if with_rt:
            flag |= _lib.ALGO_HIST_HAS_RT
        with torch.cuda.device(X.device):
            _call("dsa_mcep_fwd", _p(Xc), F, fft_length, M, n_iter, _p(G), _p(D), _p(E), _p(av),
                  _dtype_code(Xc), algo | flag, _p(images), _p(scratch), _p(mc), _p(hist), _stream())
        if need_hist:
            ctx.save_for_backward(Xc, hist, G, D, E, av)
        ctx.cfg = (fft_length, M, n_iter, algo)
        ctx.images = images
        ctx.with_rt = with_rt
        return mc

    @staticmethod
    @once_differentiable
    def backward(ctx, gmc):
        Xc, hist, G, D, E, av = ctx.saved_tensors
        fft_length, M, n_iter, algo = ctx.cfg
        gmc = gmc.contiguous()
        K = fft_length // 2 + 1
        F = Xc.numel() // K
        gX = torch.empty_like(Xc)
        images = ctx.images
        # the tuned kernel's scratch with the hand-over area of its split tail (DSA_ALGO_SCRATCH_HAS_WORKSPACE): 1 MB from the
        # caching allocator, stream-ordered
        scratch, flag = None, 0
        if images is not None:
            scratch = torch.empty(_lib.MCEP_BWD_WORKSPACE_BYTES, dtype=torch.uint8, device=gmc.device)
            flag = _lib.ALGO_SCRATCH_HAS_WORKSPACE | (_lib.ALGO_HIST_HAS_RT if ctx.with_rt else 0)
        with torch.cuda.device(gmc.device):
            _call("dsa_mcep_bwd", _p(gmc), _p(Xc), _p(hist), F, fft_length, M, n_iter, _p(G), _p(D), _p(E),
                  _p(av), _dtype_code(Xc), algo | flag, _p(images), _p(scratch), _p(gX), _stream())
        return (gX,) + (None,) * 8
