"""Every kernel route of tests/kernel_routes.py::ROUTES on the MI355X: the public call on the case's inputs, the name the launcher
recorded (`_lib.last_kernel()` right after the forward; for a backward route on autograd's thread -- the record is per host thread --
in a hook on the first input, which runs right after the backward entry returned), and the outputs or the input gradients against
the float64 restatement of tests/routes_ref.py evaluated on the same (rounded) inputs, the gradients with a stored Gaussian
cotangent.  The neighbouring shape on the other side of a launcher's condition is a case of the neighbouring route: an edited
condition fails here on the name.  Then the four refusals of csrc/lpc.hip, and both sides of every size ceiling of
tests/kernel_routes.py::CEILINGS: the last accepted shape like any route, the nearest shape past it by its message (or by the route
that runs instead), and after every refusal a synchronisation and a valid call on the same stream.  Each case prints its figures
before it asserts."""
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import diffsptk_amd.functional as DF
from diffsptk_amd import _lib, ops
from diffsptk_amd.modules.spec import device_twiddle
from diffsptk_amd.utils import tables

import kernel_routes as KR
import paramgen_ref
import routes_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f64": torch.float64, "f32": torch.float32}


def on_device(a, like):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=like.device, dtype=like.dtype)


# ------------------------------------------------------------------ the public call of every case: tensors on the device -> output(s)
def call_fwlpc(t, T, L, P, M, eps, center=True, B=2, exact=False):
    return ops.frame_window_lpc(t["x"], t["w"], L, P, M, eps, center, "constant", exact)


def call_fftr(t, len_in, nfft, fmt, F=5):
    y = dsp.RealValuedFastFourierTransform(nfft, fmt, device=DEV, dtype=t["x"].dtype)(t["x"])
    return torch.view_as_real(y) if fmt == 0 else y


def call_stft(t, T, L, P, nfft, eps=1e-9, B=2):
    return ops.StftFn.apply(t["x"], t["w"], device_twiddle(nfft, t["x"].device, t["x"].dtype), L, P, nfft, True, False, "constant", eps, None, 3,
                            _lib.ALGO_AUTO)


def call_fbank(t, nfft, C, use_power, gamma, floor=1e-5, F=7):
    return ops.FbankFn.apply(t["x"], on_device(tables.fbank_matrix(nfft, C, 16000), t["x"]), floor, gamma, use_power)


class FbankBins(torch.autograd.Function):
    """glog(max(s H, floor)) with stock operators forward; backward the entry under test, from the saved output as the fused
    STFT -> filter bank calls it (ops.StftFbankFn.backward)"""

    @staticmethod
    def forward(ctx, s, H, floor, gamma):
        v = torch.clamp(s @ H, min=floor)
        y = torch.log(v) if gamma == 0 else (v ** gamma - 1) / gamma
        ctx.save_for_backward(y, ops.fbank_bins_table(H))
        ctx.cfg = (H.size(0), H.size(1), floor, gamma)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, table = ctx.saved_tensors
        K, C, floor, gamma = ctx.cfg
        gy = gy.contiguous()
        g = torch.empty(*gy.shape[:-1], K, device=gy.device, dtype=gy.dtype)
        ops._call("dsa_fbank_bins_bwd", ops._p(gy), ops._p(y), gy.numel() // C, K, C, ops._p(table), float(floor), float(gamma),
                  ops._dtype_code(gy), ops._p(g), ops._stream())
        return g, None, None, None


def call_fbank_bins(t, nfft, C, gamma, floor=1e-5, F=7):
    return FbankBins.apply(t["s"], on_device(tables.fbank_matrix(nfft, C, 16000), t["s"]), floor, gamma)


def call_plp_tail(t, C, M, n_fft, cf=0.33, lifter=22, F=5):
    return ops.PlpFn.apply(t["y"], t["E"], on_device(tables.plp_table(C, M, n_fft, 16000, 0, None, "htk", lifter), t["y"]), M, n_fft, cf, "ycE")


def call_mcep(t, nfft, M, alpha, n_iter, F=70):
    return dsp.MelCepstralAnalysis(fft_length=nfft, cep_order=M, alpha=alpha, n_iter=n_iter, device=DEV, dtype=t["X"].dtype)(t["X"])


def call_mcep_tuned(t, n_iter, keep_rt=True):
    """keep_rt = False: ops.mcep.MCEP_HIST_RT_MAX_BYTES = 0, the documented way to have the backward recompute the forward's rt rows"""
    keep = ops.mcep.MCEP_HIST_RT_MAX_BYTES
    try:
        ops.mcep.MCEP_HIST_RT_MAX_BYTES = keep if keep_rt else 0
        return call_mcep(t, 512, 24, 0.42, n_iter)
    finally:
        ops.mcep.MCEP_HIST_RT_MAX_BYTES = keep


def call_glogx(t, K, n, n_iter, F):
    images = ops.mcep_resid_bwd_images(t["D"], t["E"])
    assert images is not None
    out = torch.empty(F, K, device=DEV, dtype=t["logx"].dtype)
    ops._call("dsa_mcep_newton_glogx_h", ops._p(t["logx"]), F, K, ops._p(t["mcs"]), n, ops._p(t["grts"]), n_iter, ops._p(images),
              ops._dtype_code(t["logx"]), ops._p(out), ops._stream())
    return out


def call_mgcep_spectra(t, nfft, M, gamma, alpha=0.42, F=9):
    mats = tables.mgcep_matrices(nfft, M, alpha)
    return ops.mgcep_spectra(t["x"], t["b1"], on_device(mats["Cr"], t["x"]), on_device(mats["Ci"], t["x"]), gamma)


def call_mgcep_step(t, nfft, M, gamma, alpha=0.42, F=9):
    images = on_device(tables.mgcep_step_images(nfft, M, alpha), t["x"])
    if not t["x"].requires_grad:
        return ops.mgcep_step(t["x"], t["b1"], images, gamma)
    return ops.MgcepStepFn.apply(t["x"], t["b1"], images, on_device(tables.mgcep_step_bwd_images(nfft, M, alpha), t["x"]), gamma)


def call_fuse_fwlpc(t, T, L, P, M, eps, center=True, B=2, exact=False):
    """fuse(Frame, Window, LPC) without a gradient: the one launch where it takes the geometry, the three modules where it refuses"""
    dt = t["x"].dtype
    fused = dsp.fuse(dsp.Frame(L, P, center=center), dsp.Window(L, device=DEV, dtype=dt), dsp.LPC(L, M, eps=eps, device=DEV, dtype=dt))
    with torch.no_grad():
        y = fused(t["x"])
    assert fused.last_path == "three-stage", fused.last_path
    return y


def call_mfcc(t, nfft, C, M, lifter=22, floor=1e-5, F=7):
    W = tables.dct_matrix(C, 2)[:, :M + 1] * tables.mfcc_lifter(M, lifter)[None, :]
    return ops.MfccFn.apply(t["x"], on_device(tables.fbank_matrix(nfft, C, 16000), t["x"]), on_device(W, t["x"]), floor, 0.0, False)


def call_mcep_generic(t, nfft, M, alpha, n_iter, F=70):
    """the generic kernel pair asked for by name, as MelCepstralAnalysis does it for |alpha| > 0.95"""
    m = dsp.MelCepstralAnalysis(fft_length=nfft, cep_order=M, alpha=alpha, n_iter=n_iter, device=DEV, dtype=t["X"].dtype)
    return ops.McepFn.apply(t["X"], m.G, m.D, m.E, m.alpha_vector, nfft, M, n_iter, _lib.ALGO_GENERIC)


class Gc2gcEntry(torch.autograd.Function):
    """dsa_gc2gc_fwd / dsa_gc2gc_bwd themselves: ops.gc2gc_fused and ops.gc2gc_fn test the transform's size first and hand what the
    entries would refuse to the operator chain, so the entries' own ceilings show only here"""

    @staticmethod
    def forward(ctx, c, m2, g1, g2, n_fft, tw):
        cc = c.contiguous()
        out = torch.empty(*cc.shape[:-1], m2 + 1, device=c.device, dtype=c.dtype)
        ops._call("dsa_gc2gc_fwd", ops._p(cc), cc.numel() // cc.size(-1), cc.size(-1), m2, float(g1), float(g2), n_fft, ops._p(tw), 0,
                  ops._dtype_code(cc), ops._p(out), ops._stream())
        ctx.save_for_backward(cc, tw)
        ctx.cfg = (m2, float(g1), float(g2), n_fft)
        return out

    @staticmethod
    def backward(ctx, g):
        cc, tw = ctx.saved_tensors
        m2, g1, g2, n_fft = ctx.cfg
        gc, gin = g.contiguous(), torch.empty_like(cc)
        ops._call("dsa_gc2gc_bwd", ops._p(cc), ops._p(gc), cc.numel() // cc.size(-1), cc.size(-1), m2, g1, g2, n_fft, ops._p(tw),
                  ops._dtype_code(cc), ops._p(gin), ops._stream())
        return gin, None, None, None, None, None


def call_mlsacheck(t, M, mode, n_fft, F=3, alpha=0.42, thr=4.5):
    kw = {"fast": True} if mode == "fast" else {"fast": False, "mod_type": mode}
    return DF.mlsacheck(t["mc"], alpha=alpha, threshold=thr, n_fft=n_fft, warn_type="ignore", **kw)


CALLS = {
    "fuse_fwlpc": call_fuse_fwlpc,
    "mfcc": call_mfcc,
    "mcep_generic": call_mcep_generic,
    "gc2gc_entry": lambda t, g1, g2, n_fft, m1, m2, F=37: Gc2gcEntry.apply(t["c"], m2, g1, g2, n_fft, device_twiddle(n_fft, t["c"].device, t["c"].dtype)),
    "mlsacheck": call_mlsacheck,
    "acorr": lambda t, L, M, fmt, F=3: dsp.Autocorrelation(L, M, fmt)(t["x"]),
    "levdur": lambda t, M, eps, F=5: dsp.LevinsonDurbin(M, eps)(t["r"]),
    "lpc": lambda t, L, M, eps, F=3: dsp.LPC(L, M, eps)(t["x"]),
    "fwlpc": call_fwlpc,
    "zerodf": lambda t, M, P, z0, ig, N, B=2: ops.ZerodfFn.apply(t["x"], t["b"], P, z0, ig),
    "fftr": call_fftr,
    "spec": lambda t, lb, la, nfft, eps, floor, fmt, F=5: dsp.Spectrum(nfft, eps=eps, relative_floor=floor, out_format=fmt)(t.get("b"), t.get("a")),
    "stft": call_stft,
    "irfft_scale": lambda t, nfft, F=5: ops.stft._irfft_scale(t["y"], nfft),
    "thsolve": lambda t, n, F=37: ops.ThSolveFn.apply(t["p"], t["q"], t["r"]),
    "freqt": lambda t, L1, L2, F=5: ops.MatmulRowsFn.apply(t["c"], t["A"]),
    "rows_log": lambda t, n: ops.RowsLogFn.apply(t["x"]),
    "rows_expsub": lambda t, n: ops.RowsExpSubFn.apply(t["a"], t["b"]),
    "fftcep": lambda t, nfft, M, accel, n_iter, F=5: dsp.CepstralAnalysis(fft_length=nfft, cep_order=M, accel=accel, n_iter=n_iter, device=DEV,
                                                                          dtype=t["x"].dtype)(t["x"]),
    "fbank": call_fbank,
    "fbank_bins": call_fbank_bins,
    "pqmf": lambda t, K, M, T, P=1, s=0, B=2: ops.PqmfFn.apply(t["x"], t["f"], P, s),
    "ipqmf": lambda t, K, M, T, U=1, s=0, B=2: ops.IpqmfFn.apply(t["y"], t["f"], U, s),
    "interpolate": lambda t, T, P, s: ops.InterpolateFn.apply(t["x"], P, s, 1),
    "delta": lambda t, T, D, seed, B=2: dsp.Delta(paramgen_ref.SEEDS[seed], True, device=DEV, dtype=t["x"].dtype)(t["x"]),
    "mlpg": lambda t, T, D, seed, B=2: dsp.MLPG(T, paramgen_ref.SEEDS[seed], device=DEV, dtype=t["u"].dtype)(t["u"]),
    "plp_tail": call_plp_tail,
    "poledf": lambda t, M, P, N, ig, B=2: ops.PoledfFn.apply(t["x"], t["a"], P, ig),
    "mcep": call_mcep,
    "mcep_tuned": call_mcep_tuned,
    "newton_update": lambda t, n, F=65: ops.McepNewtonUpdateFn.apply(t["rt"], t["av"], t["mc"]),
    "glogx": call_glogx,
    "gc2gc": lambda t, g1, g2, n_fft, m1, m2, F=37: ops.gc2gc_fn(t["c"], m2, g1, g2, n_fft, device_twiddle(n_fft, t["c"].device, t["c"].dtype)),
    "mgcep_spectra": call_mgcep_spectra,
    "mgcep_step": call_mgcep_step,
    "mgcep_gain": lambda t, M, gamma, F=9: ops.mgcep_gain(t["r"], t["b_eps"], gamma, t["b_join"]),
    "mdct": lambda t, L, T, B=2: dsp.MDCT(L, "sine", device=DEV, dtype=t["x"].dtype)(t["x"]),
    "imdct": lambda t, L, N, B=2: dsp.IMDCT(L, "sine", device=DEV, dtype=t["y"].dtype)(t["y"], (N - 1) * (L // 2)),
}


def run(c, dt):
    """(route name, tensors to compare) of case c in dtype dt on the device"""
    given = R.inputs_of(c, DT[dt])
    t = {k: v.to(DEV).requires_grad_(k in c["wrt"]) for k, v in given.items()}
    names = []
    if c["when"] == "bwd":
        t[c["wrt"][0]].register_hook(lambda g: names.append(_lib.last_kernel()))
    out = CALLS[c["call"]](t, **c["args"])
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    if c["when"] == "fwd":
        return _lib.last_kernel(), given, [o.detach().cpu() for o in outs]
    sum((o * g.to(DEV)).sum() for o, g in zip(outs, R.cotangents(outs, DT[dt]))).backward()
    return names[0], given, [t[k].grad.cpu() for k in c["wrt"]]


CASES = [pytest.param(route, c, dt, id=KR.case_id(route, c) + "-" + dt) for route, cases in KR.ROUTES.items() for c in cases for dt in c["dtypes"]]


_REFS = {}


def reference(route, c, dt, given):
    """the float64 restatement of a case on its rounded inputs: computed once, shared by the tests that need it, never modified"""
    key = KR.case_id(route, c) + "-" + dt
    if key not in _REFS:
        _REFS[key] = R.evaluate(c, {k: v.double() for k, v in given.items()})
    return _REFS[key]


def check_route(route, c, dt):
    """name, shape, finiteness, bound"""
    name, given, got = run(c, dt)
    ref = reference(route, c, dt, given)
    tol = KR.tolerance(route, c, dt)
    errs = [R.error(g, r, c["metric"]) for g, r in zip(got, ref)]
    print(f"{KR.case_id(route, c)} {dt}: kernel {name}, errors {['%.2e' % e for e in errs]}, bound {tol:.2e} ({c['tol_from']})")
    assert name == route, (name, route)
    assert len(got) == len(ref) and all(g.shape == r.shape for g, r in zip(got, ref))
    assert all(torch.isfinite(g).all() for g in got)
    assert max(errs) <= tol, (errs, tol)


@pytest.mark.parametrize("route,c,dt", CASES)
def test_route_runs_and_matches_float64(route, c, dt):
    check_route(route, c, dt)


# ------------------------------------------------------------------ the refusals of csrc/lpc.hip
VALID = ("levdur_bwd", KR.case("levdur", "bwd", wrt=("r",), M=24, eps=1e-5))   # (a case of ROUTES["levdur_bwd"]: its bound is the table's)


def check_refusal(c, dt, text, then):
    """A geometry past a launcher's ceiling raises the library's error with the launcher's message -- nothing about the output or the
    gradient buffer is required --, the device is still in order (synchronize() succeeds), and the valid call `then` = (route, case)
    that follows on the same stream runs its route and meets its bound."""
    given = R.inputs_of(c, DT[dt])
    t = {k: v.to(DEV).requires_grad_(k in c["wrt"]) for k, v in given.items()}
    if c["when"] == "fwd":
        with pytest.raises(_lib.BackendError, match=re.escape(text)):
            CALLS[c["call"]](t, **c["args"])
    else:
        out = CALLS[c["call"]](t, **c["args"])          # (the forward of this shape is supported: that is the point)
        outs = list(out) if isinstance(out, (tuple, list)) else [out]
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        with pytest.raises(RuntimeError, match=re.escape(text)):
            sum(o.sum() for o in outs).backward()
    torch.cuda.synchronize()
    check_route(then[0], then[1], dt if dt in then[1]["dtypes"] else then[1]["dtypes"][0])


@pytest.mark.parametrize("call,args,dt,when,message", KR.REFUSALS, ids=[f"{r[0]}-{r[3]}-{r[2]}" for r in KR.REFUSALS])
def test_refusal_raises_and_the_next_call_is_right(call, args, dt, when, message):
    check_refusal(KR.shape(call, when, (dt,), wrt=("r",) if when == "bwd" else (), **args), dt, message, VALID)


# ------------------------------------------------------------------ the size ceilings: the last shape in, the first shape out
def _then(row):
    """the valid call that follows a row's refusals: the row's smallest accepted case (its first), else the one of the lpc refusals"""
    return row["inside"][0] if row["inside"] else VALID


INSIDE = [pytest.param(route, c, dt, id=KR.case_id(route, c) + "-" + dt) for row in KR.CEILINGS for route, c in row["inside"] for dt in c["dtypes"]]
OUTSIDE = [(row, o, dt) for row in KR.CEILINGS if row["outside"] != KR.IN_REFUSALS for o in row["outside"] for dt in o["case"]["dtypes"]]
RESHAPED = [pytest.param(o["route"], o["case"], dt, id=KR.case_id(o["route"], o["case"]) + "-" + dt) for row, o, dt in OUTSIDE if o["expect"] == "route"]
REFUSED = [pytest.param(o["case"], dt, o["text"], _then(row), id=KR.case_id("refused", o["case"]) + "-" + dt) for row, o, dt in OUTSIDE if o["expect"] == "raises"]


@pytest.mark.parametrize("route,c,dt", INSIDE)
def test_last_accepted_shape_runs_and_matches_float64(route, c, dt):
    check_route(route, c, dt)


@pytest.mark.parametrize("route,c,dt", RESHAPED)
def test_first_reshaped_launch_runs_its_route_and_matches_float64(route, c, dt):
    check_route(route, c, dt)


@pytest.mark.parametrize("c,dt,text,then", REFUSED)
def test_first_refused_shape_raises_and_the_next_call_is_right(c, dt, text, then):
    check_refusal(c, dt, text, then)
