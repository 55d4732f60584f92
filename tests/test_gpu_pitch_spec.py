"""PitchAdaptiveSpectralAnalysis on the GPU against the reference's goldens (tests/golden/make_golden_pitch_spec.py; the cases and their
inputs: tests/pitch_spec_cases.py) and against the float64 restatement (tests/pitch_spec_ref.py).

Bounds, all relative to max(1, max |ref|).
  float64: 64 max(D_ulp, B_dep, 2^-53) of the case -- D_ulp is what one unit in the last place of every sample does to the reference's
           float64 results, B_dep what the neighbours in the batch do to them (the reference's running sum starts at the batch's widest
           boundary; the kernel's at the frame's own): the margin the route tables give a measured float64 base.
  float32: on the case without noise, the float64 kernel's result within 2^-23 max(1, |value|) element by element: one rounding of a
           float64 result, derived, not measured.  On every case, below the reference's own float32 error E_ref / E_gref.
The floor noise is 2^-52 |randn| for both dtypes, so a float32 call is the float64 call rounded on every case.
Achieved (MI355X): float64 y 0.0005 .. 0.17 and gx 0.017 .. 0.56 of the bound; float32 3e-5 .. 1e-2 of E_ref / E_gref."""
import functools

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import pitch_spec_cases as A
import pitch_spec_ref
from conftest import GOLDEN
from diffsptk_amd import _lib, ops
from diffsptk_amd.modules.spec import device_twiddle

pytestmark = pytest.mark.gpu

API, Z = A.load(GOLDEN)
CASE = {c["name"]: c for c in API["cases"]}
DT = {"float32": torch.float32, "float64": torch.float64}


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def on_gpu(a, dt):
    return torch.as_tensor(np.asarray(a)).to("cuda", DT[dt])


def module_of(name, dt, noise=None, **more):
    """the case's module; `noise`: the (noise1, noise2) its _randn hands out, by shape"""
    args, kw = A.module_args(name)
    m = dsp.PitchAdaptiveSpectralAnalysis(*args, **{**kw, **more}, device="cuda", dtype=DT[dt])
    if noise is not None:
        by_shape = {tuple(t.shape): t for t in noise}
        m._randn = lambda shape: by_shape[tuple(shape)]
    return m


def run(m, x, f0, gy=None):
    """(y, gx, the forward's last kernel); autograd runs the backward on a thread of its own, whose record of the last kernel this
    thread does not see: test_every_launch_names_its_kernel calls those entries itself"""
    x = x.detach().requires_grad_(True)
    y = m(x, f0)
    fwd = _lib.last_kernel()
    if gy is None:
        return y.detach(), None, fwd
    y.backward(gy)
    return y.detach(), x.grad, fwd


def tensors(name, dt):
    x, f0 = A.inputs(name)
    n1, n2 = A.noises(name)
    return tuple(on_gpu(a, dt) for a in (x, f0, n1, n2, A.cotangent(name)))


@functools.lru_cache(maxsize=None)
def result(name, dt):
    x, f0, n1, n2, gy = tensors(name, dt)
    m = module_of(name, dt, noise=(n1, n2))
    return run(m, *A.squeeze(name, x, f0), A.squeeze(name, gy)[0])


def float64_bound(name):
    return 64 * max(CASE[name]["D_ulp"], CASE[name]["B_dep"], 2.0 ** -53)


@pytest.mark.parametrize("name", list(A.CASES))
def test_float64_parity_with_the_reference(name):
    y, gx, kernel = result(name, "float64")
    assert kernel == "pitch_spec_f64"
    bad = []
    for key, got in (("y", y), ("gx", gx)):
        ref = Z[f"{name}_{key}"]
        assert got.shape == ref.shape and got.dtype == torch.float64
        err, lim = rel(got.cpu().numpy(), ref), float64_bound(name)
        print(f"{name} float64 {key}: {err:.3g}, bound {lim:.3g} ({err / lim:.2g} of it)")
        if not err <= lim:
            bad.append((key, err, lim))
    assert not bad, bad


@pytest.mark.parametrize("name", list(A.CASES))
def test_float32_is_never_worse_than_the_references_float32(name):
    y, gx, kernel = result(name, "float32")
    assert kernel == "pitch_spec_f32"
    bad = []
    for key, got, bound in (("y", y, "E_ref"), ("gx", gx, "E_gref")):
        ref = Z[f"{name}_{key}"]
        assert got.shape == ref.shape and got.dtype == torch.float32
        err, lim = rel(got.double().cpu().numpy(), ref), CASE[name][bound]
        print(f"{name} float32 {key}: {err:.3g}, the reference's own {lim:.3g} ({err / lim:.2g} of it)")
        if not err < lim:
            bad.append((key, err, lim))
    assert not bad, bad


@pytest.mark.parametrize("name", ["nonoise", "k16", "ceiling"])
def test_float32_is_the_float64_result_rounded_once(name):
    """the issue's case is the one without noise; the floor noise being 2^-52 |randn| for both dtypes, the cases with noise hold it too"""
    y32, gx32, _ = result(name, "float32")
    y64, gx64, _ = result(name, "float64")
    for key, a, b in (("y", y32, y64), ("gx", gx32, gx64)):
        excess = ((a.double() - b).abs() / b.abs().clamp(min=1.0)).max().item()
        print(f"{name} {key}: float32 off the float64 kernel by {excess:.3g} max(1, |value|), bound {2.0 ** -23:.3g}")
        assert excess <= 2.0 ** -23


@pytest.mark.parametrize("dt", list(DT))
def test_equal_bits_twice_and_alone(dt):
    name = "k16"
    x, f0, n1, n2, gy = tensors(name, dt)
    m = module_of(name, dt, noise=(n1, n2))
    y, gx, _ = run(m, x, f0, gy)
    y2, gx2, _ = run(m, x, f0, gy)
    assert torch.equal(y, y2) and torch.equal(gx, gx2)
    assert torch.equal(y, result(name, dt)[0]) and torch.equal(gx, result(name, dt)[1])
    for b in range(x.shape[0]):   # an utterance alone, given its noise rows: the running sum starts at the frame's own boundary
        m1 = module_of(name, dt, noise=(n1[b:b + 1], n2[b:b + 1]))
        y1, gx1, _ = run(m1, x[b:b + 1], f0[b:b + 1], gy[b:b + 1])
        assert torch.equal(y1[0], y[b]) and torch.equal(gx1[0], gx[b])
        y0, gx0, _ = run(m1, x[b], f0[b], gy[b])   # and as (T,)
        assert y0.shape == y.shape[1:] and torch.equal(y0, y[b]) and torch.equal(gx0, gx[b])


@pytest.mark.parametrize("dt", list(DT))
def test_views_and_leading_dimensions(dt):
    name = "k16"
    x, f0, n1, n2, gy = tensors(name, dt)
    m = module_of(name, dt, noise=(n1, n2))
    y, gx, _ = result(name, dt)
    # storage offset 1 (element-aligned only), a row stride that is not the row length, every second element of a wider f0
    flat = torch.zeros(x.numel() + 1, device="cuda", dtype=DT[dt])
    flat[1:] = x.flatten()
    wide = torch.zeros(x.shape[0], x.shape[1] + 3, device="cuda", dtype=DT[dt])
    wide[:, :x.shape[1]] = x
    fwide = torch.zeros(f0.shape[0], 2 * f0.shape[1], device="cuda", dtype=DT[dt])
    fwide[:, ::2] = f0
    gwide = torch.zeros(*gy.shape[:2], gy.shape[2] + 1, device="cuda", dtype=DT[dt])
    gwide[..., :-1] = gy
    for xv, fv, gv in ((flat[1:].view_as(x), f0, gy), (wide[:, :x.shape[1]], fwide[:, ::2], gwide[..., :-1])):
        assert not xv.is_contiguous() or xv.storage_offset() == 1
        yv, gxv, _ = run(m, xv, fv, gv)
        assert torch.equal(yv, y) and torch.equal(gxv, gx)
    # (2, T) as (2, 1, T): the leading dimensions come back
    y3, gx3, _ = run(m, x[:, None], f0[:, None], gy[:, None])
    assert y3.shape == (2, 1) + y.shape[1:] and torch.equal(y3[:, 0], y) and torch.equal(gx3[:, 0], gx)


@pytest.mark.parametrize("dt", list(DT))
def test_empty_batch(dt):
    m = module_of("k16", dt)
    T, N, K = 960, 12, 513
    xe = torch.zeros(0, T, device="cuda", dtype=DT[dt], requires_grad=True)
    y = m(xe, torch.zeros(0, N, device="cuda", dtype=DT[dt]))
    assert y.shape == (0, N, K)
    y.sum().backward()
    assert xe.grad.shape == (0, T)
    # the entries themselves: a zero count returns before any pointer is looked at
    for B, Nn, Tt in ((0, N, T), (2, 0, 0)):
        ops._call("dsa_pitch_spec", None, None, None, None, None, B, Nn, Tt, 80, 16000, 1024, 500.0, -0.15, 0.0, 0.0, 3, _lib.F32, None, None)
        ops._call("dsa_pitch_spec_vjp_frames", None, None, None, None, None, None, B, Nn, Tt, 80, 16000, 1024, 500.0, -0.15, 0.0, 0.0, 3, _lib.F32,
                  None, None)
        ops._call("dsa_pitch_spec_vjp_gather", None, B, Nn, Tt, 80, 1024, _lib.F32, None, None)


@pytest.mark.parametrize("dt", list(DT))
def test_only_unvoiced_frames(dt):
    """every f0 <= f_min: all frames at default_f0, compared with the restatement at the float64 bound of the case (float32: one rounding
    more)"""
    name = "k16"
    x, f0, n1, n2, gy = tensors(name, dt)
    f0 = torch.full_like(f0, 40.0)
    f0[:, ::3] = 0
    m = module_of(name, dt, noise=(n1, n2))
    y, gx, _ = run(m, x, f0, gy)
    (P, sr, L), _ = A.module_args(name)
    ry, rgx = pitch_spec_ref.pitch_spec(x.cpu().numpy(), f0.cpu().numpy(), P, sr, L, noise1=n1.cpu().numpy(), noise2=n2.cpu().numpy(),
                                        noise_eps=float(np.finfo(np.float64).eps), gy=gy.double().cpu().numpy())
    alone = pitch_spec_ref.pitch_spec(x.cpu().numpy(), np.full(f0.shape, 500.0), P, sr, L, noise1=n1.cpu().numpy(), noise2=n2.cpu().numpy(),
                                      noise_eps=float(np.finfo(np.float64).eps))[0]
    assert np.array_equal(ry, alone)   # the restatement too reads them as 500 Hz
    lim = float64_bound(name) + (2.0 ** -23 if dt == "float32" else 0.0)
    err, gerr = rel(y.double().cpu().numpy(), ry), rel(gx.double().cpu().numpy(), rgx)
    print(f"unvoiced {dt}: y {err:.3g}, gx {gerr:.3g}, bound {lim:.3g}")
    assert torch.isfinite(y).all() and err <= lim and gerr <= lim


def test_a_silent_waveform_with_noise_is_finite():
    """x = 0 exactly: what is analysed is 1e-12 noise1, in dB so that the values are of magnitude 100 and not 1e-25.  Against the
    restatement in float64; the bound is 64 times what one unit in the last place of every noise value does to the restatement, the largest
    of three draws (the measure D_ulp of the goldens, taken on this input), at least 64 2^-53"""
    name, dt = "k16", "float64"
    x, f0, n1, n2, gy = tensors(name, dt)
    x = torch.zeros_like(x)
    y, gx, _ = run(module_of(name, dt, noise=(n1, n2), out_format="db"), x, f0, gy)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all() and (y < -100).all()
    (P, sr, L), _ = A.module_args(name)
    kw = dict(out_format="db", noise2=n2.cpu().numpy(), gy=gy.cpu().numpy())
    ry, rgx = pitch_spec_ref.pitch_spec(x.cpu().numpy(), f0.cpu().numpy(), P, sr, L, noise1=n1.cpu().numpy(), **kw)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(3):
        n1p = n1.cpu().numpy()
        n1p = np.where(rng.integers(0, 2, n1p.shape) == 1, np.nextafter(n1p, np.inf), np.nextafter(n1p, -np.inf))
        py, pgx = pitch_spec_ref.pitch_spec(x.cpu().numpy(), f0.cpu().numpy(), P, sr, L, noise1=n1p, **kw)
        worst = max(worst, rel(py, ry), rel(pgx, rgx))
    lim = 64 * max(worst, 2.0 ** -53)
    err, gerr = rel(y.cpu().numpy(), ry), rel(gx.cpu().numpy(), rgx)
    print(f"silent: y {err:.3g} (max |y| {np.abs(ry).max():.3g}), gx {gerr:.3g} (max |gx| {np.abs(rgx).max():.3g}), bound {lim:.3g}")
    assert err <= lim and gerr <= lim


def test_every_launch_names_its_kernel():
    name = "k16"
    (P, sr, L), _ = A.module_args(name)
    p = ops._p
    for dt, code, routes in (("float32", _lib.F32, ("pitch_spec_f32", "pitch_spec_vjp_frames_f32", "pitch_spec_vjp_gather_f32")),
                             ("float64", _lib.F64, ("pitch_spec_f64", "pitch_spec_vjp_frames_f64", "pitch_spec_vjp_gather_f64"))):
        x, f0, n1, n2, gy = tensors(name, dt)
        (B, T), N, K = x.shape, f0.shape[1], L // 2 + 1
        tw = device_twiddle(L, x.device, torch.float64)
        y = torch.empty(B, N, K, device="cuda", dtype=DT[dt])
        common = (p(x), p(f0), p(n1), p(n2), p(tw), B, N, T, P, sr, L, 500.0, -0.15, 0.0, 0.0, 3, code)
        ops._call("dsa_pitch_spec", *common, p(y), ops._stream())
        assert _lib.last_kernel() == routes[0] and torch.equal(y, result(name, dt)[0])
        gframes = torch.full((B, N, L), float("nan"), device="cuda", dtype=torch.float64)
        ops._call("dsa_pitch_spec_vjp_frames", p(gy), *common, p(gframes), ops._stream())
        assert _lib.last_kernel() == routes[1] and torch.isfinite(gframes).all()
        gx = torch.full((B, T), float("nan"), device="cuda", dtype=DT[dt])
        ops._call("dsa_pitch_spec_vjp_gather", p(gframes), B, N, T, P, L, code, p(gx), ops._stream())
        assert _lib.last_kernel() == routes[2] and torch.equal(gx, result(name, dt)[1])
        # a frame's cotangent is zero outside its window of 2 h + 1 samples
        f = np.where(A.inputs(name)[1] <= 3 * sr / (L - 3), 500.0, A.inputs(name)[1].astype(np.float64))
        h = torch.as_tensor(np.round(1.5 * sr / f)).cuda()[..., None]
        j = (torch.arange(L, device="cuda") - L // 2).abs()
        assert not gframes[j > h].any() and gframes[j <= h].any()


@pytest.mark.parametrize("dt", list(DT))
def test_graphed_capture_replays_to_the_same_bits(dt):
    name = "k16"
    x, f0, n1, n2, _ = tensors(name, dt)
    m = module_of(name, dt, noise=(n1, n2))
    eager = m(x, f0).clone()
    g = dsp.Graphed(lambda a, b: m(a, b), x, f0)   # no host read anywhere, so the capture holds the whole operator
    assert torch.equal(g(x, f0), eager)
    x2 = torch.flip(x, dims=(1,))
    assert torch.equal(g(x2, f0), m(x2, f0)) and not torch.equal(g(x2, f0), eager)


def test_analysis_feeds_synthesis_and_the_gradient_comes_back():
    """x -> (sp, ap) -> waveform on the device, and the gradient of the waveform back to x through both analyses; no numeric claim"""
    name, dt = "k16", "float32"
    (P, sr, L), _ = A.module_args(name)
    x, f0, _, _, _ = tensors(name, dt)
    torch.manual_seed(0)
    x = x.requires_grad_(True)
    sp = dsp.PitchAdaptiveSpectralAnalysis(P, sr, L, device="cuda")(x, f0)
    ap = dsp.Aperiodicity(P, sr, L, device="cuda")(x, f0)
    y = dsp.WorldSynthesis(P, sr, L, device="cuda")(f0, ap, sp)
    assert sp.shape == ap.shape and y.shape == x.shape and torch.isfinite(sp).all() and torch.isfinite(y).all() and y.abs().max() > 0
    gsp, gap = torch.autograd.grad(y.square().sum(), (sp, ap), retain_graph=True)
    via_sp, = torch.autograd.grad(sp, x, gsp, retain_graph=True)
    via_ap, = torch.autograd.grad(ap, x, gap, retain_graph=True)
    y.square().sum().backward()
    for g in (via_sp, via_ap, x.grad):
        assert torch.isfinite(g).all() and g.abs().max() > 0
