"""Aperiodicity on the GPU against the reference's goldens (tests/golden/make_golden_ap.py; the cases and their inputs: tests/ap_cases.py)
and against the float64 restatement (tests/ap_ref.py).

Bounds, all relative to max(1, max |ref|).  float64: 16 max(restatement_deviation, D_ulp) of the case -- D_ulp is what one unit in the
last place of every input does to the reference's float64 results (the 6 x 6 systems are ill-conditioned, so this, not 2^-52, is the
scale of any float64 implementation's error).  float32: 4 E_ref on the value and 4 E_gref on the gradient, the largest of the case's
sample-rate group, E the reference's own float32 error.  Where the reference's float32 run truncated other integers than its float64 run
(same_decisions false), the float32 result is judged against the restatement on the float32 integers: a wrong curr_pos moves a run by a
sample and misses these bounds by orders of magnitude.  Cases outside the goldens take the bounds of their sample-rate group."""
import functools

import numpy as np
import pytest
import torch

import ap_cases as A
import ap_ref
import diffsptk_amd as dsp
from conftest import GOLDEN
from diffsptk_amd import _lib, ops

pytestmark = pytest.mark.gpu

API, Z = A.load(GOLDEN)
CASE = {c["name"]: c for c in API["cases"]}
DT = {"float32": torch.float32, "float64": torch.float64}
NP = {"float32": np.float32, "float64": np.float64}
RUNS = [(n, dt) for n in A.CASES for dt in DT]


def group_bound(sr, dt, key):
    """the bound of a sample-rate group: key 'y' or 'gx'"""
    if dt == "float64":
        return 16 * max(max(c["restatement_deviation"], c["D_ulp"]) for c in CASE.values() if c["sr"] == sr and "D_ulp" in c)
    return 4 * API["groups"][str(sr)]["E_ref" if key == "y" else "E_gref"]


def bound(name, dt, key):
    c = CASE[name]
    if dt == "float64" and "D_ulp" in c:
        return 16 * max(c["restatement_deviation"], c["D_ulp"])
    return group_bound(c["sr"], dt, key)


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def on_gpu(a, dt):
    return torch.as_tensor(np.asarray(a)).to("cuda", DT[dt])


def module_of(name, dt, **more):
    args, kw = A.module_args(name)
    return dsp.Aperiodicity(*args, **{**kw, **more}, device="cuda", dtype=DT[dt])


def run(m, x, f0, gy=None):
    """(y, gx, the forward's last kernel); autograd runs the backward on a thread of its own, whose record of the last kernel this thread
    does not see: test_every_launch_names_its_kernel calls those entries itself"""
    x = x.detach().requires_grad_(True)
    y = m(x, f0)
    fwd = _lib.last_kernel()
    if gy is None:
        return y.detach(), None, fwd
    y.backward(gy)
    return y.detach(), x.grad, fwd


@functools.lru_cache(maxsize=None)
def result(name, dt):
    gy = on_gpu(A.cotangent(name, Z[f"{name}_y"].shape), dt)
    return run(module_of(name, dt), on_gpu(Z[f"{name}_x"], dt), on_gpu(Z[f"{name}_f0"], dt), gy)


@functools.lru_cache(maxsize=None)
def restated(name, dt):
    """the restatement on the integers of `dt`: what the float32 kernels are judged against where the reference's two runs part"""
    (P, sr, L), kw = A.module_args(name)
    kw = dict(kw)
    fmt = A.FORMATS[kw.pop("out_format")]
    return ap_ref.aperiodicity(Z[f"{name}_x"], Z[f"{name}_f0"], P, sr, L, out_format=fmt, gy=A.cotangent(name, Z[f"{name}_y"].shape), dtype=NP[dt], **kw)


@pytest.mark.parametrize("name,dt", RUNS)
def test_parity_with_the_reference(name, dt):
    y, gx, kernel = result(name, dt)
    assert kernel == "ap_tandem_" + ("f32" if dt == "float32" else "f64")
    if name == A.SILENT or (dt == "float32" and not CASE[name]["same_decisions"]):
        ref = dict(zip(("y", "gx"), restated(name, dt)))
    else:
        ref = {"y": Z[f"{name}_y"], "gx": Z[f"{name}_gx"]}
    bad = []
    for key, got in (("y", y), ("gx", gx)):
        assert got.shape == ref[key].shape and got.dtype == DT[dt]
        err, lim = rel(got.double().cpu().numpy(), ref[key]), bound(name, dt, key)
        print(f"{name} {dt} {key}: {err:.3g}, bound {lim:.3g}")
        if not err <= lim:
            bad.append((key, err, lim))
    assert not bad, bad


@pytest.mark.parametrize("dt", list(DT))
def test_the_ties_case_reads_the_references_samples(dt):
    """odd frame_period: curr_pos of the deep bands is an exact integer before the truncation; against the reference's own run of the dtype"""
    name = "ties8k"
    assert CASE[name]["same_decisions"]   # else the float32 goldens would have to be the float32 run's
    y, gx, _ = result(name, dt)
    for key, got in (("y", y), ("gx", gx)):
        err, lim = rel(got.double().cpu().numpy(), Z[f"{name}_{key}"]), bound(name, dt, key)
        print(f"{name} {dt} {key}: {err:.3g}, bound {lim:.3g}")
        assert err <= lim


@pytest.mark.parametrize("dt", list(DT))
def test_the_silent_case_is_finite_and_at_the_lower_bound(dt):
    y, gx, _ = result(A.SILENT, dt)
    nan = torch.as_tensor(np.isnan(Z["silent_y"]))
    assert nan.sum() == CASE[A.SILENT]["reference_nan_y"] > 0
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    assert (y.cpu()[nan] == torch.tensor(0.001, dtype=DT[dt])).all()   # where the reference has NaN from log 0: lower_bound
    got, ref = y.double().cpu().numpy()[~nan.numpy()], Z["silent_y"][~nan.numpy()]
    err, lim = float(np.abs(got - ref).max()), bound(A.SILENT, dt, "y")
    print(f"silent {dt}: the reference's finite bins off by {err:.3g}, bound {lim:.3g}")
    assert err <= lim


@pytest.mark.parametrize("dt", list(DT))
def test_equal_bits_whatever_the_layout(dt):
    name = "batched"
    x, f0 = on_gpu(Z[f"{name}_x"], dt), on_gpu(Z[f"{name}_f0"], dt)
    gy = on_gpu(A.cotangent(name, Z[f"{name}_y"].shape), dt)
    m = module_of(name, dt)
    y, gx, _ = run(m, x, f0, gy)
    y2, gx2, _ = run(m, x, f0, gy)   # a repeat call
    assert torch.equal(y, y2) and torch.equal(gx, gx2)
    for b in range(x.shape[0]):   # a row alone, as (1, T) and as (T,): the escalation is the fit's own, so the batch does not matter
        y1, gx1, _ = run(m, x[b:b + 1], f0[b:b + 1], gy[b:b + 1])
        y0, gx0, _ = run(m, x[b], f0[b], gy[b])
        xe, fe = torch.as_strided(x[b], (1, x.shape[1]), (0, 1)), torch.as_strided(f0[b], (1, f0.shape[1]), (0, 1))
        ye, gxe, _ = run(m, xe, fe, gy[b:b + 1])   # one row whose stride(0) is 0: contiguous all the same, so its stride says nothing
        assert xe.stride(0) == 0 and xe.is_contiguous() and torch.equal(ye[0], y[b]) and torch.equal(gxe[0], gx[b])
        assert y0.shape == y.shape[1:] and gx0.shape == x.shape[1:]
        assert torch.equal(y1[0], y[b]) and torch.equal(gx1[0], gx[b]) and torch.equal(y0, y[b]) and torch.equal(gx0, gx[b])
    # storage offset 1 (element-aligned only) and a row stride that is not the row length
    flat = torch.zeros(x.numel() + 1, device="cuda", dtype=DT[dt])
    flat[1:] = x.flatten()
    wide = torch.zeros(x.shape[0], x.shape[1] + 3, device="cuda", dtype=DT[dt])
    wide[:, :x.shape[1]] = x
    fwide = torch.zeros(f0.shape[0], 2 * f0.shape[1], device="cuda", dtype=DT[dt])
    fwide[:, ::2] = f0
    for xv, fv in ((flat[1:].view_as(x), f0), (wide[:, :x.shape[1]], fwide[:, ::2])):
        assert not xv.is_contiguous() or xv.storage_offset() == 1
        yv, gxv, _ = run(m, xv, fv, gy)
        assert torch.equal(yv, y) and torch.equal(gxv, gx)


@pytest.mark.parametrize("dt", list(DT))
def test_empty_batch_and_no_frames(dt):
    m = module_of("bins16k", dt)
    x = on_gpu(Z["bins16k_x"], dt)
    y = m(x[:0], torch.zeros(0, 12, device="cuda", dtype=DT[dt]))
    assert y.shape == (0, 12, 33)
    xg = x.clone().requires_grad_(True)
    y = m(xg, torch.zeros(1, 0, device="cuda", dtype=DT[dt]))
    assert y.shape == (1, 0, 33)
    y.sum().backward()
    assert xg.grad.shape == x.shape and not xg.grad.any()
    xe = x[:0].clone().requires_grad_(True)
    m(xe, torch.zeros(0, 12, device="cuda", dtype=DT[dt])).sum().backward()
    assert xe.grad.shape == (0, x.shape[1])


def sinusoid(T, sr, dt):
    return (0.5 * torch.sin(2 * torch.pi * 220.0 * torch.arange(T, dtype=torch.float64) / sr)).to(DT[dt])


def test_a_pure_float32_sinusoid_alone_and_beside_a_noisy_neighbour():
    """the input on which the reference's float32 Cholesky fails and its whole batch escalates (three to ten trials); here every fit
    decides for itself, in float64, so the row's bits do not depend on its neighbour, and the values are the restatement's"""
    sr, P, L, N, dt = 48000, 240, 2048, 12, "float32"
    clean = sinusoid(N * P, sr, dt)
    noisy = clean + 0.05 * torch.randn(N * P, generator=torch.Generator().manual_seed(1))
    f0 = torch.full((2, N), 220.0)
    m = dsp.Aperiodicity(P, sr, L, lower_bound=0.0, device="cuda")
    gy = on_gpu(A.cotangent("wide48k", (2, N, L // 2 + 1)), dt)
    y2, gx2, _ = run(m, torch.stack([clean, noisy]).cuda(), f0.cuda(), gy)
    y1, gx1, _ = run(m, clean.cuda()[None], f0[:1].cuda(), gy[:1])
    assert torch.equal(y1[0], y2[0]) and torch.equal(gx1[0], gx2[0])
    detail = {}
    ry = ap_ref.aperiodicity(clean.double().numpy()[None], f0[:1].numpy(), P, sr, L, lower=0.0, dtype=np.float32, detail=detail)
    assert all(f.ok.all() for f in detail["fits"])
    err, lim = rel(y1.double().cpu().numpy(), ry), group_bound(sr, dt, "y")
    print(f"sinusoid float32: {err:.3g}, bound {lim:.3g}; trials of the restatement: {sorted({int(t) for f in detail['fits'] for t in f.trial.ravel()})}")
    assert torch.isfinite(y1).all() and torch.isfinite(gx1).all() and err <= lim


def test_fits_that_escalate_and_recover():
    """A clean float64 sinusoid with eps = 1e-22 (tests/ap_cases.py): R is singular to working precision, the first trials fail and a later
    m factors the fit.  Whether a pivot that is rounding noise comes out positive differs between two correct implementations, so the
    kernel's trial counts are read (ops.ap_trials) and the restatement is held to them: then value and gradient must agree, at 16 times
    what one unit in the last place of x does to the restatement under the same trials."""
    c, dt = A.ESCALATING, "float64"
    x, f0 = A.escalating_inputs()
    n_band = ops.ap_bands(c["sr"])[0]
    gy = A.cotangent("band8k", (1, c["N"], n_band + 1)).astype(np.float64)
    m = dsp.Aperiodicity(c["P"], c["sr"], None, eps=c["eps"], lower_bound=c["lower"], device="cuda", dtype=DT[dt])
    xg, fg, gg = on_gpu(x, dt), on_gpu(f0, dt), on_gpu(gy, dt)
    y, gx, _ = run(m, xg, fg, gg)
    y2, gx2, _ = run(m, xg, fg, gg)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all() and torch.equal(y, y2) and torch.equal(gx, gx2)
    noisy = xg + 0.05 * torch.randn(xg.shape, generator=torch.Generator().manual_seed(3), dtype=DT[dt]).cuda()
    yb, gxb, _ = run(m, torch.cat([noisy, xg]), fg.expand(2, -1), gg.expand(2, -1, -1))
    assert torch.equal(yb[1], y[0]) and torch.equal(gxb[1], gx[0])   # the neighbour's fits take m = 1: not this row's business
    e = m.extractor
    cfg = (e.frame_period, e.sample_rate, e.window_length_ms, e.eps, m.lower_bound, m.upper_bound, m.out_format)
    both = ops.ap_trials(torch.cat([noisy, xg]), fg.expand(2, -1), e.window, e.window_sqrt, cfg).cpu().numpy()
    assert not both[0].any()
    kernel = np.moveaxis(both[1:], -1, 0)   # (n_band, 1, N)
    assert np.array_equal(kernel, np.moveaxis(ops.ap_trials(xg, fg, e.window, e.window_sqrt, cfg).cpu().numpy(), -1, 0))
    detail = {}
    ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], eps=c["eps"], detail=detail)
    own = np.stack([f.trial for f in detail["fits"]])
    print("trials per band, kernel:", [sorted({int(t) for t in b.ravel()}) for b in kernel], "restatement:",
          [sorted({int(t) for t in b.ravel()}) for b in own], f"; equal in {(kernel == own).sum()} of {own.size} fits")
    assert kernel.max() < ap_ref.TRIALS and (kernel > 0).any() and (own > 0).any()
    assert ((kernel == own) & (own > 0)).any()   # fits on which both took the same m > 1
    ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], eps=c["eps"], trials=kernel, detail=detail)
    ok = A.fit_mask(detail["fits"])   # where the kernel's m factors the fit in the restatement's arithmetic too
    # the others get no cotangent (with fft_length None every output position belongs to one fit), so the gradients compare as well
    ry, rgx = ap_ref.aperiodicity(x, f0, c["P"], c["sr"], None, lower=c["lower"], eps=c["eps"], gy=gy * ok, trials=kernel)
    ym, gxm, _ = run(m, xg, fg, on_gpu(gy * ok, dt))
    d_y, d_g = A.escalating_sensitivity(ap_ref, x, f0, gy, kernel)
    err = float(np.abs(ym.cpu().numpy() - ry)[ok].max() / max(1.0, np.abs(ry).max()))
    gerr = rel(gxm.cpu().numpy(), rgx)
    escalated = np.stack([kernel[-1]] + list(kernel[::-1]), -1) > 0
    print(f"held to the kernel's trials {ok.sum()} of {ok.size} values factor in the restatement, {(ok & escalated).sum()} of them at m > 1: "
          f"y off by {err:.3g}, bound {16 * d_y:.3g}; gx off by {gerr:.3g}, bound {16 * d_g:.3g} (max |gx| {np.abs(rgx).max():.3g})")
    assert torch.equal(ym, y) and ok.sum() * 2 > ok.size and (ok & escalated).any() and np.abs(rgx).max() > 0
    assert 0 < d_y and err <= 16 * d_y and 0 < d_g and gerr <= 16 * d_g


@pytest.mark.parametrize("dt", list(DT))
def test_a_fit_that_never_factors_gives_the_upper_bound(dt):
    """NaN samples fail the pivot test at every m: upper_bound, a zero gradient, and the neighbour in the batch is not touched (the
    reference would raise for the whole batch)"""
    name = "band8k"
    x, f0 = np.repeat(Z[f"{name}_x"], 2, axis=0), np.repeat(Z[f"{name}_f0"], 2, axis=0)
    x[1] = np.nan
    gy = on_gpu(np.repeat(A.cotangent(name, Z[f"{name}_y"].shape), 2, axis=0), dt)
    y, gx, _ = run(module_of(name, dt), on_gpu(x, dt), on_gpu(f0, dt), gy)
    y0, gx0, _ = result(name, dt)
    assert (y[1] == torch.tensor(0.999, dtype=DT[dt])).all() and not gx[1].any()
    assert torch.equal(y[0], y0[0]) and torch.equal(gx[0], gx0[0])


@pytest.mark.parametrize("dt", list(DT))
def test_a_few_thousand_frames_twice(dt):
    sr, P, L, B, N = 16000, 80, 64, 4, 1024
    g = torch.Generator().manual_seed(2)
    t = torch.arange(N * P, dtype=torch.float64) / sr
    x = torch.stack([0.4 * torch.sin(2 * torch.pi * (150 + 40 * b) * t) for b in range(B)]) + 0.05 * torch.randn(B, N * P, generator=g, dtype=torch.float64)
    x = (torch.round(x * 4096) / 4096)
    f0 = (150.0 + 40 * torch.arange(B))[:, None] + torch.arange(N)[None, :] % 7 * 0.25
    gy = torch.round(torch.randn(B, N, L // 2 + 1, generator=g) * 256) / 256
    m = dsp.Aperiodicity(P, sr, L, device="cuda", dtype=DT[dt])
    y, gx, _ = run(m, x.to("cuda", DT[dt]), f0.to("cuda", DT[dt]), gy.to("cuda", DT[dt]))
    y2, gx2, _ = run(m, x.to("cuda", DT[dt]), f0.to("cuda", DT[dt]), gy.to("cuda", DT[dt]))
    assert torch.equal(y, y2) and torch.equal(gx, gx2)
    ry, rgx = ap_ref.aperiodicity(x[:1].numpy(), f0[:1].numpy(), P, sr, L, gy=gy[:1].double().numpy(), dtype=NP[dt])   # a row is its own
    frames = [0, N // 2, N - 1]
    err, lim = rel(y[0, frames].double().cpu().numpy(), ry[0, frames]), group_bound(sr, dt, "y")
    gerr, glim = rel(gx[:1].double().cpu().numpy(), rgx), group_bound(sr, dt, "gx")
    print(f"{B} x {N} frames {dt}: first, middle and last frame {err:.3g}, bound {lim:.3g}; gradient of the row {gerr:.3g}, bound {glim:.3g}")
    assert err <= lim and gerr <= glim


@pytest.mark.parametrize("sr,P,wms", [(96000, 480, 30), (48000, 240, None)])
def test_the_largest_workgroups(sr, P, wms):
    """more than 64 KiB of dynamic LDS per workgroup: 96 kHz with the default window (seven waves; the backward holds 116 168 bytes), and
    at 48 kHz the longest window inside DSA_AP_MAX_LDS_BYTES.  float32 against the restatement, at the bound of the 48 kHz group: inside
    the library everything is float64, so what is measured is the rounding of the output"""
    n_band = ops.ap_bands(sr)[0]
    if wms is None:
        wms = max(w for w in range(30, 200) if ops.ap_lds_bytes(sum(ops.ap_bands(sr, w)[2]), n_band) <= _lib.AP_MAX_LDS_BYTES)
    need = ops.ap_lds_bytes(sum(ops.ap_bands(sr, wms)[2]), n_band)
    assert 65536 < need <= _lib.AP_MAX_LDS_BYTES
    N, L, dt = 4, 64, "float32"
    T = max(N * P, ops.ap_min_length(sr))
    rng = np.random.default_rng(11)
    t = np.arange(T) / sr
    x = (np.round((0.4 * np.sin(2 * np.pi * 203 * t) + 0.05 * rng.standard_normal(T)) * 4096) / 4096)[None]
    f0 = np.asarray([[203.0, 0.0, 397.0, 101.0]])
    gy = A.cotangent("wide48k", (1, N, L // 2 + 1))
    m = dsp.Aperiodicity(P, sr, L, window_length_ms=wms, device="cuda")
    y, gx, _ = run(m, on_gpu(x, dt), on_gpu(f0, dt), on_gpu(gy, dt))
    ry, rgx = ap_ref.aperiodicity(x, f0, P, sr, L, window_length_ms=wms, gy=gy, dtype=np.float32)
    err, gerr = rel(y.double().cpu().numpy(), ry), rel(gx.double().cpu().numpy(), rgx)
    print(f"{sr} Hz, window {wms} ms, {need} bytes of LDS: y {err:.3g}, bound {group_bound(48000, dt, 'y'):.3g}; gx {gerr:.3g}, "
          f"bound {group_bound(48000, dt, 'gx'):.3g}")
    assert err <= group_bound(48000, dt, "y") and gerr <= group_bound(48000, dt, "gx")


def test_every_launch_names_its_kernel():
    name = "bins16k"
    n_band, _, seg = ops.ap_bands(16000)
    p = ops._p
    for dt, code, tag in (("float32", _lib.F32, "f32"), ("float64", _lib.F64, "f64")):
        m = module_of(name, dt)
        e = m.extractor
        x, f0 = on_gpu(Z[f"{name}_x"], dt), on_gpu(Z[f"{name}_f0"], dt)
        T, N = x.shape[1], f0.shape[1]
        lens = ops.ap_band_lengths(T, n_band)
        ld = sum(lens)
        hp, lp = (torch.empty(1, lens[0], device="cuda", dtype=torch.float64) for _ in range(2))   # the bands are float64 whatever the dtype
        ops._call("dsa_ap_qmf", p(x), 1, T, T, code, p(hp), lens[0], p(lp), lens[0], ops._stream())
        assert _lib.last_kernel() == "ap_qmf_" + tag
        gx = torch.empty_like(x)
        ops._call("dsa_ap_qmf_vjp", p(hp), lens[0], p(lp), lens[0], 1, T, code, p(gx), T, ops._stream())
        assert _lib.last_kernel() == "ap_qmf_vjp_" + tag and torch.isfinite(gx).all()
        bands = torch.randn(1, ld, device="cuda", dtype=torch.float64)
        y = torch.empty(1, N, 33, device="cuda", dtype=DT[dt])
        common = (p(bands), ld, p(f0), p(e.window), p(e.window_sqrt), e.window.stride(0), p(e.interp_indices), p(e.interp_weights), 1, N, T, 80, 16000,
                  30.0, 33, 1e-5, 0.001, 0.999, 0, code)
        ops._call("dsa_ap_tandem", *common, p(y), ops._stream())
        assert _lib.last_kernel() == "ap_tandem_" + tag and torch.isfinite(y).all()
        gruns = torch.empty(1, N, 3 * (sum(seg) + 2 * n_band), device="cuda", dtype=DT[dt])
        starts = torch.empty(1, N, n_band, _lib.AP_START_WORDS, device="cuda", dtype=torch.int64)
        gbands = torch.empty_like(bands)
        ops._call("dsa_ap_tandem_vjp", p(torch.ones_like(y)), *common, p(gruns), p(starts), p(gbands), ld, ops._stream())
        assert _lib.last_kernel() == "ap_tandem_vjp_" + tag and torch.isfinite(gbands).all() and torch.isfinite(gruns).all()
        cpos = starts[0, :, :, 3]
        assert (cpos[1:] >= cpos[:-1]).all()   # what the gather's bisection rests on


@pytest.mark.parametrize("dt", list(DT))
def test_graphed_capture_replays_to_the_same_bits(dt):
    name = "bins16k"
    m = module_of(name, dt)
    x, f0 = on_gpu(Z[f"{name}_x"], dt), on_gpu(Z[f"{name}_f0"], dt)
    eager = m(x, f0).clone()
    g = dsp.Graphed(lambda a, b: m(a, b), x, f0)   # no host read anywhere, so the capture holds the whole operator
    assert torch.equal(g(x, f0), eager)
    x2 = torch.flip(x, dims=(1,))
    assert torch.equal(g(x2, f0), m(x2, f0)) and not torch.equal(g(x2, f0), eager)


def test_it_feeds_world_synthesis_on_the_device():
    sr, P, L, B, N = 16000, 80, 1024, 2, 12
    x = on_gpu(np.stack([Z["bins16k_x"][0], Z["fmt_a_x"][0]]), "float32")
    f0 = on_gpu(np.stack([Z["bins16k_f0"][0]] * 2), "float32")
    ap = dsp.Aperiodicity(P, sr, L, device="cuda")(x, f0)
    assert ap.shape == (B, N, L // 2 + 1) and torch.isfinite(ap).all() and (ap >= 0.001).all() and (ap <= 0.999).all()
    y = dsp.WorldSynthesis(P, sr, L, device="cuda")(f0, ap, torch.ones_like(ap))
    assert y.shape == (B, N * P) and torch.isfinite(y).all()
