"""Yingram on the GPU (csrc/yingram.hip) against the goldens of the reference (tests/golden/yingram.npz, make_golden_yingram.py) and the
float64 restatement tests/yingram_ref.py, which tests/test_yingram_cpu.py pins to the same goldens.

Bounds.  float64: 16 times the largest deviation of the restatement from the reference's float64 that the generator recorded, relative
to max(1, max |ref|).  float32: 4 E_ref for y and 4 E_gref for the gradient, E the reference's own float32 error, the larger of the
cases that share the frame length.  Every test prints its worst figure beside its bound before it asserts."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import yingram_ref as R
from conftest import GOLDEN
from diffsptk_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
API, CASES = R.golden_cases(GOLDEN)
F64_BOUND = 16 * API["restatement_deviation"]
DTYPES = {"f64": torch.float64, "f32": torch.float32}
ALGOS = {"direct": _lib.ALGO_GENERIC, "fft": _lib.ALGO_TUNED}
GRID_CASES = [c for c in CASES if c["kind"] in ("noise", "voiced")]
E_REF = {L: max(c["E_ref"] for c in GRID_CASES if c["L"] == L) for L in {c["L"] for c in GRID_CASES}}
E_GREF = {L: max(c["E_gref"] for c in GRID_CASES if c["L"] == L) for L in {c["L"] for c in GRID_CASES}}


def dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().double().cpu().numpy()


def module(c, dtype, route=None):
    m = dsp.Yingram(c["L"], device=DEV, dtype=dtype, **R.options(c))
    if route is not None:
        m.algo = ALGOS[route]
    return m


def bounds(c, dt, y_ref, g_ref):
    if dt == "f64":
        return F64_BOUND * max(1.0, float(np.abs(y_ref).max())), F64_BOUND * max(1.0, float(np.abs(g_ref).max()))
    return 4 * E_REF[c["L"]], 4 * E_GREF[c["L"]]


def b64(want):
    return F64_BOUND * max(1.0, float(np.abs(want).max()))


def run(m, x, gy):
    """(y, gx, the kernel of the forward, the kernel of the backward as a hook on x's gradient saw it)"""
    x = x.clone().requires_grad_(True)
    seen = []
    x.register_hook(lambda g: seen.append(_lib.last_kernel()))
    y = m(x)
    fwd = _lib.last_kernel()
    y.backward(gy)
    return y.detach(), x.grad, fwd, seen[0]


# ------------------------------------------------------------------ the goldens, every case in both precisions on both routes
@pytest.mark.parametrize("route", ["direct", "fft"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_golden_parity_and_routes(dt, route):
    worst, bad = [0.0, 0.0], []
    for c in GRID_CASES:
        m = module(c, DTYPES[dt], route)
        y, gx, fwd, bwd = run(m, dev(c["x"], DTYPES[dt]), dev(c["gy"], DTYPES[dt]))
        if (fwd, bwd) != (f"yingram_{route}_{dt}", f"yingram_vjp_{route}_{dt}"):
            bad.append((c["name"], "kernels", fwd, bwd))
        by, bg = bounds(c, dt, c["y"], c["gx"])
        ey, eg = float(np.abs(host(y) - c["y"]).max()), float(np.abs(host(gx) - c["gx"]).max())
        print(f"{c['name']} {dt} {route}: y {ey:.3g} / {by:.3g}, gradient {eg:.3g} / {bg:.3g}")
        worst = [max(worst[0], ey / by), max(worst[1], eg / bg)]
        if not (ey <= by and eg <= bg):
            bad.append((c["name"], ey, by, eg, bg))
        assert y.shape == (c["F"], c["M"]) and y.dtype == DTYPES[dt] and gx.shape == (c["F"], c["L"])
    print(f"worst share of the bound, {dt} {route}: y {worst[0]:.3g}, gradient {worst[1]:.3g}")
    assert not bad, bad


def small(L, dtype=torch.float64, **kw):
    o = dict(sample_rate=16000, lag_min=22, lag_max=60, n_bin=2)
    o.update(kw)
    return dsp.Yingram(L, device=DEV, dtype=dtype, **o), o


def test_auto_switches_at_the_constant():
    at = _lib.YINGRAM_FFT_MIN_FRAME_LENGTH
    g = torch.Generator().manual_seed(1)
    for L, route in ((at - 1, "direct"), (at, "fft")):
        m, o = small(L, lag_max=min(60, L - 2))
        assert m.algo == _lib.ALGO_AUTO
        x = torch.randn(3, L, generator=g, dtype=torch.float64)
        y, gx, fwd, bwd = run(m, x.to(DEV), torch.ones(3, len(m.lags), dtype=torch.float64, device=DEV))
        print(f"L = {L}: {fwd}, {bwd} (the switch: {at})")
        assert (fwd, bwd) == (f"yingram_{route}_f64", f"yingram_vjp_{route}_f64")
        lags, floor, ceil, K = R.tables(L, **o)
        want = R.forward(x.numpy(), host(m.lags), floor, ceil, K)
        err = float(np.abs(host(y) - want).max())
        print(f"against the restatement: {err:.3g} / {b64(want):.3g}")
        assert err <= b64(want)


@pytest.mark.parametrize("route", ["direct", "fft"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_leading_shapes_offsets_strides_and_repeats_give_the_same_bits(dt, route):
    L = 65
    m, _ = small(L, DTYPES[dt])
    m.algo = ALGOS[route]
    g = torch.Generator().manual_seed(2)
    flat = torch.randn(6, L, generator=g, dtype=DTYPES[dt]).to(DEV)
    gy = torch.randn(6, len(m.lags), generator=g, dtype=DTYPES[dt]).to(DEV)
    y, gx, _, _ = run(m, flat, gy)
    y3, gx3, _, _ = run(m, flat.reshape(2, 3, L), gy.reshape(2, 3, -1))
    assert y3.shape == (2, 3, len(m.lags)) and torch.equal(y3.reshape(6, -1), y) and torch.equal(gx3.reshape(6, L), gx)
    y1, gx1, _, _ = run(m, flat[4], gy[4])
    assert y1.shape == (len(m.lags),) and torch.equal(y1, y[4]) and torch.equal(gx1, gx[4])
    store = torch.zeros(6 * L + 1, dtype=DTYPES[dt], device=DEV)   # one element past the allocation's alignment
    store[1:] = flat.reshape(-1)
    off = store[1:].view(6, L)
    assert off.storage_offset() == 1 and off.is_contiguous()
    yo, gxo, _, _ = run(m, off, gy)
    assert torch.equal(yo, y) and torch.equal(gxo, gx)
    wide = torch.zeros(6, L + 3, dtype=DTYPES[dt], device=DEV)      # rows a stride apart
    wide[:, :L] = flat
    ys, gxs, _, _ = run(m, wide[:, :L], gy)
    assert not wide[:, :L].is_contiguous() and torch.equal(ys, y) and torch.equal(gxs, gx)
    again, gagain, _, _ = run(m, flat, gy)
    assert torch.equal(again, y) and torch.equal(gagain, gx)
    print(f"{dt} {route}: (2, 3, L), (L,), storage offset 1, row stride {L + 3} and a second call: equal bits")


@pytest.mark.parametrize("route", ["direct", "fft"])
def test_grid_limits(route):
    c = next(c for c in CASES if c["name"] == "L32_noise")
    m = module(c, torch.float64, route)
    empty = torch.zeros(0, 32, dtype=torch.float64, device=DEV, requires_grad=True)
    y = m(empty)
    y.sum().backward()
    assert y.shape == (0, c["M"]) and empty.grad.shape == (0, 32)
    F = 65537
    x = torch.randn(F, 32, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    y = m(x.to(DEV))
    rows = [0, F // 2, F - 1]
    z = R.golden_tables(GOLDEN, str(c["table"]))
    want = R.forward(x[rows].numpy(), z["lags64"], z["floor"], z["ceil"], c["K"])
    err = float(np.abs(host(y[rows]) - want).max())
    print(f"F = {F} {route}: rows {rows} {err:.3g} / {b64(want):.3g}")
    assert y.shape == (F, c["M"]) and err <= b64(want) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("route", ["direct", "fft"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_silence_is_exactly_zero(dt, route):
    c = next(c for c in CASES if c["name"] == "silent")
    y, gx, _, _ = run(module(c, DTYPES[dt], route), dev(c["x"], DTYPES[dt]), dev(c["gy"], DTYPES[dt]))
    print(f"silence {dt} {route}: max |y| {float(y.abs().max())}, max |gradient| {float(gx.abs().max())}")
    assert not bool(y.any()) and bool(torch.isfinite(gx).all())


@pytest.mark.parametrize("route", ["direct", "fft"])
def test_an_integral_lag_returns_the_limit(route):
    o = dict(R.INTEGRAL)
    L = o.pop("L")
    m = dsp.Yingram(L, device=DEV, dtype=torch.float64, **o)
    m.algo = ALGOS[route]
    lags, floor, ceil, K = R.tables(L, **o)
    assert (floor == ceil).any()
    g = np.random.default_rng(4)
    x, gy = g.normal(size=(3, L)), g.normal(size=(3, len(lags)))
    y, gx, _, _ = run(m, dev(x), dev(gy))
    weight = host(m.lags) - floor
    want_y = R.forward(x, lags, floor, ceil, K, weight)
    ey = float(np.abs(host(y) - want_y).max())
    want = R.gradient(x, gy, lags, floor, ceil, K, weight)
    eg = float(np.abs(host(gx) - want).max())
    by, bg = b64(want_y), b64(want)
    print(f"integral lag {route}: y {ey:.3g} / {by:.3g}, gradient {eg:.3g} / {bg:.3g}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all()) and ey <= by and eg <= bg


# ------------------------------------------------------------------ fuse(frame, yingram)
@pytest.mark.parametrize("route", ["direct", "fft"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_fused_equals_the_two_modules(dt, route):
    for c in (c for c in CASES if c["kind"] == "fused"):
        P, center = c["frame"]
        m = module(c, DTYPES[dt], route)
        frame = dsp.Frame(c["L"], P, center=center)
        fused = dsp.fuse(frame, m)
        x, gy = dev(c["x"], DTYPES[dt]), dev(c["gy"], DTYPES[dt])
        y, gx, fwd, _ = run(fused, x, gy)
        y2, gx2, fwd2, _ = run(lambda t: m(frame(t)), x, gy)
        assert fused.last_path == "fused" and (fwd, fwd2) == (f"frame_yingram_{route}_{dt}", f"yingram_{route}_{dt}")
        assert torch.equal(y, y2), "the fused forward differs from yingram(frame(x))"
        by, bg = bounds(c, dt, c["y"], c["gx"])
        ey, eg, ec = float(np.abs(host(y) - c["y"]).max()), float(np.abs(host(gx) - c["gx"]).max()), float((gx - gx2).abs().max())
        print(f"{c['name']} {dt} {route}: y {ey:.3g} / {by:.3g}, gradient {eg:.3g} / {bg:.3g}, against the composed gradient {ec:.3g} / {bg:.3g}")
        assert ey <= by and eg <= bg and ec <= bg
        # batched waveforms: the frames of every utterance
        xb = torch.stack([x, x.flip(0)])
        assert torch.equal(fused(xb), m(frame(xb)))
        for other in (dsp.Frame(c["L"], P, center=center, mode="reflect"), dsp.Frame(c["L"], P, center=center, zmean=True)):
            two = dsp.fuse(other, m)   # what the one launch does not cover runs the two modules
            assert torch.equal(two(x), m(other(x))) and two.last_path == "two-stage"


# ------------------------------------------------------------------ workgroups of several waves: a few thousand long frames
@pytest.mark.parametrize("route", ["direct", "fft"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_many_long_frames_repeat_bit_for_bit_and_match_the_restatement(dt, route):
    """L = 2048: eight waves per workgroup on the fft route, and enough frames that the waves of a workgroup do not run in step -- a
    missing barrier shows as bits that change between two calls.  Rows first, middle and last against the restatement."""
    c = next(c for c in CASES if c["name"] == "L2048_noise")
    m = module(c, DTYPES[dt], route)
    F = 3072
    g = torch.Generator().manual_seed(6)
    xq = torch.randint(-4096, 4097, (F, c["L"]), generator=g).to(DTYPES[dt]) / 4096   # exact in float32
    gq = torch.randint(-4096, 4097, (F, c["M"]), generator=g).to(DTYPES[dt]) / 4096
    y, gx, _, _ = run(m, xq.to(DEV), gq.to(DEV))
    y2, gx2, _, _ = run(m, xq.to(DEV), gq.to(DEV))
    same = bool(torch.equal(y, y2)) and bool(torch.equal(gx, gx2))
    rows = [0, F // 2, F - 1]
    z = R.golden_tables(GOLDEN, str(c["table"]))
    weight = host(m.lags) - z["floor"]
    args = (z["lags64"], z["floor"], z["ceil"], c["K"], weight)
    want_y, want_g = R.forward(xq[rows].double().numpy(), *args), R.gradient(xq[rows].double().numpy(), gq[rows].double().numpy(), *args)
    by, bg = (b64(want_y), b64(want_g)) if dt == "f64" else bounds(c, dt, want_y, want_g)
    ey, eg = float(np.abs(host(y[rows]) - want_y).max()), float(np.abs(host(gx[rows]) - want_g).max())
    print(f"L = 2048, F = {F} {dt} {route}: equal bits {same}; rows {rows}: y {ey:.3g} / {by:.3g}, gradient {eg:.3g} / {bg:.3g}")
    assert same and ey <= by and eg <= bg and bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
