"""The three entries of csrc/pitch_spec.hip called directly, where the module's cases (tests/test_gpu_pitch_spec.py: fft_length >= 1024,
F0 <= 1.52 kHz, T >= 84) do not go.

The gather, bit for bit.  dsa_pitch_spec_vjp_gather sums what it is given, so the frames' cotangents are integers in [-8, 8] in EVERY
column (column 0 and the columns outside any window included), gx is pre-filled with NaN, and the expected value is the clipped
scatter-add np.add.at(out, clip(n P + arange(L) - L / 2, 0, T - 1), g[n]).  All sums are integers far below 2^24: exact in any order, in
float64 and in float32, so the comparison is torch.equal.  T = 1 is the case DSA_VERSION 147 had wrong (the columns behind the middle of
the one frame were dropped: every T = 1 row below fails on it).

The frames kernels below 1024 points and up to Nyquist (the cases: tests/pitch_spec_cases.py, EDGE_CASES; tests/test_pitch_spec_cpu.py
holds their margins and caps the bounds at 1e-10).  Bounds, relative to max(1, max |ref|) (the frames' cotangents: row by row):
  float64: 64 max(D_ulp, 2^-53) against the restatement (tests/pitch_spec_ref.py); D_ulp is what one unit in the last place of every
           sample does to the restatement's y and gx (three draws), for gframes the same measure on the per-frame cotangents.
  float32: the float64 kernel's y and gx rounded once, within 2^-23 max(1, |value|) element by element.
Achieved (MI355X): float64 y 4.5e-5 .. 0.018, gframes 0.0009 .. 0.049 and gx 0.0002 .. 0.037 of the bound; float32 within
5.9e-8 max(1, |value|) of the float64 kernel."""
import functools

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import pitch_spec_cases as A
import pitch_spec_ref
from diffsptk_amd import _lib, ops
from diffsptk_amd.modules.spec import device_twiddle

pytestmark = pytest.mark.gpu

DT = {"float32": (torch.float32, _lib.F32), "float64": (torch.float64, _lib.F64)}
SMALL_P = (1, 3, 8, 9, 17, 40)
SMALL_T = tuple(range(1, 41)) + (255, 256, 257, 258, 513)
WIDE = ((80, 1), (80, 2), (80, 400), (600, 1300), (2000, 4100))


def frames_of(T, P):
    return (T - 1) // P + 1


def integers(seed, *shape):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float64)


def scatter_add(g, P, T):
    """g:(B, N, L) -> (B, T): every column of every frame added to the sample the replicate padding clamps it to"""
    B, N, L = g.shape
    out = np.zeros((B, T))
    for b in range(B):
        for n in range(N):
            np.add.at(out[b], np.clip(n * P + np.arange(L) - L // 2, 0, T - 1), g[b, n])
    return out


def gather(gframes, P, T, dt):
    """dsa_pitch_spec_vjp_gather on gframes:(B, N, L) float64 on the device -> (gx:(B, T) of dt, pre-filled with NaN; the route)"""
    B, N, L = gframes.shape
    assert gframes.dtype == torch.float64 and gframes.is_contiguous() and N == frames_of(T, P)
    gx = torch.full((B, T), float("nan"), device="cuda", dtype=DT[dt][0])
    ops._call("dsa_pitch_spec_vjp_gather", ops._p(gframes), B, N, T, P, L, DT[dt][1], ops._p(gx), ops._stream())
    return gx, _lib.last_kernel()


def check_gather(L, P, T, dt, seed):
    g = integers(seed, 2, frames_of(T, P), L)
    gx, route = gather(torch.as_tensor(g).cuda(), P, T, dt)
    want = torch.as_tensor(scatter_add(g, P, T)).to(DT[dt][0])
    assert route == "pitch_spec_vjp_gather_" + ("f64" if dt == "float64" else "f32")
    return torch.equal(gx.cpu(), want), gx.cpu(), want


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("P", SMALL_P)
def test_gather_is_the_clipped_scatter_add_at_16_points(P, dt):
    """L = 16, B = 2: T = 1 and 2, T below, at and above L / 2, P below, at and above L / 2 and above L (the frames do not overlap and an
    interior sample has no frame: n0 > n1), both sides of the 256-sample block"""
    bad = []
    for T in SMALL_T:
        ok, got, want = check_gather(16, P, T, dt, 100 * P + T)
        if not ok:
            at = (got != want).nonzero()[0].tolist()   # (NaN != anything: an unwritten element shows here)
            bad.append(f"T = {T}: gx[{at[0]}, {at[1]}] = {got[at[0], at[1]].item()}, the scatter-add gives {want[at[0], at[1]].item()}")
    assert not bad, f"L = 16, P = {P}, {dt}: " + "; ".join(bad)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("P,T", WIDE)
def test_gather_is_the_clipped_scatter_add_at_1024_points(P, T, dt):
    ok, got, want = check_gather(1024, P, T, dt, 7 * P + T)
    assert ok, f"L = 1024, P = {P}, T = {T}, {dt}: {int((got != want).sum())} of {want.numel()} elements differ; gx[0, 0] = {got[0, 0].item()}, " \
               f"the scatter-add gives {want[0, 0].item()}"


@pytest.mark.parametrize("dt", list(DT))
def test_gather_at_the_largest_batch(dt):
    """B = 65535, the grid's y: utterance b carries the integers of row b % 251, so gx[b] is gx[b % 251] and that row's scatter-add
    (65536 is refused by message: tests/test_pitch_spec_cpu.py::test_the_two_ceilings)"""
    B, L, P, T = 65535, 16, 2, 5
    rows = integers(65535, 251, frames_of(T, P), L)
    g = torch.as_tensor(rows).cuda()[torch.arange(B, device="cuda") % 251].contiguous()
    gx, _ = gather(g, P, T, dt)
    want = torch.as_tensor(scatter_add(rows, P, T)).to(DT[dt][0]).cuda()
    assert torch.equal(gx[:251], want) and torch.equal(gx, want[torch.arange(B, device="cuda") % 251])


# ------------------------------------------------------------------ one sample, through the module and through the entries
def test_one_sample_through_the_module_and_its_gradient_cancels():
    """x:(2, 1), f0:(2, 1), float64, the noise supplied.  The one frame is x[0] w + 1e-12 noise1 with its weighted mean removed, so y is
    held to the restatement at 64 max(D_ulp, 2^-53), D_ulp measured on this input as everywhere (in dB: the values are of magnitude
    100).  Every column of the frame's cotangent lands on the one sample, and the mean removal makes them sum to zero: what is left
    is the rounding of an L-term sum of cancelling terms plus the kernel's own `dot`, |gx| <= 8 L 2^-53 sum |gframes| (derived, not
    measured).  The half sum that DSA_VERSION 147 returned is of the size of the terms."""
    P, sr, L, K = 80, 16000, 1024, 513
    x = np.array([[0.25], [-0.5]])
    f0 = np.array([[203.0], [0.0]])
    n1, n2, gy = (np.round(np.random.default_rng(s).standard_normal((2, 1, n)) * 256) / 256 for s, n in ((31, L), (32, K), (33, K)))
    dev = [torch.as_tensor(a).cuda() for a in (x, f0, n1, n2, gy)]
    m = dsp.PitchAdaptiveSpectralAnalysis(P, sr, L, out_format="db", device="cuda", dtype=torch.float64)
    by_shape = {tuple(t.shape): t for t in dev[2:4]}
    m._randn = lambda shape: by_shape[tuple(shape)]
    xg = dev[0].clone().requires_grad_(True)
    y = m(xg, dev[1])
    assert _lib.last_kernel() == "pitch_spec_f64"
    y.backward(dev[4])
    kw = dict(out_format="db", noise1=n1, noise2=n2)
    ry, _ = pitch_spec_ref.pitch_spec(x, f0, P, sr, L, **kw)
    d = 0.0
    for signs in ((1, 1), (1, -1), (-1, 1)):   # three draws of the directions of two samples
        xp = np.nextafter(x, np.asarray(signs)[:, None] * np.inf)
        d = max(d, A.rel(pitch_spec_ref.pitch_spec(xp, f0, P, sr, L, **kw)[0], ry))
    lim = 64 * max(d, 2.0 ** -53)
    err = A.rel(y.detach().cpu().numpy(), ry)
    print(f"one sample: y off the restatement by {err:.3g} of max |y| = {np.abs(ry).max():.3g}, bound {lim:.3g} (D_ulp {d:.3g})")
    assert np.isfinite(ry).all() and err <= lim
    # the two entries of the backward, called here: the frames' cotangents, then the gather
    tw = device_twiddle(L, "cuda", torch.float64)
    gframes = torch.full((2, 1, L), float("nan"), device="cuda", dtype=torch.float64)
    p = ops._p
    ops._call("dsa_pitch_spec_vjp_frames", p(dev[4]), p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(tw), 2, 1, 1, P, sr, L, 500.0, -0.15, 0.0, 0.0, 0,
              _lib.F64, p(gframes), ops._stream())
    assert _lib.last_kernel() == "pitch_spec_vjp_frames_f64" and torch.isfinite(gframes).all()
    gx, _ = gather(gframes, P, 1, "float64")
    assert torch.equal(gx, xg.grad)   # the module's backward is these two calls
    for b in range(2):
        terms = gframes[b].abs().sum().item()
        lim = 8 * L * 2.0 ** -53 * terms
        print(f"one sample, utterance {b}: |gx| = {abs(gx[b, 0].item()):.3g}, bound 8 L 2^-53 sum |gframes| = {lim:.3g} (sum |gframes| = {terms:.3g})")
        assert terms > 0 and abs(gx[b, 0].item()) <= lim


# ------------------------------------------------------------------ the frames kernels below 1024 points and up to Nyquist
EDGE = [(name, mode) for name in A.EDGE_CASES for mode in A.EDGE_MODES]


@functools.lru_cache(maxsize=None)
def edge_result(name, mode, dt):
    """(y, gframes, gx) of the three entries on the case, and their routes"""
    (P, sr, L), kw = A.edge_options(name, mode)
    B, N, T, _, K = A.edge_sizes(name)
    tdt, code = DT[dt]
    x, f0 = A.edge_inputs(name)
    x, f0, n1, n2, gy = (torch.as_tensor(a).to("cuda", tdt) for a in (x, f0, *A.edge_noises(name), A.edge_cotangent(name)))
    tw = device_twiddle(L, "cuda", torch.float64)
    floor_ratio = 0.0 if kw["relative_floor"] is None else 10 ** (kw["relative_floor"] / 10)
    p = ops._p
    common = (p(x), p(f0), p(n1), p(n2), p(tw), B, N, T, P, sr, L, float(kw["default_f0"]), kw["q1"], kw["eps"], floor_ratio, kw["out_format"], code)
    y = torch.full((B, N, K), float("nan"), device="cuda", dtype=tdt)
    ops._call("dsa_pitch_spec", *common, p(y), ops._stream())
    routes = [_lib.last_kernel()]
    gframes = torch.full((B, N, L), float("nan"), device="cuda", dtype=torch.float64)
    ops._call("dsa_pitch_spec_vjp_frames", p(gy), *common, p(gframes), ops._stream())
    routes.append(_lib.last_kernel())
    gx, route = gather(gframes, P, T, dt)
    return y.cpu(), gframes.cpu(), gx.cpu(), routes + [route]


@pytest.mark.parametrize("name,mode", EDGE)
def test_float64_against_the_restatement_below_1024_points(name, mode):
    ref = A.edge_reference(name, mode)
    y, gframes, gx, routes = edge_result(name, mode, "float64")
    assert routes == ["pitch_spec_f64", "pitch_spec_vjp_frames_f64", "pitch_spec_vjp_gather_f64"]
    assert y.dtype == gx.dtype == gframes.dtype == torch.float64
    bad = []
    for key, err, lim in (("y", A.rel(y.numpy(), ref["y"]), ref["bound"]), ("gframes", A.rel_rows(gframes.numpy(), ref["cot"]), ref["bound_cot"]),
                          ("gx", A.rel(gx.numpy(), ref["gx"]), ref["bound"])):
        print(f"{name} {mode} float64 {key}: {err:.3g}, bound {lim:.3g} ({err / lim:.2g} of it)")
        if not err <= lim:   # (a NaN fails)
            bad.append((key, err, lim))
    assert not bad, bad
    # a frame's cotangent is exactly zero outside its window of 2 h + 1 samples, and every element was written
    (P, sr, L), kw = A.edge_options(name, mode)
    f0 = A.edge_inputs(name)[1].astype(np.float64)
    h = np.round(1.5 * sr / np.where(f0 <= 3 * sr / (L - 3), kw["default_f0"], f0))[..., None]
    outside = torch.as_tensor(np.abs(np.arange(L) - L // 2) > h)
    assert outside.any() and not gframes[outside].any() and torch.isfinite(gframes).all()


@pytest.mark.parametrize("name,mode", EDGE)
def test_float32_is_the_float64_result_rounded_once_below_1024_points(name, mode):
    y32, _, gx32, routes = edge_result(name, mode, "float32")
    y64, _, gx64, _ = edge_result(name, mode, "float64")
    assert routes == ["pitch_spec_f32", "pitch_spec_vjp_frames_f32", "pitch_spec_vjp_gather_f32"] and y32.dtype == gx32.dtype == torch.float32
    for key, a, b in (("y", y32, y64), ("gx", gx32, gx64)):
        excess = ((a.double() - b).abs() / b.abs().clamp(min=1.0)).max().item()
        print(f"{name} {mode} {key}: float32 off the float64 kernel by {excess:.3g} max(1, |value|), bound {2.0 ** -23:.3g}")
        assert excess <= 2.0 ** -23   # (a NaN fails)
