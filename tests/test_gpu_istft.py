"""The inverse STFT path on the GPU -- ISTFT on each of its kernel routes (csrc/stft.hip, stft_bwd_impl), its backward, Unframe and ifftr
-- against float64, on spectra that are NOT the STFT of a signal (random in every bin, the imaginary parts of DC and Nyquist included).

Checker and rules: tests/istft_ref.py (oracle.istft / oracle.unframe / oracle.ifftr for results; float64 autograd of the same sums in
plain real arithmetic for gradients; results compared as overlap-added numerators, so that every sample counts although the window-square
sum vanishes at the open ends; gradients taken with a cotangent of the same weight).  The bounds are the ones the same kernels are held
to elsewhere in the suite (istft_ref.B_*).  Every figure is printed beside its bound before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import istft_ref as R
from diffsptk_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

ALL = {c["id"]: c for c in R.CASES_F32 + R.CASES_F64}

# one geometry per route for the properties that do not depend on the size: (label, real dtype, L, P, nfft, N, forward kernel)
ROUTES = [
    ("packed-P80", torch.float32, 400, 80, 512, 50, R.PACKED),
    ("packed-P160", torch.float32, 400, 160, 512, 50, R.PACKED),
    ("span-gather", torch.float32, 399, 77, 512, 50, R.SPAN),
    ("generic-fft2048", torch.float32, 1200, 240, 2048, 9, R.GENERIC),
    ("generic-dft60", torch.float32, 48, 20, 60, 50, R.GENERIC),
    ("float64", torch.float64, 400, 80, 512, 50, R.GENERIC),
]
ROUTE_IDS = [r[0] for r in ROUTES]


def cdtype(dt):
    return torch.complex64 if dt == torch.float32 else torch.complex128


def dtype_of(c):
    return torch.float64 if c["id"].startswith("f64-") else torch.float32


def bounds(dt, route):
    """(result, gradient) bounds of a case."""
    if dt == torch.float64:
        return R.B_F64, R.B_F64
    if route == R.GENERIC:
        return R.B_GEN_RESULT, R.B_GEN_GRAD
    return R.B_TUNED, R.B_TUNED


def backward_kernels(dt, nfft):
    if dt == torch.float32 and nfft == 512:
        return ("stft512_fwd",)
    return ("row_fft_generic",) if nfft & (nfft - 1) == 0 else ("row_dft_generic",)


def to_device(Y, dt):
    """The spectra on the device in the dtype under test, and the values the kernels see as complex128 on the host."""
    Yd = Y.to(DEV, cdtype(dt))
    return Yd, Yd.cpu().to(torch.complex128)


def forward(ist, Yd, out_length, route):
    with torch.no_grad():
        x = ist(Yd, out_length=out_length)
    assert _lib.last_kernel() == route, (_lib.last_kernel(), route)
    return x


def grad_and_kernel(y, x, cot):
    """Gradient of y w.r.t. x and the kernel that produced it: dsa_last_kernel() is per thread and the backward runs on autograd's worker
    thread, where a hook on x sees it right after the backward function (as in tests/test_gpu_stft_bwd.py)."""
    names = []
    h = x.register_hook(lambda g: names.append(_lib.last_kernel()))
    (gx,) = torch.autograd.grad(y, x, cot)
    h.remove()
    return gx, names[-1]


def device_gradient(ist, Yd, out_length, cot):
    Yg = Yd.clone().requires_grad_(True)
    g, kern = grad_and_kernel(ist(Yg, out_length=out_length), Yg, cot)
    return torch.view_as_real(g.resolve_conj()), kern


def reference_gradient(Yh, L, P, nfft, center, out_length, cot64):
    Yr = torch.view_as_real(Yh).clone().requires_grad_(True)
    (R.istft_torch(Yr, L, P, nfft, center, out_length=out_length) * cot64).sum().backward()
    return Yr.grad


# --------------------------------------------------------------------------- 1. results and gradients against float64, by route
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("cid", list(ALL))
def test_results_and_gradients_against_float64(cid, center):
    """Every route at every geometry, out_length None and -- where the case says so -- inside the fold, at its full length (with centring:
    the case that appends zero frames), beyond it and 1.  out_length beyond the fold gives the full fold's bits, every shorter one a prefix
    of them."""
    c = ALL[cid]
    dt, route = dtype_of(c), c["route"]
    L, P, nfft, N = c["L"], c["P"], c["nfft"], c["N"]
    K = nfft // 2 + 1
    rb, gb = bounds(dt, route)
    tag = "%s %s" % ("f64" if dt == torch.float64 else "f32", route)
    Y = R.spectra(N + L + P, int(np.prod(c["lead"])), N, K).reshape(*c["lead"], N, K)
    Yd, Yh = to_device(Y, dt)
    assert float(Yh.imag[..., 0].abs().min()) > 0 and float(Yh.imag[..., K - 1].abs().min()) > 0
    ist = dsp.ISTFT(L, P, nfft, center=center, device=DEV, dtype=dt)
    full = R.full_length(N, L, P, center)
    x_full = forward(ist, Yd, full, route) if c["extra"] else None
    res, grd = [], []
    for ol in R.out_lengths(c, center):
        x = forward(ist, Yd, ol, route)
        ref, d = R.reference(Yh, L, P, nfft, center, out_length=ol)
        assert x.shape == ref.shape and x.dtype == dt, (x.shape, ref.shape)
        res.append(R.hold("result   %s | %s center=%d out_length=%s" % (tag, c["id"], center, ol), R.weighted_ratio(x, ref, d), rb))
        if x_full is not None:
            assert x.shape[-1] == min(full, x.shape[-1])
            assert torch.equal(x, x_full[..., :x.shape[-1]]), ("not the full fold's bits", ol)
            if ol == 10 ** 9:
                assert x.shape == x_full.shape
        # gradient with the weighted cotangent (the values the device gets, so that the reference differentiates the same functional)
        cot = R.cotangent(N + (ol or 0) % 1000, ref.shape, d).to(DEV, dt)
        g, kern = device_gradient(ist, Yd, ol, cot)
        assert kern in backward_kernels(dt, nfft), kern
        gref = reference_gradient(Yh, L, P, nfft, center, ol, cot.cpu().double())
        assert g.shape == gref.shape
        grd.append(R.hold("gradient %s | %s center=%d out_length=%s" % (tag, c["id"], center, ol), R.relative_ratio(g, gref, 3), gb))
    R.worst("result of %s center=%d" % (c["id"], center), res, rb)
    R.worst("gradient of %s center=%d" % (c["id"], center), grd, gb)


# --------------------------------------------------------------------------- 2. Im(DC), Im(Nyquist) carry no weight
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_imaginary_parts_of_dc_and_nyquist_carry_no_weight(route, center):
    """irfft ignores Im Y_0 and Im Y_{n/2} (ifftr.py:138): the result's bits do not change when they are zeroed, and the gradient with
    respect to them (float64 run of the same geometry) is zero to 1e-9 of the largest entry -- the reference's is exactly 0."""
    label, dt, L, P, nfft, N, kern = route
    K = nfft // 2 + 1
    Y = R.spectra(21, 3, N, K)
    Y0 = Y.clone()
    Y0.imag[..., 0] = 0.0
    Y0.imag[..., K - 1] = 0.0
    assert not torch.equal(Y, Y0) and torch.equal(Y[..., 1:K - 1], Y0[..., 1:K - 1]) and torch.equal(Y.real, Y0.real)
    ist = dsp.ISTFT(L, P, nfft, center=center, device=DEV, dtype=dt)
    a = forward(ist, Y.to(DEV, cdtype(dt)), None, kern)
    b = forward(ist, Y0.to(DEV, cdtype(dt)), None, kern)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    ist64 = dsp.ISTFT(L, P, nfft, center=center, device=DEV, dtype=torch.float64)
    Yd, Yh = to_device(Y, torch.float64)
    ref, d = R.reference(Yh, L, P, nfft, center)
    cot = R.cotangent(22, ref.shape, d)
    g, _ = device_gradient(ist64, Yd, None, cot.to(DEV))
    gref = reference_gradient(Yh, L, P, nfft, center, None, cot)
    assert float(gref[..., 0, 1].abs().max()) == 0.0 and float(gref[..., K - 1, 1].abs().max()) == 0.0
    edge = max(float(g[..., 0, 1].abs().max()), float(g[..., K - 1, 1].abs().max()))
    R.hold("Im grad  f64 | %s center=%d (DC, Nyquist)" % (label, center), edge / float(gref.abs().max()), R.B_F64)
    R.hold("gradient f64 | %s center=%d" % (label, center), R.relative_ratio(g, gref, 3), R.B_F64)


# --------------------------------------------------------------------------- 3. bits do not depend on the batch or the run partition
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("P,N,copies", [(80, 200, (1, 3, 600)), (160, 100, (1, 1024))])
def test_packed_result_does_not_depend_on_the_run_partition(P, N, copies, center):
    """The host cuts an utterance of the packed kernel into min(ceil(4096 / B), max(1, ceil(N / 4) // 4)) runs: P = 80, N = 200 gives 12
    runs alone and among 3 copies and 7 among 600; P = 160, N = 100 gives 6 runs alone and 4 among 1024.  With the division by the
    window-square sum fused into the store, every copy has the bits of the utterance run alone."""
    def runs(B):
        return min(-(-4096 // B), max(1, -(-N // 4) // 4))
    assert [runs(B) for B in copies] == ([12, 12, 7] if P == 80 else [6, 4])
    Yd = R.spectra(31 + P, 1, N, 257).to(DEV, torch.complex64)
    ist = dsp.ISTFT(400, P, 512, center=center, device=DEV)
    single = forward(ist, Yd, None, R.PACKED)
    assert torch.isfinite(single).all() and float(single.abs().max()) > 0
    for B in copies:
        x = forward(ist, Yd.expand(B, -1, -1).contiguous(), None, R.PACKED)
        assert x.shape == (B, single.shape[-1])
        assert torch.equal(x, single.expand_as(x)), B
        del x


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_result_does_not_depend_on_the_batch_or_the_call(route, center):
    """Each of three different utterances alone has the bits it has in the batch; two calls on the same input agree bit for bit."""
    label, dt, L, P, nfft, N, kern = route
    Yd = R.spectra(41, 3, N, nfft // 2 + 1).to(DEV, cdtype(dt))
    ist = dsp.ISTFT(L, P, nfft, center=center, device=DEV, dtype=dt)
    x = forward(ist, Yd, None, kern)
    assert torch.isfinite(x).all()
    assert torch.equal(x, forward(ist, Yd, None, kern))
    for b in range(3):
        assert torch.equal(forward(ist, Yd[b:b + 1].contiguous(), None, kern)[0], x[b]), b
    Yg = Yd.clone().requires_grad_(True)
    y = ist(Yg)
    cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(42), dtype=torch.float64).to(DEV, dt)
    (g1,) = torch.autograd.grad(y, Yg, cot, retain_graph=True)
    (g2,) = torch.autograd.grad(y, Yg, cot)
    assert torch.equal(torch.view_as_real(g1), torch.view_as_real(g2))


# --------------------------------------------------------------------------- 4. a non-finite bin stays in its frame
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_nonfinite_bin_stays_in_its_frame(route, center):
    """A NaN in one bin of frame n0 of utterance 1 reaches the samples of that frame, [n0 P - left, n0 P - left + L), and nothing else:
    every other sample keeps the bits of the clean run."""
    label, dt, L, P, nfft, N, kern = route
    Y = R.spectra(51, 3, N, nfft // 2 + 1)
    n0 = N // 2 + 1
    ist = dsp.ISTFT(L, P, nfft, center=center, device=DEV, dtype=dt)
    clean = forward(ist, Y.to(DEV, cdtype(dt)), None, kern)
    assert torch.isfinite(clean).all()
    Y[1, n0, 17] = complex(float("nan"), 0.0)
    x = forward(ist, Y.to(DEV, cdtype(dt)), None, kern)
    bad = ~torch.isfinite(x)
    T = x.shape[-1]
    lo = n0 * P - (L // 2 if center else 0)
    inside = torch.zeros(3, T, dtype=torch.bool, device=x.device)
    inside[1, max(lo, 0):min(lo + L, T)] = True
    assert 0 <= lo and lo + L <= T, "the frame lies inside the result"
    assert bad.any() and not (bad & ~inside).any()
    assert torch.equal(x[~inside], clean[~inside])


# --------------------------------------------------------------------------- 5. input forms
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_conjugated_and_strided_inputs(route):
    label, dt, L, P, nfft, N, kern = route
    K = nfft // 2 + 1
    big = R.spectra(61, 3, 2 * N, K).to(DEV, cdtype(dt))
    ist = dsp.ISTFT(L, P, nfft, device=DEV, dtype=dt)
    Yd = big[:, :N].contiguous()
    lazy = Yd.conj()
    assert lazy.is_conj()
    a = forward(ist, lazy, None, kern)
    b = forward(ist, Yd.conj().resolve_conj(), None, kern)
    assert torch.equal(a, b) and not torch.equal(a, forward(ist, Yd, None, kern))
    strided = big[:, ::2]
    assert not strided.is_contiguous() and strided.shape == (3, N, K)
    assert torch.equal(forward(ist, strided, None, kern), forward(ist, strided.contiguous(), None, kern))
    # ... and in the backward: a gradient of the strided view lands on the frames it selects
    bg = big.clone().requires_grad_(True)
    y = ist(bg[:, ::2])
    cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(62), dtype=torch.float64).to(DEV, dt)
    (g,) = torch.autograd.grad(y, bg, cot)
    Yc = strided.contiguous().requires_grad_(True)
    (gc,) = torch.autograd.grad(ist(Yc), Yc, cot)
    assert torch.equal(torch.view_as_real(g[:, ::2]), torch.view_as_real(gc)) and float(g[:, 1::2].abs().max()) == 0.0


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_empty_batch(route, center):
    label, dt, L, P, nfft, N, kern = route
    K = nfft // 2 + 1
    ist = dsp.ISTFT(L, P, nfft, center=center, device=DEV, dtype=dt)
    Y = torch.zeros(0, N, K, dtype=cdtype(dt), device=DEV, requires_grad=True)
    T = N * P if center else R.full_length(N, L, P, center)
    x = ist(Y)
    assert x.shape == (0, T) and x.dtype == dt
    (g,) = torch.autograd.grad(x, Y, torch.zeros_like(x))
    assert g.shape == (0, N, K) and g.dtype == cdtype(dt)


def test_real_input_is_refused():
    ist = dsp.ISTFT(400, 80, 512, device=DEV)
    with pytest.raises(ValueError, match="Input must be a complex tensor."):
        ist(torch.zeros(2, 5, 257, device=DEV))
    with pytest.raises(ValueError, match="Input must be a complex tensor."):
        dsp.RealValuedInverseFastFourierTransform(512, device=DEV)(torch.zeros(2, 257, device=DEV))


# --------------------------------------------------------------------------- 6. Unframe and ifftr
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("L,P", R.UNFRAME_GEOMETRIES)
def test_unframe_matches_oracle_and_autograd(L, P, center, dt):
    """Unframe (window, overlap-add on the Frame backward kernel -- vec4 at L = 400, scalar otherwise --, division) for three windows and
    two normalisations, out_length None, the full fold and inside it: results under the weighted rule, gradients against float64 autograd
    of unframe_torch, both at the generic bounds."""
    rb, gb = bounds(dt, R.GENERIC)
    tag = "f64" if dt == torch.float64 else "f32"
    B, N = R.UNFRAME_B, R.UNFRAME_N
    yd = R.frames(L + P, B, N, L).to(DEV, dt)
    yh = yd.cpu().double()
    res, grd = [], []
    for window in R.UNFRAME_WINDOWS:
        for norm in R.UNFRAME_NORMS:
            unf = dsp.Unframe(L, P, center=center, window=window, norm=norm, device=DEV, dtype=dt)
            w64 = torch.from_numpy(R.window64(L, window, norm).copy())
            for ol in R.unframe_out_lengths(L, P, center):
                what = "unframe %s | L=%d P=%d %s/%s center=%d out_length=%s" % (tag, L, P, window, norm, center, ol)
                ref, d = R.reference_unframe(yh, P, center, window, norm, ol)
                yg = yd.clone().requires_grad_(True)
                x = unf(yg, out_length=ol)
                assert _lib.last_kernel() == "div_rows"
                assert x.shape == ref.shape and x.dtype == dt
                res.append(R.hold("result   " + what, R.weighted_ratio(x, ref, d), rb))
                cot = R.cotangent(L + (ol or 0), ref.shape, d).to(DEV, dt)
                (g,) = torch.autograd.grad(x, yg, cot)
                yr = yh.clone().requires_grad_(True)
                (R.unframe_torch(yr, P, center, w64, ol) * cot.cpu().double()).sum().backward()
                grd.append(R.hold("gradient " + what, R.relative_ratio(g, yr.grad, 2), gb))
    R.worst("result of unframe %s L=%d P=%d center=%d" % (tag, L, P, center), res, rb)
    R.worst("gradient of unframe %s L=%d P=%d center=%d" % (tag, L, P, center), grd, gb)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rows", R.IFFTR_ROWS)
@pytest.mark.parametrize("nfft", R.IFFTR_LENGTHS)
def test_ifftr_matches_oracle_and_autograd(nfft, rows, dt):
    """ifftr on spectra with imaginary parts at DC and Nyquist, power-of-two lengths (the LDS FFT) and 60 (the direct sum), cropped
    outputs down to one sample: each row relative to its largest entry, at the generic bounds."""
    rb, gb = bounds(dt, R.GENERIC)
    tag = "f64" if dt == torch.float64 else "f32"
    K = nfft // 2 + 1
    Yd, Yh = to_device(R.spectra(nfft + rows, 1, rows, K)[0], dt)
    assert float(Yh.imag[:, 0].abs().min()) > 0 and float(Yh.imag[:, K - 1].abs().min()) > 0
    res, grd = [], []
    for ol in R.ifftr_out_lengths(nfft):
        what = "ifftr %s | nfft=%d rows=%d out_length=%s" % (tag, nfft, rows, ol)
        mod = dsp.RealValuedInverseFastFourierTransform(nfft, ol, device=DEV, dtype=dt)
        Yg = Yd.clone().requires_grad_(True)
        x = mod(Yg)
        # the inverse transform is the adjoint of the forward row transform: it runs on the rows' backward kernel
        assert _lib.last_kernel() == ("row_fft_bwd_generic" if nfft & (nfft - 1) == 0 else "row_dft_bwd_generic")
        ref = O.ifftr(Yh.numpy(), ol)
        assert x.shape == ref.shape and x.dtype == dt
        res.append(R.hold("result   " + what, R.relative_ratio(x, ref, 1), rb))
        cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(nfft), dtype=torch.float64).to(DEV, dt)
        (g,) = torch.autograd.grad(x, Yg, cot)
        Yr = torch.view_as_real(Yh).clone().requires_grad_(True)
        (R.ifftr_torch(Yr, nfft, ol) * cot.cpu().double()).sum().backward()
        grd.append(R.hold("gradient " + what, R.relative_ratio(torch.view_as_real(g.resolve_conj()), Yr.grad, 2), gb))
    R.worst("result of ifftr %s nfft=%d rows=%d" % (tag, nfft, rows), res, rb)
    R.worst("gradient of ifftr %s nfft=%d rows=%d" % (tag, nfft, rows), grd, gb)
