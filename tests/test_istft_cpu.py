"""CPU side of tests/test_gpu_istft.py: the helpers of tests/istft_ref.py are pinned to the float64 oracle (itself pinned to the
reference's exported results by tests/test_oracle_golden.py), the inputs are shown to leave the stated margin under the tight bound, and
ops._fold_plan -- which decides the lengths the inverse kernels run with -- is held to the shape of the oracle's result."""
import numpy as np
import pytest
import torch

import istft_ref as R
from oracle import oracle as O

GEOMETRIES = {c["id"]: c for c in R.CASES_F32}   # CASES_F64 repeats a subset of these geometries
TUNED = [c for c in R.CASES_F32 if c["route"] in (R.PACKED, R.SPAN)]


def _spectra(c, seed=0):
    B = int(np.prod(c["lead"]))
    return R.spectra(seed + c["N"] + c["L"], B, c["N"], c["nfft"] // 2 + 1)


@pytest.mark.parametrize("cid", list(GEOMETRIES))
def test_istft_torch_is_the_oracle(cid):
    """istft_torch (the reference of every gradient) against oracle.istft: 1e-12 of the largest entry, every centring and out_length."""
    c = GEOMETRIES[cid]
    Y = _spectra(c)
    for center in (True, False):
        for ol in R.out_lengths(c, center):
            ref, d = R.reference(Y, c["L"], c["P"], c["nfft"], center, out_length=ol)
            got = R.istft_torch(torch.view_as_real(Y), c["L"], c["P"], c["nfft"], center, out_length=ol).numpy()
            assert got.shape == ref.shape and d.shape == ref.shape[-1:]
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (center, ol)
            assert R.weighted_ratio(got, ref, d) <= 1e-12


@pytest.mark.parametrize("L,P", R.UNFRAME_GEOMETRIES)
def test_unframe_torch_is_the_oracle(L, P):
    y = R.frames(L, R.UNFRAME_B, R.UNFRAME_N, L)
    for window in R.UNFRAME_WINDOWS:
        for norm in R.UNFRAME_NORMS:
            w = torch.from_numpy(R.window64(L, window, norm).copy())
            for center in (True, False):
                for ol in R.unframe_out_lengths(L, P, center):
                    ref, d = R.reference_unframe(y, P, center, window, norm, ol)
                    got = R.unframe_torch(y, P, center, w, ol).numpy()
                    assert got.shape == ref.shape and d.shape == ref.shape[-1:]
                    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (window, norm, center, ol)


@pytest.mark.parametrize("nfft", R.IFFTR_LENGTHS)
def test_ifftr_torch_is_the_oracle(nfft):
    Y = R.spectra(nfft, 1, 65, nfft // 2 + 1)[0]
    for ol in R.ifftr_out_lengths(nfft):
        ref = O.ifftr(Y.numpy(), ol)
        got = R.ifftr_torch(torch.view_as_real(Y), nfft, ol).numpy()
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # ... and the definition agrees with the FFT on spectra whose DC and Nyquist bins carry imaginary parts
    assert Y[:, 0].imag.abs().min() > 0 and Y[:, -1].imag.abs().min() > 0
    assert np.abs(O.ifftr(Y.numpy()) - np.fft.irfft(Y.numpy(), n=nfft)).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("cid", [c["id"] for c in TUNED])
def test_float32_stock_operators_leave_the_margin(cid):
    """A float32 run of the same composition on stock operators (irfft, index_add, one division) stays within 5e-7 under the weighted rule
    on every tuned-route case: the 2e-6 the kernels are held to is four times that, so it is the kernels that are measured, not the inputs."""
    c = GEOMETRIES[cid]
    Y = _spectra(c).to(torch.complex64)
    w = torch.from_numpy(R.window64(c["L"]).copy()).float()
    worst = 0.0
    for center in (True, False):
        for ol in R.out_lengths(c, center):
            ref, d = R.reference(Y, c["L"], c["P"], c["nfft"], center, out_length=ol)
            fr = torch.fft.irfft(Y, n=c["nfft"])[..., :c["L"]]
            got = R.unframe_torch(fr, c["P"], center, w, ol)
            assert got.dtype == torch.float32
            worst = max(worst, R.weighted_ratio(got, ref, d))
    print("[istft] float32 stock operators %s: %.3e (bound 5e-7)" % (cid, worst))
    assert worst <= 5e-7


def test_weighted_rule_counts_every_sample():
    """The weight keeps the open ends comparable (d there is 1e-34 of its maximum) without leaving a sample out: an error of the bound's
    size in the NUMERATOR of any one sample, the first and the last included, is seen."""
    L, P, N = 400, 80, 6
    Y = R.spectra(1, 1, N, 257)
    ref, d = R.reference(Y, L, P, 512, center=False)
    assert d.min() < 1e-30 * d.max()
    assert R.weighted_ratio(ref, ref, d) == 0.0
    scale = (np.abs(ref) * (d + R.EPS)).max()
    for t in (0, 1, ref.shape[-1] // 2, ref.shape[-1] - 1):
        bad = ref.copy()
        bad[0, t] += 1e-5 * scale / (d[t] + R.EPS)
        assert 0.9e-5 < R.weighted_ratio(bad, ref, d) < 1.1e-5
    bad = ref.copy()
    bad[0, 3] = np.nan
    assert R.weighted_ratio(bad, ref, d) == float("inf")


@pytest.mark.parametrize("center", [True, False])
def test_rule_and_inputs_see_the_errors_they_are_there_for(center):
    """Float64 models of the slips the GPU tests are written against, on the tests' own inputs: each lands orders of magnitude above the
    loosest float32 bound (2e-4), so a kernel that made one of them could not pass.  On the STFT of a signal the second is invisible."""
    L, P, nfft, N, K = 400, 80, 512, 6, 257
    Y = R.spectra(7, 2, N, K)
    ref, d = R.reference(Y, L, P, nfft, center)

    def ratio_of(Ybad, **kw):
        return R.weighted_ratio(R.reference(Ybad, L, P, nfft, center, **kw)[0], ref, d)

    Yb = Y.clone()
    Yb[..., K - 1] *= 2                                  # the Nyquist bin with the weight 2 / n of the inner bins
    assert ratio_of(Yb) > 1e-2
    Yb = Y.clone()
    Yb.real[..., 0] += Y.imag[..., 0]                    # Im Y_0 mixed into the half-length packing
    assert ratio_of(Yb) > 1e-2
    Ys = torch.from_numpy(O.stft(np.random.default_rng(0).standard_normal((2, 480)), L, P, nfft, out_format="complex", eps=0.0))
    assert float(Ys.imag[..., 0].abs().max()) < 1e-9 and float(Ys.imag[..., K - 1].abs().max()) < 1e-9
    Yb = Y.clone()
    Yb[:, N - 1] = 0                                     # the last frame dropped (a frame count or a fold length off by one)
    assert ratio_of(Yb) > 1e-2
    assert R.weighted_ratio(np.roll(ref, 1, -1), ref, d) > 1e-2   # the result shifted by one sample (the centre trim off by one)


def test_spectra_are_random_in_every_bin():
    Y = R.spectra(3, 2, 5, 17)
    assert Y.dtype == torch.complex128 and Y.shape == (2, 5, 17)
    assert Y.imag[..., 0].abs().min() > 0 and Y.imag[..., -1].abs().min() > 0
    assert torch.equal(Y, R.spectra(3, 2, 5, 17)) and not torch.equal(Y, R.spectra(4, 2, 5, 17))


def test_cotangent_keeps_the_backward_division_bounded():
    _, d = R.reference(R.spectra(1, 1, 6, 257), 400, 80, 512, center=False)
    cot = R.cotangent(2, (1, d.size), d)
    q = cot.numpy() / (d + R.EPS) * d.max()        # what the division leaves: the seeded normal values
    assert np.isfinite(q).all() and 1.0 < np.abs(q).max() < 6.0


@pytest.mark.parametrize("cid", list(GEOMETRIES))
def test_fold_plan_matches_the_oracles_length(cid):
    """ops._fold_plan (pure Python, no device): T is the length oracle.unframe returns, for out_length None, inside the fold, at its full
    length and beyond it, with and without centring; the kernels run with Nc >= N frames and Tc >= T samples, num_frames(Tc) = Nc."""
    from diffsptk_amd.ops.stft import _fold_plan, num_frames

    c = GEOMETRIES[cid]
    N, L, P = c["N"], c["L"], c["P"]
    y = np.zeros((N, L))
    for center in (True, False):
        full = R.full_length(N, L, P, center)
        for ol in (None, 1, (N - 2) * P, N * P - 37, full, full - 1, full + 1, (N - 1) * P, (N - 1) * P + 1, N * P, 10 ** 9):
            if ol is not None and ol < 1:
                continue
            T, Tc, Nc = _fold_plan(N, L, P, center, ol)
            assert T == O.unframe(y, P, center, out_length=ol).shape[-1], (center, ol)
            assert Nc >= N and Tc >= T and Tc >= 1 and num_frames(Tc, P) == Nc, (center, ol, T, Tc, Nc)
            # the frames the kernels add beyond N are zero: they may not reach a sample that a real frame does not, unless it is cut off
            assert (Nc - 1) * P < Tc
