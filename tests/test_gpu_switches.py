"""The route switches of the library that used to be cached on the first call follow the environment in-process: for each, ONE
process makes the same call with the variable unset, set to the other value, and unset again, and reads the route name
(`_lib.last_kernel()`) after each -- the default route, the other route, the default route.  Shapes: the smallest that reach the
launcher's condition (tests/kernel_routes.py).  The other route's result agrees with the default route's within the float32 bound
tests/kernel_routes.py carries for the pair (relative to the largest entry, or to each row's, as that bound is defined there); where
the table carries none, only the name and finiteness are asserted.  The unset-again result equals the first bit for bit.
DSA_LPC_LAGSUMS selects between two kernels of one route name, so there the outputs are compared.  Each case prints its figures."""
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, ops

import kernel_routes as KR
import routes_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def inputs(call, **args):
    return {k: v.to(DEV) for k, v in R.inputs_of(KR.case(call, "fwd", KR.F32, **args), torch.float32).items()}


def fftr():
    t = inputs("fftr", len_in=32, nfft=32, fmt=0, F=5)
    return torch.view_as_real(dsp.RealValuedFastFourierTransform(32, 0, device=DEV)(t["x"]))


def thsolve():
    t = inputs("thsolve", n=24, F=37)
    return ops.ThSolveFn.apply(t["p"], t["q"], t["r"])


def fftcep():
    t = inputs("fftcep", nfft=32, M=5, accel=0.5, n_iter=1, F=5)
    return dsp.CepstralAnalysis(fft_length=32, cep_order=5, accel=0.5, n_iter=1, device=DEV)(t["x"])


def freqt():
    t = inputs("freqt", L1=49, L2=25, F=5)
    return ops.MatmulRowsFn.apply(t["c"], t["A"])


def stft():
    x = R.gauss(1024, 2, 2048).to(device=DEV, dtype=torch.float32)
    return dsp.STFT(1024, 256, 1024, device=DEV)(x)


FFTR_BOUND = KR.tolerance("row_fft_generic", KR.case("fftr", "fwd", len_in=32, nfft=32, fmt=0), "f32")     # the restatement's, at this shape
FREQT_BOUND = KR.tolerance("freqt_mfma_fwd", KR.ROUTES["freqt_mfma_fwd"][0], "f32")                       # L1 = 49, L2 = 25: this shape
# (variable, the other value, call, default route, other route, (bound, metric) or None)
SWITCHES = [
    ("DSA_ROWDFT_DIRECT", "1", fftr, "row_fft_generic", "row_dft_generic", (FFTR_BOUND, "max")),
    ("DSA_THSOLVE_QUAD", "0", thsolve, "th_solve_quad_fwd", "th_solve_fwd", None),
    ("DSA_FFTCEP_DIRECT", "1", fftcep, "fftcep_fft_fwd", "fftcep_fwd", (KR.FFTCEP["tol"][1], KR.FFTCEP["metric"])),
    ("DSA_FREQT_GENERIC", "1", freqt, "freqt_mfma_fwd", "freqt_lds_fwd", (FREQT_BOUND, "max")),
    ("DSA_STFT_BIG", "0", stft, "stft1024_fwd", "row_fft_generic", None),
]


@pytest.mark.parametrize("name,other,call,route,other_route,bound", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_a_switch_follows_the_environment_within_one_process(name, other, call, route, other_route, bound, monkeypatch):
    monkeypatch.delenv(name, raising=False)
    first, k_first = call(), _lib.last_kernel()
    monkeypatch.setenv(name, other)
    second, k_second = call(), _lib.last_kernel()
    monkeypatch.delenv(name)
    third, k_third = call(), _lib.last_kernel()
    err = R.error(second.cpu(), first.cpu(), bound[1] if bound else "max")
    print(f"{name}: unset {k_first}, ={other} {k_second}, unset {k_third}; other route against default {err:.2e}, bound {bound[0] if bound else None}")
    assert (k_first, k_second, k_third) == (route, other_route, route)
    assert all(bool(torch.isfinite(y).all()) for y in (first, second, third)) and second.shape == first.shape
    assert torch.equal(third, first)
    if bound:
        assert err <= bound[0], (err, bound)


def test_lpc_lag_sums_follow_the_environment_within_one_process(monkeypatch):
    """DSA_LPC_LAGSUMS=f64 is exact_lag_sums=True, bit for bit; unset again, the first output again"""
    x = inputs("fwlpc", T=250, L=50, P=20, M=24, eps=1e-5)["x"]

    def run(**options):
        fused = dsp.fuse(dsp.Frame(50, 20), dsp.Window(50, device=DEV), dsp.LPC(50, 24, eps=1e-5, device=DEV), **options)
        with torch.no_grad():
            y = fused(x)
        assert fused.last_path == "fused-forward", fused.last_path
        return y

    monkeypatch.delenv("DSA_LPC_LAGSUMS", raising=False)
    first, exact = run(), run(exact_lag_sums=True)
    monkeypatch.setenv("DSA_LPC_LAGSUMS", "f64")
    by_env = run()
    monkeypatch.delenv("DSA_LPC_LAGSUMS")
    third = run()
    print(f"DSA_LPC_LAGSUMS: default against exact {float((first - exact).abs().max()):.2e} (largest |a| {float(exact.abs().max()):.2e})")
    assert all(bool(torch.isfinite(y).all()) for y in (first, exact, by_env, third))
    assert torch.equal(by_env, exact)
    assert torch.equal(third, first)
