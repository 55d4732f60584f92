"""Every entry with tensors that are only element-aligned.

The C entries take raw pointers and the ops layer only calls .contiguous(), which keeps the storage offset of a view that is already
contiguous: wave[1:], or a slice of a flat buffer, reaches the kernels 4 bytes (float64: 8) past a 16-byte boundary.  Several
launchers and kernels choose another kernel, or another load / store width, on the address of a caller's tensor (DESIGN.md lists
them).  Part A drives each of those branches from both sides and pins (1) the kernel that runs, (2) the result against a float64
reference at the tolerance the family's own test file states, (3) bit equality with the aligned call wherever the same kernel runs.
Part B sweeps every public module (tests/alignment_rows.py) forward and backward with every tensor argument and the cotangent one
element off the allocator's block, against the aligned call, bit for bit.

Output pointers (the ops layer allocates them) are reached through the entries themselves; the four spare elements around such a
view keep the sentinel they were filled with."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from alignment_rows import ROWS
from diffsptk_amd import _lib, ops
from diffsptk_amd.utils import tables
from oracle import oracle as O
from oracle import torch_port as TP
# The tolerances, float64 references and input generators of the families' own test files, imported so that they cannot drift apart --
# at the price that this file has to follow when one of those modules is reorganised.
from test_gpu_fused import oracle_fbank
from test_gpu_lpc_fused import _chain64, _mods
from test_gpu_lsp import benign_lsp, rough_lsp
from test_gpu_parcor import benign_rows
from test_gpu_parity import F32_MCEP, spec_close
from test_gpu_plp import spectra
from test_gpu_stft_bwd import grad_and_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0
F32 = torch.float32


def host(t):
    return t.detach().cpu().numpy()


def offset_view(t, k):
    """`t` copied k elements into a fresh flat buffer of numel + 4 elements (the rest holds SENTINEL), viewed in t's shape: contiguous,
    and k elements past the allocator's (at least 16-byte aligned) block."""
    buf = torch.full((t.numel() + 4,), SENTINEL, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == k
    assert v.data_ptr() % 16 == (k * t.element_size()) % 16, "this view is not where the test says it is"
    return v


def spare_intact(v):
    """the four elements around an offset_view still hold the sentinel"""
    base, k, n = v._base, v.storage_offset(), v.numel()
    assert base is not None and base.numel() == n + 4
    return bool((base[:k] == SENTINEL).all()) and bool((base[k + n:] == SENTINEL).all())


def out_view(shape, k, dtype=F32):
    return offset_view(torch.full(shape, float("nan"), dtype=dtype, device=DEV), k)


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


_CACHE = {}


def cached(key, make):
    """a reference computed once and shared by the cases of a test"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# =================================================================================================== Part A
# ---------------------------------------------------------------------------------------------------- Frame (csrc/spec.hip)
@pytest.mark.parametrize("kx,ky", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1)])
@pytest.mark.parametrize("B,T", [(2, 2000), (1, 400)])
def test_frame_forward(B, T, kx, ky):
    """dsa_frame_fwd: frame_fwd_vec4 needs F L >= 4096 and y on a 16-byte boundary; inside it an x off the boundary takes the
    sample-by-sample loads (src_aligned).  Framing copies: exact against the oracle (tests/test_gpu_parity.py::test_frame_big_matches_oracle)."""
    L, P = 400, 80
    N = (T - 1) // P + 1
    x = randn(B, T, seed=T)
    xd, y = offset_view(x.to(DEV), kx), out_view((B, N, L), ky)
    ops._call("dsa_frame_fwd", ops._p(xd), B, T, L, P, 1, 0, 0, _lib.F32, ops._p(y), ops._stream())
    assert _lib.last_kernel() == ("frame_fwd_vec4" if ky == 0 and B * N * L >= 4096 else "frame_fwd")
    assert spare_intact(y)
    assert np.array_equal(host(y).astype(np.float64), O.frame(x.double().numpy(), L, P))
    ya = dsp.Frame(L, P)(x.to(DEV))   # the aligned call (its kernel copies the same values whatever it is)
    assert torch.equal(y, ya)


# ---------------------------------------------------------------------------------------------------- Window (csrc/spec.hip)
@pytest.mark.parametrize("which,k", [("none", 0)] + [(w, k) for w in ("in", "w", "out") for k in (1, 2, 3)])
def test_window_forward_and_backward(which, k):
    """dsa_window_fwd / _bwd: window_vec4 needs all three pointers on a 16-byte boundary.  One float32 product per element: the result
    is the float64 product rounded once, whichever kernel runs."""
    F_, L = 16, 400
    x, gy = randn(F_, L, seed=1).to(DEV), randn(F_, L, seed=2).to(DEV)
    w = dsp.Window(L, device=DEV).window
    ki, kw, ko = (k if which == "in" else 0), (k if which == "w" else 0), (k if which == "out" else 0)
    xo, gyo, wo = offset_view(x, ki), offset_view(gy, ki), offset_view(w, kw)   # (named: a temporary's block would be handed out again)
    y = out_view((F_, L), ko)
    ops._call("dsa_window_fwd", ops._p(xo), F_, L, ops._p(wo), L, _lib.F32, ops._p(y), ops._stream())
    assert _lib.last_kernel() == ("window_vec4" if which == "none" else "window_fwd")
    assert spare_intact(y)
    assert torch.equal(y, (x.double() * w.double()).float())
    gx, gw = out_view((F_, L), ko), out_view((L,), ko)
    ops._call("dsa_window_bwd", ops._p(gyo), ops._p(xo), F_, L, ops._p(wo), L, _lib.F32, ops._p(gx), ops._p(gw), ops._stream())
    assert _lib.last_kernel() == "window_bwd"   # (one name for both kernels of the backward)
    assert spare_intact(gx) and spare_intact(gw)
    assert torch.equal(gx, (gy.double() * w.double()).float())
    # gw[l] = sum_f gy x, 16 products and 15 additions in float32: at most 31 roundings of 2^-24 of the sum of magnitudes
    ref = (gy.double() * x.double()).sum(0)
    assert bool(((gw.double() - ref).abs() <= 31 * 2.0 ** -24 * (gy.double() * x.double()).abs().sum(0)).all())
    gxa, gwa = torch.empty_like(x), torch.empty(L, device=DEV)
    ops._call("dsa_window_bwd", ops._p(gy), ops._p(x), F_, L, ops._p(w), L, _lib.F32, ops._p(gxa), ops._p(gwa), ops._stream())
    assert torch.equal(gw, gwa)   # window_gw_kernel: one kernel, one order of summation


# ---------------------------------------------------------------------------------------------------- STFT 1024 / 2048 (csrc/stft.hip)
BIG = [(800, 200, 1024), (1200, 240, 2048)]
BIG_T = 4800


def _big(fl, fp, nfft):
    def make():
        x = randn(2, BIG_T, seed=fl)
        cot = randn(2, (BIG_T - 1) // fp + 1, nfft // 2 + 1, seed=fl + 1)
        st = dsp.STFT(fl, fp, nfft, device=DEV)
        xa = x.to(DEV).requires_grad_(True)
        ya = st(xa)
        assert _lib.last_kernel() == f"stft{nfft}_fwd"
        (ga,) = torch.autograd.grad(ya, xa, cot.to(DEV))
        xd = x.double().to(DEV).requires_grad_(True)
        (g64,) = torch.autograd.grad(dsp.STFT(fl, fp, nfft, device=DEV, dtype=torch.float64)(xd), xd, cot.double().to(DEV))
        return dict(x=x, cot=cot, st=st, ya=ya.detach(), ga=ga, y64=O.stft(x.double().numpy(), fl, fp, nfft), g64=g64)
    return cached(("big", nfft), make)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("fl,fp,nfft", BIG)
def test_stft_big_forward(fl, fp, nfft, k):
    """dsa_stft_fwd: stft1024_fwd / stft2048_fwd read sample pairs and need x on an 8-byte boundary; else the generic route.  Bound:
    tests/test_gpu_stft_big.py (spec_close)."""
    r = _big(fl, fp, nfft)
    y = r["st"](offset_view(r["x"].to(DEV), k))
    assert _lib.last_kernel() == (f"stft{nfft}_fwd" if k == 2 else "row_fft_generic")
    spec_close(host(y), r["y64"])
    if k == 2:
        assert torch.equal(y, r["ya"])


@pytest.mark.parametrize("kx,kg", [(2, 2), (2, 0), (0, 2), (1, 0), (0, 1), (2, 1), (3, 3)])
@pytest.mark.parametrize("fl,fp,nfft", BIG)
def test_stft_big_backward(fl, fp, nfft, kx, kg):
    """dsa_stft_bwd: the packed 1024 / 2048 backward needs x and gx on 8-byte boundaries; else the generic backward (whose last launch
    is the overlap-add, frame_bwd).  Bound: tests/test_gpu_stft_big.py, 3e-6 of the largest entry of the float64 gradient."""
    r = _big(fl, fp, nfft)
    st, B = r["st"], 2
    x, gy, gx = offset_view(r["x"].to(DEV), kx), r["cot"].to(DEV), out_view((B, BIG_T), kg)
    ops._call("dsa_stft_bwd", ops._p(gy), ops._p(x), B, BIG_T, fl, fp, nfft, ops._p(st.window), ops._p(st.twiddle), 1, 0, 0, float(st.eps), 0, 0.0,
              3, _lib.F32, _lib.ALGO_AUTO, ops._p(gx), None, ops._stream())
    packed = kx % 2 == 0 and kg % 2 == 0
    assert _lib.last_kernel() == (f"stft{nfft}_bwd" if packed else "frame_bwd")
    assert spare_intact(gx)
    err = float((gx.double() - r["g64"]).abs().max()) / float(r["g64"].abs().max())
    assert err < 3e-6, err
    if packed:
        assert torch.equal(gx, r["ga"])


# ---------------------------------------------------------------------------------------------------- STFT 512 (csrc/stft.hip, stft_pk.h, stft_bwd_pk.h)
def _stft512(L, P, T):
    def make():
        x = randn(2, T, seed=L + P + T)
        st = dsp.STFT(L, P, 512, device=DEV)
        cot = randn(2, (T - 1) // P + 1, 257, seed=7)
        xa = x.to(DEV).requires_grad_(True)
        ya = st(xa)
        assert _lib.last_kernel() == "stft512_fwd"
        ga, kern = grad_and_kernel(ya, xa, cot.to(DEV))
        xr = x.double().clone().requires_grad_(True)
        (TP.stft_power(xr, L, P, 512) * cot.double()).sum().backward()
        return dict(x=x, st=st, cot=cot, ya=ya.detach(), ga=ga, kern=kern, y64=O.stft(x.double().numpy(), L, P, 512), g64=xr.grad)
    return cached(("stft512", L, P, T), make)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("T", [4000, 4001])
@pytest.mark.parametrize("L,P,bwd_kernel", [(400, 80, "stft512_bwd_pk"), (400, 160, "stft512_bwd_pk"), (320, 80, "stft512_bwd")])
def test_stft512_forward_and_backward(L, P, bwd_kernel, T, k):
    """The tuned fft_length-512 kernels -- packed (frame_length 400: stft_pk.h, stft_bwd_pk.h) and register-FFT (any other frame length:
    stft512_fwd_kernel / stft512_bwd_kernel) -- fetch a run's stretch in 16-byte pieces when (x + g0) is on a 16-byte boundary and
    sample by sample otherwise: per run, inside one kernel, so the name does not move and the bits must not.  Bounds: spec_close;
    tests/test_gpu_stft_bwd.py, 2e-6 of the utterance's largest gradient entry."""
    r = _stft512(L, P, T)
    st = r["st"]
    assert r["kern"] == bwd_kernel
    xo = offset_view(r["x"].to(DEV), k).requires_grad_(True)
    y = st(xo)
    assert _lib.last_kernel() == "stft512_fwd"
    assert torch.equal(y, r["ya"])
    spec_close(host(y), r["y64"])
    g, kern = grad_and_kernel(y, xo, offset_view(r["cot"].to(DEV), k))
    assert kern == bwd_kernel
    assert torch.equal(g, r["ga"])
    err = (g.cpu().double() - r["g64"]).abs().amax(-1) / r["g64"].abs().amax(-1)
    assert float(err.max()) < 2e-6
    for kx, kg in ((k, k), (0, k)):   # the gradient's own pointer: through the entry
        gy, xk, gx = r["cot"].to(DEV), offset_view(r["x"].to(DEV), kx), out_view((2, T), kg)
        ops._call("dsa_stft_bwd", ops._p(gy), ops._p(xk), 2, T, L, P, 512, ops._p(st.window), ops._p(st.twiddle), 1, 0, 0, float(st.eps), 0, 0.0, 3,
                  _lib.F32, _lib.ALGO_AUTO, ops._p(gx), None, ops._stream())
        assert _lib.last_kernel() == bwd_kernel
        assert spare_intact(gx)
        assert torch.equal(gx, r["ga"])


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("T", [4000, 4001])
@pytest.mark.parametrize("P", [80, 160])
def test_fused_stft_mcep(P, T, k):
    """fuse(stft, mcep): the one-launch kernel fetches its tile's stretch like the packed STFT kernel.  Bound: F32_MCEP against the oracle."""
    n_iter = 5
    x = randn(2, T, seed=P + T)
    stft = dsp.STFT(400, P, 512, device=DEV)
    mcep = dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=n_iter, device=DEV)
    fused = dsp.fuse(stft, mcep)
    with torch.no_grad():
        ma = fused(x.to(DEV))
        name = _lib.last_kernel()
        mo = fused(offset_view(x.to(DEV), k))
    assert fused.last_path == "fused" and name == "stft512_mcep_fused_fwd" and _lib.last_kernel() == name
    assert torch.equal(mo, ma)
    ref = cached(("mcep", P, T), lambda: O.mcep(O.stft(x.double().numpy(), 400, P, 512), 24, 0.42, n_iter))
    np.testing.assert_allclose(host(mo), ref, **F32_MCEP)
    # with a gradient the same launch also writes the spectrogram and the Newton history; the backward is the two stages' own
    cot = randn(*ma.shape, seed=3).to(DEV)
    grads = []
    for xs, c in ((x.to(DEV), cot), (offset_view(x.to(DEV), k), offset_view(cot, k))):
        xs = xs.requires_grad_(True)
        grads.append(torch.autograd.grad(fused(xs), xs, c)[0])
        assert fused.last_path == "fused"
    assert torch.equal(grads[1], grads[0])


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("T", [4000, 4001])
@pytest.mark.parametrize("P", [80, 160])
def test_fused_stft_fbank(P, T, k):
    """fuse(stft, fbank): stft512_fwd_pk_kernel with the mel sums behind it.  Bound: tests/test_gpu_fused.py, 2e-5 absolute against the oracle."""
    x = randn(2, T, seed=P + T + 1)
    stft = dsp.STFT(400, P, 512, device=DEV)
    fb = dsp.MelFilterBankAnalysis(fft_length=512, n_channel=40, sample_rate=16000, use_power=True, device=DEV)
    fused = dsp.fuse(stft, fb)
    with torch.no_grad():
        ya = fused(x.to(DEV))
        name = _lib.last_kernel()
        yo = fused(offset_view(x.to(DEV), k))
    assert fused.last_path == "fused" and name == "stft512_fbank_fwd" and _lib.last_kernel() == name
    assert torch.equal(yo, ya)
    ref = cached(("fbank", P, T), lambda: oracle_fbank(x.numpy(), P, 40, 16000, use_power=True))
    np.testing.assert_allclose(host(yo), ref, rtol=0, atol=2e-5)
    cot = randn(*ya.shape, seed=4).to(DEV)
    grads = []
    for xs, c in ((x.to(DEV), cot), (offset_view(x.to(DEV), k), offset_view(cot, k))):
        xs = xs.requires_grad_(True)
        grads.append(torch.autograd.grad(fused(xs), xs, c)[0])
        assert fused.last_path == "fused"
    assert torch.equal(grads[1], grads[0])


# ---------------------------------------------------------------------------------------------------- LPC (csrc/lpc.hip, lpc24.hip, lpc24_bwd.hip)
def _lpc_fused(P, T):
    def make():
        x = randn(2, T, seed=P + T + 2).to(DEV)
        gy = randn(2, (T - 1) // P + 1, 25, seed=5).to(DEV)
        y64, g64 = _chain64(x, 400, P, gy=gy)
        out = dict(x=x, gy=gy, y64=y64, g64=g64)
        for exact in (False, True):
            fl = dsp.fuse(*_mods(400, P), exact_lag_sums=exact)
            with torch.no_grad():
                out[exact] = fl(x)
            assert _lib.last_kernel() == ("frame_window_lpc24_fwd" if exact else "frame_window_lpc24_mfma_fwd")
        fl = dsp.fuse(*_mods(400, P))
        xg = x.clone().requires_grad_(True)
        (out["ga"],) = torch.autograd.grad(fl(xg), xg, gy)
        assert fl.last_path == "fused"
        return out
    return cached(("lpc", P, T), make)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("T", [4000, 4001])
@pytest.mark.parametrize("P", [80, 160])
def test_fused_lpc_forward_and_backward(P, T, k):
    """fuse(frame, window, lpc).  Forward: frame_window_lpc24_kernel (exact lag sums) stages a run's stretch in 16-byte pieces when
    (x + g0) is on a 16-byte boundary; the matrix-pipe kernel reads sample by sample.  Backward (frame_window_lpc24_bwd_mfma): each
    flush of the overlap-add ring stores 16 bytes at a time when that stretch of gx is on a 16-byte boundary.  Bound:
    tests/test_gpu_lpc_fused.py, 2e-5 (outputs: of max(1, largest); gradient: of its largest entry) against the float64 chain."""
    r = _lpc_fused(P, T)
    w = dsp.Window(400, device=DEV).window
    for exact in (False, True):
        fl = dsp.fuse(*_mods(400, P), exact_lag_sums=exact)
        with torch.no_grad():
            y = fl(offset_view(r["x"], k))
        assert fl.last_path == "fused-forward"
        assert _lib.last_kernel() == ("frame_window_lpc24_fwd" if exact else "frame_window_lpc24_mfma_fwd")
        assert torch.equal(y, r[exact])
        assert float((y.double() - r["y64"]).abs().max()) < 2e-5 * max(1.0, float(r["y64"].abs().max()))
    for kx, kg in ((k, 0), (0, k), (k, k)):
        gy, xk, gx = offset_view(r["gy"], kx), offset_view(r["x"], kx), out_view((2, T), kg)
        ops._call("dsa_frame_window_lpc_bwd", ops._p(gy), ops._p(xk), 2, T, 400, P, ops._p(w), 1, 0, 24, 1e-5, _lib.F32, ops._p(gx), ops._stream())
        assert _lib.last_kernel() == "frame_window_lpc24_bwd_mfma"
        assert spare_intact(gx)
        assert torch.equal(gx, r["ga"])
        assert float((gx.double() - r["g64"]).abs().max()) < 2e-5 * float(r["g64"].abs().max())


@pytest.mark.parametrize("kx,kg", [(1, 0), (2, 0), (0, 1), (0, 2), (3, 3)])
def test_lpc24_backward(kx, kg):
    """dsa_lpc_bwd (lpc24_bwd_kernel): frames are staged 16 bytes at a time when x and gx are both on a 16-byte boundary.  Bound:
    tests/test_gpu_parity.py::test_lpc_tuned_backward_matches_float64_path, 2e-6 of the largest entry of the float64 gradient."""
    Fr, L = 70, 400

    def make():
        x32, gy = randn(Fr, L, seed=8), randn(Fr, 25, seed=9)
        out = dict(gy=gy.to(DEV))
        for dt in (torch.float32, torch.float64):
            x = x32.to(DEV, dt).requires_grad_(True)
            a = dsp.LPC(L, 24, eps=1e-5, dtype=dt, device=DEV)(x)
            (g,) = torch.autograd.grad(a, x, gy.to(DEV, dt))
            out[dt] = (x.detach(), a.detach(), g)
        return out
    r = cached("lpc24_bwd", make)
    x, a, ga = r[torch.float32]
    xk, gx = offset_view(x, kx), out_view((Fr, L), kg)
    ops._call("dsa_lpc_bwd", ops._p(r["gy"]), ops._p(xk), ops._p(a), Fr, L, 24, 1e-5, _lib.F32, ops._p(gx), ops._stream())
    assert _lib.last_kernel() == "lpc24_bwd"
    assert spare_intact(gx)
    assert torch.equal(gx, ga)
    g64 = r[torch.float64][2]
    assert float((gx.double() - g64).abs().max()) <= 2e-6 * float(g64.abs().max())


# ---------------------------------------------------------------------------------------------------- filter bank (csrc/fbank.hip)
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("which", ["x", "H", "y"])
def test_fbank_matrix_core_forward(which, k):
    """fbank_mfma_fwd: 16-byte tile loads of x (vec4), the 16-byte copy of H into LDS, 16-byte stores of y (yvec4), each with a
    scalar twin.  Bound: tests/test_gpu_parity.py::test_fbank_matrix_core_forward_matches_float64, 2e-5 / 2e-5 against the float64 kernel."""
    K, C, Fr = 257, 40, 130

    def make():
        x = (torch.rand(Fr, K, generator=torch.Generator().manual_seed(1)) * 10 + 1e-3) ** 3
        H = torch.from_numpy(np.asarray(tables.fbank_matrix(512, C, 16000, 0.0, None, "htk", None))).double()
        y64, E64 = ops.FbankFn.apply(x.double().to(DEV), H.to(DEV), 1e-5, 0.0, True)
        ya, Ea = ops.FbankFn.apply(x.to(DEV), H.float().to(DEV), 1e-5, 0.0, True)
        assert _lib.last_kernel() == "fbank_mfma_fwd"
        return dict(x=x.to(DEV), H=H.float().to(DEV), y64=host(y64), E64=host(E64), ya=ya, Ea=Ea)
    r = cached("fbank", make)
    x = offset_view(r["x"], k if which == "x" else 0)
    H = offset_view(r["H"], k if which == "H" else 0)
    y, E = out_view((Fr, C), k if which == "y" else 0), out_view((Fr, 1), 0)
    ops._call("dsa_fbank_fwd", ops._p(x), Fr, K, ops._p(H), C, 1e-5, 0.0, 1, _lib.F32, ops._p(y), ops._p(E), ops._stream())
    assert _lib.last_kernel() == "fbank_mfma_fwd"
    assert spare_intact(y) and spare_intact(E)
    assert torch.equal(y, r["ya"]) and torch.equal(E, r["Ea"])
    np.testing.assert_allclose(host(y), r["y64"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(host(E), r["E64"], rtol=2e-5, atol=2e-5)


# =================================================================================================== Part B
class _Recorder:
    """the loaded library, noting the name of every entry that is looked up on it"""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        if name.startswith("dsa_"):
            self.names.add(name)
        return getattr(self._lib, name)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _complex(rng, shape, dt):
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return torch.from_numpy(z).to(torch.complex64 if dt == torch.float32 else torch.complex128)


def _case(name, dt, odd):
    """(callable, [host tensors]) of a row: batch 3, rows of M + 1 with M = 24 / 25, spectra (50, 257), waveforms of 1600 / 1601 samples
    (filters with one coefficient row per frame: 20 frames of 80 samples / 1601 frames of one sample -- 1601 is prime)."""
    rng = np.random.default_rng(len(name) * 7 + odd)
    kw = dict(device=DEV, dtype=dt)
    M = 24 + odd
    M1 = M + 1
    T = 1600 + odd
    P, N = (1, T) if odd else (80, T // 80)
    Nf = (T - 1) // 80 + 1
    wave = lambda: _t(rng.standard_normal((3, T)), dt)                       # noqa: E731
    rows = lambda n=M1, s=1.0: _t(s * rng.standard_normal((3, 10, n)), dt)   # noqa: E731
    spec = lambda: _t(spectra(rng, 50), dt)                                  # noqa: E731
    stable = lambda F_: benign_rows(rng, F_, M)                              # noqa: E731
    stft = lambda: dsp.STFT(400, 80, 512, **kw)                              # noqa: E731
    if name == "Frame":
        return dsp.Frame(400, 80), [wave()]
    if name == "Window":
        return dsp.Window(M1, **kw), [rows()]
    if name == "RealValuedFastFourierTransform":
        return dsp.RealValuedFastFourierTransform(64, **kw), [rows()]
    if name == "RealValuedInverseFastFourierTransform":
        return dsp.RealValuedInverseFastFourierTransform(64, M1, **kw), [_complex(rng, (3, 10, 33), dt)]
    if name == "Spectrum":
        a = rows()
        a[..., 0] = a[..., 0].abs() + 0.5
        return dsp.Spectrum(64, eps=1e-3), [rows(), a]
    if name == "ShortTimeFourierTransform":
        return stft(), [wave()]
    if name == "InverseShortTimeFourierTransform":
        m = dsp.ISTFT(400, 80, 512, **kw)
        return (lambda y: m(y, out_length=T)), [_complex(rng, (3, Nf, 257), dt)]
    if name == "Unframe":
        m = dsp.Unframe(400, 80, window="blackman", norm="power", **kw)
        return (lambda y: m(y, out_length=T)), [_t(rng.standard_normal((3, Nf, 400)), dt)]
    if name == "GriffinLim":
        m = dsp.GriffinLim(400, 80, 512, n_iter=2, init_phase="zeros", **kw)
        return (lambda y: m(y, out_length=T)), [_t(rng.exponential(1.0, (3, Nf, 257)), dt)]
    if name == "Autocorrelation":
        return dsp.Autocorrelation(64 + odd, M), [rows(64 + odd)]
    if name == "LevinsonDurbin":
        x = rng.standard_normal((3, 10, 64))
        r = np.stack([(x[..., :64 - m] * x[..., m:]).sum(-1) for m in range(M1)], -1)
        return dsp.LevinsonDurbin(M, eps=1e-5, **kw), [_t(r, dt)]
    if name == "LinearPredictiveCodingAnalysis":
        return dsp.LPC(64 + odd, M, eps=1e-5, **kw), [rows(64 + odd)]
    if name == "FusedFrameWindowLPC":
        return dsp.fuse(dsp.Frame(400, 80), dsp.Window(400, **kw), dsp.LPC(400, M, eps=1e-5, **kw)), [wave()]
    if name == "LinearPredictiveCoefficientsToParcorCoefficients":
        return dsp.LinearPredictiveCoefficientsToParcorCoefficients(M), [_t(stable(30)[0].reshape(3, 10, M1), dt)]
    if name == "ParcorCoefficientsToLinearPredictiveCoefficients":
        return dsp.ParcorCoefficientsToLinearPredictiveCoefficients(M), [_t(stable(30)[1].reshape(3, 10, M1), dt)]
    if name == "LinearPredictiveCoefficientsStabilityCheck":
        a = benign_rows(rng, 30, M, unstable_every=4)[0]
        return dsp.LinearPredictiveCoefficientsStabilityCheck(M, margin=0.01, warn_type="ignore"), [_t(a.reshape(3, 10, M1), dt)]
    if name == "ParcorCoefficientsToLogAreaRatio":
        return dsp.ParcorCoefficientsToLogAreaRatio(M), [_t(stable(30)[1].reshape(3, 10, M1), dt)]
    if name == "LogAreaRatioToParcorCoefficients":
        return dsp.LogAreaRatioToParcorCoefficients(M), [rows()]
    if name == "ParcorCoefficientsToInverseSine":
        return dsp.ParcorCoefficientsToInverseSine(M), [_t(stable(30)[1].reshape(3, 10, M1), dt)]
    if name == "InverseSineToParcorCoefficients":
        return dsp.InverseSineToParcorCoefficients(M), [rows(s=0.3)]
    if name == "LinearPredictiveCoefficientsToLineSpectralPairs":
        return dsp.LinearPredictiveCoefficientsToLineSpectralPairs(M, **kw), [_t(stable(30)[0].reshape(3, 10, M1), dt)]
    if name == "LineSpectralPairsToLinearPredictiveCoefficients":
        return dsp.LineSpectralPairsToLinearPredictiveCoefficients(M, **kw), [_t(benign_lsp(rng, 30, M).reshape(3, 10, M1), dt)]
    if name == "LineSpectralPairsStabilityCheck":
        return dsp.LineSpectralPairsStabilityCheck(M, rate=0.3, n_iter=4, warn_type="ignore"), [_t(rough_lsp(rng, 30, M).reshape(3, 10, M1), dt)]
    if name == "FrequencyTransform":
        return dsp.FrequencyTransform(M, M + 3, alpha=0.42, **kw), [rows()]
    if name == "DiscreteCosineTransform":
        return dsp.DCT(M1, **kw), [rows()]
    if name == "MelFilterBankAnalysis":
        return dsp.MelFilterBankAnalysis(fft_length=512, n_channel=40, sample_rate=16000, **kw), [spec()]
    if name == "MelFrequencyCepstralCoefficientsAnalysis":
        return dsp.MFCC(fft_length=512, mfcc_order=12, n_channel=40, sample_rate=16000, **kw), [spec()]
    if name == "PerceptualLinearPredictiveCoefficientsAnalysis":
        return dsp.PLP(fft_length=512, plp_order=12, n_channel=40, sample_rate=16000, **kw), [spec()]
    if name == "FusedSTFTFilterBank":
        return dsp.fuse(stft(), dsp.MelFilterBankAnalysis(fft_length=512, n_channel=40, sample_rate=16000, use_power=True, **kw)), [wave()]
    if name == "CepstralAnalysis":
        return dsp.CepstralAnalysis(fft_length=512, cep_order=M, n_iter=2, **kw), [spec()]
    if name == "MelCepstralAnalysis":
        return dsp.MelCepstralAnalysis(fft_length=512, cep_order=M, alpha=0.42, n_iter=3, **kw), [spec()]
    if name == "FusedSTFTMelCepstralAnalysis":
        return dsp.fuse(stft(), dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=3, **kw)), [wave()]
    if name == "MelGeneralizedCepstralAnalysis":
        # (rows of 25 / 24 here: cep_order 24 runs the one-launch step, 23 the step kernel with its float32 adjoint; 25 has neither)
        return dsp.MelGeneralizedCepstralAnalysis(fft_length=512, cep_order=24 - odd, alpha=0.42, gamma=-0.5, n_iter=2, **kw), [spec()]
    if name == "GeneralizedCepstrumGainNormalization":
        return dsp.GeneralizedCepstrumGainNormalization(M, gamma=-0.5), [rows(s=0.1)]
    if name == "GeneralizedCepstrumInverseGainNormalization":
        y = rows(s=0.1)
        y[..., 0] = y[..., 0].abs() + 0.5
        return dsp.GeneralizedCepstrumInverseGainNormalization(M, gamma=-0.5), [y]
    if name == "MelCepstrumToMLSADigitalFilterCoefficients":
        return dsp.MelCepstrumToMLSADigitalFilterCoefficients(M, alpha=0.42, **kw), [rows()]
    if name == "MLSADigitalFilterCoefficientsToMelCepstrum":
        return dsp.MLSADigitalFilterCoefficientsToMelCepstrum(M, alpha=0.42, **kw), [rows()]
    if name == "MelGeneralizedCepstrumToMelGeneralizedCepstrum":
        return dsp.MelGeneralizedCepstrumToMelGeneralizedCepstrum(M, M + 2, in_alpha=0.42, out_alpha=0.1, in_gamma=-0.5, out_gamma=-0.25,
                                                                  n_fft=128, **kw), [rows(s=0.1)]
    if name == "MelGeneralizedCepstrumToSpectrum":
        return dsp.MelGeneralizedCepstrumToSpectrum(M, 512, alpha=0.42, **kw), [rows(s=0.1)]
    if name == "AllZeroDigitalFilter":
        return dsp.AllZeroDigitalFilter(M, P, **kw), [wave(), _t(rng.standard_normal((3, N, M1)), dt)]
    if name == "LinearInterpolation":
        return dsp.LinearInterpolation(P), [_t(rng.standard_normal((3, N, M1)), dt)]
    if name == "AllPoleDigitalFilter":
        return dsp.AllPoleDigitalFilter(M, P), [wave(), _t(stable(3 * N)[0].reshape(3, N, M1), dt)]
    if name == "PseudoMGLSADigitalFilter":
        return (dsp.MLSA(M, P, alpha=0.42, mode="multi-stage", taylor_order=7, cep_order=100, **kw),
                [wave(), _t(0.1 * rng.standard_normal((3, N, M1)), dt)])
    if name == "Decimation":
        return dsp.Decimation(3, 1), [wave()]
    if name == "Interpolation":
        return dsp.Interpolation(3, 1), [wave()]
    if name == "PseudoQuadratureMirrorFilterBankAnalysis":
        return dsp.PQMF(4, 40, **kw), [_t(rng.standard_normal((3, 1, T)), dt)]
    if name == "PseudoQuadratureMirrorFilterBankSynthesis":
        return dsp.IPQMF(4, 40, **kw), [_t(rng.standard_normal((3, 4, T)), dt)]
    if name == "FusedPQMFDecimation":
        return dsp.fuse(dsp.PQMF(4, 40, **kw), dsp.Decimation(4, 1)), [_t(rng.standard_normal((3, 1, T)), dt)]
    if name == "FusedInterpolationIPQMF":
        return dsp.fuse(dsp.Interpolation(4, 1), dsp.IPQMF(4, 40, **kw)), [_t(rng.standard_normal((3, 4, T // 4)), dt)]
    raise KeyError(name)


def _run(fn, inputs, k):
    """forward without a graph (several modules keep launches for that case), then forward and backward, with every tensor argument
    and the cotangent k elements into its buffer (0: as allocated)"""
    place = (lambda t: offset_view(t, k)) if k else (lambda t: t.clone())
    xs = [place(t.to(DEV)) for t in inputs]
    with torch.no_grad():
        plain = fn(*xs)
    xs = [t.requires_grad_(True) for t in xs]
    out = fn(*xs)
    names = [_lib.last_kernel()]
    assert isinstance(out, torch.Tensor)
    grads = []
    if out.requires_grad:
        # dsa_last_kernel() is per thread and the backward runs on autograd's: a hook on an input sees it there (as grad_and_kernel)
        hooks = [t.register_hook(lambda g: names.append(_lib.last_kernel())) for t in xs]
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(out.real.dtype)
        if out.is_complex():
            cot = torch.complex(cot, cot.flip(-1))
        grads = torch.autograd.grad(out, xs, place(cot.to(DEV)), allow_unused=True)
        for h in hooks:
            h.remove()
    return (plain, out.detach()), grads, (names[0], names[-1])


_CALLED = {}   # (row, dtype, odd) -> the entries looked up while the row ran


def _sweep(name, dt, odd):
    if (name, dt, odd) in _CALLED:
        return
    # (every call into the library goes through _lib.load(), which hands out the module's `_lib`: the one place to listen in)
    rec = _Recorder(_lib.load())
    _lib._lib = rec
    try:
        fn, inputs = _case(name, dt, odd)
        ya, ga, ka = _run(fn, inputs, 0)
        yo, go, ko = _run(fn, inputs, 1)
    finally:
        _lib._lib = rec._lib
    assert ko == ka, (ka, ko)   # (last forward kernel, last kernel seen on the backward's thread)
    for a, o in zip(ya, yo):   # (without a graph, with one)
        assert bool(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all())
        assert torch.equal(o, a)
    assert len(go) == len(ga)
    for a, o in zip(ga, go):
        assert (a is None) == (o is None)
        if a is not None:
            assert bool(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all())
            assert torch.equal(o, a)
    _CALLED[(name, dt, odd)] = rec.names


SWEEP = [(name, dt, odd) for name in sorted(ROWS) for dt in (torch.float32, torch.float64) for odd in (0, 1)]


@pytest.mark.parametrize("name,dt,odd", SWEEP, ids=[f"{n}-{'f32' if d == torch.float32 else 'f64'}-{'odd' if o else 'even'}" for n, d, o in SWEEP])
def test_every_module_one_element_off(name, dt, odd):
    """Outputs and every gradient equal the all-aligned call's, bit for bit (whose own float64 parity the family's tests hold), and the
    last kernel of the forward and of the backward is the one the aligned call ran: at the sweep's small shapes no row changes its
    kernel.  (Which kernel that is, is the business of the family's own tests: the sweep names none.)"""
    _sweep(name, dt, odd)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_the_rows_reach_the_entries_they_name(name):
    """tests/alignment_rows.py is what the CPU completeness test trusts: every entry a row names is really called by that row's
    forward or backward, at one of the sweep's types and sizes."""
    called = set()
    for n, dt, odd in SWEEP:
        if n == name:
            _sweep(n, dt, odd)   # (already run by the sweep above unless this test was selected alone)
            called |= _CALLED[(n, dt, odd)]
    missing = set(ROWS[name]) - called
    assert not missing, f"{name} never called {sorted(missing)} (it called {sorted(n for n in called if n.endswith(('_fwd', '_bwd')))})"
