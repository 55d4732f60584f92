"""AllPoleDigitalFilter on the MI355X (csrc/poledf.hip): the reference's goldens (tests/golden/poledf.npz), an LPC analysis ->
synthesis round trip on data.wav, the bench-size batch against a float64 oracle, batch invariance, gradcheck, the generic kernels,
an empty batch and graph capture.  Float64 tolerances: rtol 1e-5 / atol 1e-8 (the suite's convention); float32 against 4 x the
error of a plain sequential float32 loop."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, functional as F, ops

pytestmark = pytest.mark.gpu

F64 = dict(rtol=1e-5, atol=1e-8)
DEV = "cuda:0"


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().double().numpy()


def coefs(a, P):
    """Per-sample interpolated rows: a:(..., N, M+1) -> (..., N P, M+1), in a's dtype."""
    N = a.shape[-2]
    t = np.arange(N * P)
    n = t // P
    n1 = np.minimum(n + 1, N - 1)
    w = ((t - n * P) / P).astype(a.dtype)[:, None]
    a0, a1 = a[..., n, :], a[..., n1, :]
    return a0 + w * (a1 - a0)


def oracle_fwd(x, c, ig):
    """x:(B, T), c:(T, M+1) shared by the rows -> y:(B, T); the plain sequential loop, vectorised over B, in x's dtype."""
    B, T = x.shape
    M = c.shape[1] - 1
    y = np.zeros_like(x)
    g = np.ones(T, x.dtype) if ig else c[:, 0]
    for t in range(T):
        v = g[t] * x[:, t]
        for k in range(min(M, t), 0, -1):
            v = v - c[t, k] * y[:, t - k]
        y[:, t] = v
    return y


def oracle_bwd(gy, x, y, c, ig, P, want_ga=True):
    """u, gx, ga of the adjoint (c:(T, M+1) shared by the rows; ga per row)."""
    B, T = gy.shape
    M = c.shape[1] - 1
    u = np.zeros_like(gy)
    for t in range(T - 1, -1, -1):
        v = gy[:, t].copy()
        for k in range(min(M, T - 1 - t), 0, -1):
            v = v - c[t + k, k] * u[:, t + k]
        u[:, t] = v
    g = np.ones(T, gy.dtype) if ig else c[:, 0]
    gx = g * u
    if not want_ga:
        return u, gx, None
    N = T // P
    dc = np.zeros((B, T, M + 1), gy.dtype)
    for k in range(1, M + 1):
        dc[:, k:, k] = -u[:, k:] * y[:, :-k]
    if not ig:
        dc[:, :, 0] = u * x
    t = np.arange(T)
    n = t // P
    n1 = np.minimum(n + 1, N - 1)
    w = ((t - n * P) / P)[None, :, None]
    ga = np.zeros((B, N, M + 1), gy.dtype)
    np.add.at(ga, (slice(None), n), (1 - w) * dc)
    np.add.at(ga, (slice(None), n1), w * dc)
    return u, gx, ga


def test_reference_goldens_float64(golden):
    z = golden("poledf")
    keys = sorted({k.rsplit("_", 1)[0] for k in z.files if k.startswith("M")})
    assert len(keys) == 36
    for key in keys:
        M, P, ig, d = (int(s[2:]) if s.startswith("ig") else int(s[1:]) for s in key.split("_"))
        x = dev(z[key + "_x"]).requires_grad_(True)
        a = dev(z[key + "_a"]).requires_grad_(True)
        m = dsp.AllPoleDigitalFilter(M, P, ignore_gain=bool(ig))
        y = m(x, a) if d == 2 else F.poledf(x, a, frame_period=P, ignore_gain=bool(ig))
        y.backward(dev(z[key + "_gy"]))
        np.testing.assert_allclose(host(y), z[key + "_y"], **F64, err_msg=key)
        np.testing.assert_allclose(host(x.grad), z[key + "_gx"], **F64, err_msg=key)
        np.testing.assert_allclose(host(a.grad), z[key + "_ga"], **F64, err_msg=key)
    for dt in (torch.float64, torch.float32):   # the docstring example, module and functional
        y1 = dsp.AllPoleDigitalFilter(0, 1)(dev(z["doc_x"], dt), dev(z["doc_a"], dt))
        y2 = F.poledf(dev(z["doc_x"], dt), dev(z["doc_a"], dt), frame_period=1)
        assert host(y1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] == host(y2).tolist()


def test_ring_kernels_are_the_ones_that_run():
    """(dsa_last_kernel is per host thread, and autograd runs the backward on a thread of its own: the backward entry is called
    here directly.)"""
    x, a = dev(np.random.default_rng(0).standard_normal((1, 160))), dev(np.full((1, 2, 25), 0.01))
    y = F.poledf(x, a, 80)
    assert _lib.last_kernel() == "poledf_ring_fwd"
    u, gx, ga = torch.empty_like(x), torch.empty_like(x), torch.empty_like(a)
    code = ops._dtype_code(x)
    ops._call("dsa_poledf_bwd", ops._p(x), ops._p(x), ops._p(a), ops._p(y), 1, 160, 24, 80, 0, code, ops._p(u), ops._p(gx), None, ops._stream())
    assert _lib.last_kernel() == "poledf_ring_bwd"
    ops._call("dsa_poledf_bwd", ops._p(x), ops._p(x), ops._p(a), ops._p(y), 1, 160, 24, 80, 0, code, ops._p(u), None, ops._p(ga), ops._stream())
    assert _lib.last_kernel() == "poledf_bwd_a"
    with pytest.raises(_lib.BackendError, match="u buffer"):
        ops._call("dsa_poledf_bwd", ops._p(x), ops._p(x), ops._p(a), ops._p(y), 1, 160, 24, 80, 0, code, None, ops._p(gx), None, ops._stream())


def _f32_bound(got, ref64, plain32):
    """4 x the error of the plain float32 loop, relative to max|ref|."""
    scale = np.abs(ref64).max()
    e_plain = np.abs(plain32.astype(np.float64) - ref64).max() / scale
    e_got = np.abs(got - ref64).max() / scale
    return e_got, e_plain


def test_round_trip_on_data_wav(golden):
    """poledf(zerodf(x, [1, a_1..a_M]), a, ignore_gain=True) == x with the data.wav LPC (19 200 samples, 240 frames, M = 24)."""
    z = golden("datawav")
    x64 = z["pcm"].astype(np.float64) / 32768.0
    a64 = z["lpc_f64"]
    b64 = a64.copy()
    b64[:, 0] = 1.0
    # float64: the inverse filter, then the synthesis filter
    e = F.zerodf(dev(x64), dev(b64), 80)
    xr = F.poledf(e, dev(a64), 80, ignore_gain=True)
    assert _lib.last_kernel() == "poledf_ring_fwd"
    err = np.abs(host(xr) - x64).max()
    assert err <= 1e-10 * np.abs(x64).max(), err
    # float32: the synthesis of the float64 residual, against the plain float32 loop's error
    e64 = host(e)
    c32, c64 = coefs(a64.astype(np.float32), 80), coefs(a64, 80)
    ref = oracle_fwd(e64[None], c64, True)[0]
    plain = oracle_fwd(e64[None].astype(np.float32), c32, True)[0]
    got = host(F.poledf(dev(e64, torch.float32), dev(a64, torch.float32), 80, ignore_gain=True))
    e_got, e_plain = _f32_bound(got, ref, plain)
    assert e_got <= 4 * e_plain, (e_got, e_plain)


def test_bench_size_float32_forward_and_backward(golden):
    """White noise through the data.wav LPC, B = 1024, T = 19 200, float32, forward and backward against a float64 oracle."""
    z = golden("datawav")
    a64 = z["lpc_f64"]
    B, P = 1024, 80
    rng = np.random.default_rng(7)
    x64 = rng.standard_normal((B, 19200)) * 0.1
    gy64 = rng.standard_normal((B, 19200))
    x32, gy32, a32 = x64.astype(np.float32), gy64.astype(np.float32), a64.astype(np.float32)
    xd = dev(x32, torch.float32).requires_grad_(True)
    ad = dev(np.broadcast_to(a32, (B, *a32.shape)), torch.float32).requires_grad_(True)
    y = F.poledf(xd, ad, P)
    y.backward(dev(gy32, torch.float32))
    c64, c32 = coefs(a64, P), coefs(a32, P)
    # forward, every row
    y64 = oracle_fwd(x64, c64, False)
    e_got, e_plain = _f32_bound(host(y), y64, oracle_fwd(x32, c32, False))
    assert e_got <= 4 * e_plain, ("y", e_got, e_plain)
    # gx, every row (the adjoint of the float64 oracle's own y)
    _, gx64, _ = oracle_bwd(gy64, x64, y64, c64, False, P, want_ga=False)
    _, gx32, _ = oracle_bwd(gy32, x32, oracle_fwd(x32, c32, False), c32, False, P, want_ga=False)
    e_got, e_plain = _f32_bound(host(xd.grad), gx64, gx32)
    assert e_got <= 4 * e_plain, ("gx", e_got, e_plain)
    # ga on 16 rows (the oracle forms the (B, T, M+1) per-sample gradients)
    rows = np.arange(0, B, B // 16)
    y32 = oracle_fwd(x32[rows], c32, False)
    _, _, ga64 = oracle_bwd(gy64[rows], x64[rows], y64[rows], c64, False, P)
    _, _, ga32 = oracle_bwd(gy32[rows], x32[rows], y32, c32, False, P)
    e_got, e_plain = _f32_bound(host(ad.grad)[rows], ga64, ga32)
    assert e_got <= max(4 * e_plain, 1e-6), ("ga", e_got, e_plain)


def test_batch_invariance_bitwise():
    rng = np.random.default_rng(3)
    B, N, P, M = 1024, 30, 80, 24
    x = dev(rng.standard_normal((B, N * P)), torch.float32)
    a = np.zeros((B, N, M + 1))
    a[..., 1:] = rng.uniform(-1, 1, (B, N, M)) * 0.6 / M
    a[..., 0] = rng.uniform(0.5, 1.5, (B, N))
    a = dev(a, torch.float32)
    gy = dev(rng.standard_normal((B, N * P)), torch.float32)
    xg, ag = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    y = F.poledf(xg, ag, P)
    y.backward(gy)
    for r in (0, 517, 1023):
        x1, a1 = x[r:r + 1].clone().requires_grad_(True), a[r:r + 1].clone().requires_grad_(True)
        y1 = F.poledf(x1, a1, P)
        y1.backward(gy[r:r + 1])
        assert torch.equal(y1[0], y[r]) and torch.equal(x1.grad[0], xg.grad[r]) and torch.equal(a1.grad[0], ag.grad[r]), r


@pytest.mark.parametrize("ig", [False, True])
def test_gradcheck_float64(ig):
    rng = np.random.default_rng(11)
    T, M, P = 48, 3, 8
    N = T // P
    a = rng.uniform(-0.2, 0.2, (2, N, M + 1))
    a[..., 0] = rng.uniform(0.5, 1.5, (2, N))
    x = dev(rng.standard_normal((2, T))).requires_grad_(True)
    ad = dev(a).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x_, a_: F.poledf(x_, a_, P, ig), (x, ad), eps=1e-6, atol=1e-7, rtol=1e-5)
    # 1-D input, and a batch of signals with one unbatched coefficient matrix (broadcast)
    m = dsp.AllPoleDigitalFilter(M, P, ignore_gain=ig)
    assert torch.autograd.gradcheck(lambda x_, a_: m(x_, a_), (x[0].detach().clone().requires_grad_(True),
                                                                  ad[0].detach().clone().requires_grad_(True)),
                                    eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda x_, a_: m(x_, a_), (x, ad[0].detach().clone().requires_grad_(True)), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("M,P,N", [(0, 16, 6), (64, 16, 12), (100, 16, 12), (24, 1, 200)])
def test_generic_path_against_the_oracle(M, P, N):
    rng = np.random.default_rng(M + P)
    T = N * P
    a = rng.uniform(-1, 1, (2, N, M + 1)) * 0.6 / max(M, 1)
    a[..., 0] = rng.uniform(0.5, 1.5, (2, N))
    x = rng.standard_normal((2, T))
    gy = rng.standard_normal((2, T))
    for ig in (False, True):
        xd, ad = dev(x).requires_grad_(True), dev(a).requires_grad_(True)
        y = F.poledf(xd, ad, P, ig)
        assert _lib.last_kernel() == "poledf_generic_fwd"
        y.backward(dev(gy))
        for r in range(2):
            c = coefs(a[r], P)
            y64 = oracle_fwd(x[r:r + 1], c, ig)
            _, gx64, ga64 = oracle_bwd(gy[r:r + 1], x[r:r + 1], y64, c, ig, P)
            np.testing.assert_allclose(host(y)[r], y64[0], **F64)
            np.testing.assert_allclose(host(xd.grad)[r], gx64[0], **F64)
            np.testing.assert_allclose(host(ad.grad)[r], ga64[0], **F64)


def test_empty_batch_and_graph_capture():
    for dt in (torch.float32, torch.float64):
        x = torch.empty(0, 160, device=DEV, dtype=dt, requires_grad=True)
        a = torch.empty(0, 2, 25, device=DEV, dtype=dt, requires_grad=True)
        y = F.poledf(x, a, 80)
        assert y.shape == (0, 160)
        y.sum().backward()
        assert x.grad.shape == x.shape and a.grad.shape == a.shape
    rng = np.random.default_rng(5)
    a = np.zeros((8, 20, 25))
    a[..., 1:] = rng.uniform(-1, 1, (8, 20, 24)) * 0.6 / 24
    a[..., 0] = 1.0
    x, ad = dev(rng.standard_normal((8, 1600)), torch.float32), dev(a, torch.float32)
    m = dsp.AllPoleDigitalFilter(24, 80)
    g = dsp.Graphed(m, x, ad)
    x2 = dev(rng.standard_normal((8, 1600)), torch.float32)
    out = g(x2, ad).clone()
    assert torch.equal(out, m(x2, ad))


def test_ops_rejects_mismatched_shapes():
    x, a = dev(np.zeros((2, 160))), dev(np.zeros((3, 2, 25)))
    with pytest.raises(ValueError):
        ops.poledf(x, a, 80, False)
