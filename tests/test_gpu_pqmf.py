"""PQMF / IPQMF / Decimation / Interpolation on the MI355X (csrc/pqmf.hip): the reference's goldens (tests/golden/pqmf.npz), the
bench size against a numpy float64 restatement, the folded routes against the module chain bit for bit, gradcheck, batch
invariance, empty and non-contiguous inputs, graph capture, and the README's subband example.  Tolerances relative to the largest
magnitude: 1e-12 in float64, 1e-5 in float32."""
import json
import os

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = json.load(open(os.path.join(ROOT, "tests", "golden", "pqmf_api.json")))
TOL = {torch.float64: 1e-12, torch.float32: 1e-5}


def wave(shape, seed):
    """the closed-form inputs of tests/golden/make_golden_pqmf.py"""
    n = np.arange(int(np.prod(shape)), dtype=np.float64)
    return (np.sin(0.0123 * (seed + 1) * n + seed) + 0.3 * np.cos(0.71 * n + 0.2 * seed)).reshape(shape)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().double().numpy()


def close(got, want, dtype, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max() / scale
    assert err <= TOL[dtype], (what, err)


def pads(M, analysis):
    if M % 2 == 0:
        return M // 2, M // 2
    return ((M + 1) // 2, (M - 1) // 2) if analysis else ((M - 1) // 2, (M + 1) // 2)


def np_pqmf(x, f):
    """numpy float64 restatement: x:(B, T), f:(K, M+1) stored (time-flipped) -> (B, K, T)."""
    M = f.shape[1] - 1
    dl, dr = pads(M, True)
    xp = np.concatenate([np.zeros((x.shape[0], dl)), x, np.repeat(x[:, -1:], dr, axis=1)], axis=1)
    win = np.lib.stride_tricks.sliding_window_view(xp, M + 1, axis=1)   # (B, T, M+1)
    return np.einsum("btj,kj->bkt", win, f)


def np_pqmf_gx(gy, f):
    """the adjoint of np_pqmf: gy:(B, K, T) -> gx:(B, T) (the replicate pad's gradients summed into the last sample)."""
    B, K, T = gy.shape
    M = f.shape[1] - 1
    dl, _ = pads(M, True)
    gxp = np.zeros((B, T + M))
    for i in range(M + 1):
        gxp[:, i:i + T] += np.einsum("bkt,k->bt", gy, f[:, i])
    gx = gxp[:, dl:dl + T].copy()
    gx[:, -1] += gxp[:, dl + T:].sum(1)
    return gx


def np_ipqmf(y, f):
    """y:(B, K, T), f:(K, M+1) stored -> (B, T)."""
    M = f.shape[1] - 1
    dl, dr = pads(M, False)
    yp = np.concatenate([np.zeros(y.shape[:2] + (dl,)), y, np.repeat(y[:, :, -1:], dr, axis=2)], axis=2)
    win = np.lib.stride_tricks.sliding_window_view(yp, M + 1, axis=2)   # (B, K, T, M+1)
    return np.einsum("bktj,kj->bt", win, f)


def run_case(K, M, T, route, P, s, form, dtype, fused, learnable=False):
    if route.startswith("pqmf"):
        m = dsp.PQMF(K, M, learnable=learnable, device=DEV, dtype=dtype)
        shape = {"1d": (T,), "2d": (2, T), "3d": (2, 1, T)}[form]
    else:
        m = dsp.IPQMF(K, M, learnable=learnable, device=DEV, dtype=dtype)
        shape = {"2d": (K, T), "3d": (2, K, T)}[form]
    x = dev(wave(shape, 1), dtype).requires_grad_(True)
    if route in ("pqmf", "ipqmf"):
        out = m(x)
    elif route == "pqmf_dec":
        out = dsp.fuse(m, dsp.Decimation(P, s))(x) if fused else dsp.Decimation(P, s)(m(x))
    else:
        out = dsp.fuse(dsp.Interpolation(P, s), m)(x) if fused else m(dsp.Interpolation(P, s)(x))
    (out * dev(wave(tuple(out.shape), 2), dtype)).sum().backward()
    return host(out), host(x.grad), None if not learnable else host(m.filters.grad)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_reference_goldens(golden, dtype):
    """Every case of the fixture, through the module chain and through fuse() (the float32 runs against the reference's float64)."""
    z = golden("pqmf")
    assert len(API["cases"]) == 94
    for i, (K, M, T, route, P, s, form, learnable) in enumerate(API["cases"]):
        for fused in ((False, True) if route in ("pqmf_dec", "interp_ipqmf") else (False,)):
            what = (i, K, M, T, route, P, s, form, fused, str(dtype))
            out, gin, gf = run_case(K, M, T, route, P, s, form, dtype, fused, learnable)
            close(out, z[f"case{i}_out"], dtype, ("out",) + what)
            close(gin, z[f"case{i}_gin"], dtype, ("gin",) + what)
            if learnable:
                close(gf, z[f"case{i}_gf"], dtype, ("gf",) + what)
    assert list(dsp.PQMF(4, 40, device=DEV)(torch.ones(1, 3, device=DEV)).shape) == API["short_input_shape"]


def test_tuned_and_generic_kernels_are_the_ones_that_run():
    x = torch.randn(2, 500, device=DEV)
    for K, M, want in ((4, 40, "tuned"), (8, 127, "tuned"), (9, 40, "generic"), (4, 128, "generic")):
        dsp.PQMF(K, M, device=DEV)(x)
        assert _lib.last_kernel() == f"pqmf_fwd_{want}", (K, M)
        dsp.IPQMF(K, M, device=DEV)(torch.randn(2, K, 125, device=DEV))
        assert _lib.last_kernel() == f"ipqmf_fwd_{want}", (K, M)
    dsp.fuse(dsp.PQMF(4, 40, device=DEV), dsp.Decimation(17))(x)
    assert _lib.last_kernel() == "pqmf_fwd_generic"   # a period above 16


@pytest.mark.parametrize("K,M", [(4, 40), (4, 62)])
def test_bench_size_float32_against_numpy(K, M):
    """B = 1024 x T = 16 000, float32, all four routes forward and the input gradients, 16 rows against a float64 numpy restatement."""
    B, T = 1024, 16000
    g = torch.Generator(device=DEV).manual_seed(K + M)
    x = torch.randn(B, T, device=DEV, generator=g).requires_grad_(True)
    pq, ip = dsp.PQMF(K, M, device=DEV), dsp.IPQMF(K, M, device=DEV)
    fa, fs = host(pq.filters[:, 0]), host(ip.filters[0])
    rows = np.arange(0, B, B // 16)
    y = pq(x)
    gy = torch.randn(B, K, T, device=DEV, generator=g)
    y.backward(gy)
    x64, gy64 = host(x)[rows], host(gy)[rows]
    close(host(y)[rows], np_pqmf(x64, fa), torch.float32, "pqmf")
    close(host(x.grad)[rows], np_pqmf_gx(gy64, fa), torch.float32, "pqmf gx")
    xd = x.detach().clone().requires_grad_(True)
    yd = dsp.fuse(pq, dsp.Decimation(K, 1))(xd)
    gyd = torch.randn(yd.shape, device=DEV, generator=g)
    yd.backward(gyd)
    full = np.zeros((16, K, T))
    full[:, :, 1::K] = host(gyd)[rows]
    close(host(yd)[rows], np_pqmf(x64, fa)[:, :, 1::K], torch.float32, "pqmf_dec")
    close(host(xd.grad)[rows], np_pqmf_gx(full, fa), torch.float32, "pqmf_dec gx")
    ys = torch.randn(B, K, T // K, device=DEV, generator=g)
    xs = dsp.fuse(dsp.Interpolation(K), ip)(ys, keepdim=False)
    up = np.zeros((16, K, T))
    up[:, :, ::K] = host(ys)[rows]
    close(host(xs)[rows], np_ipqmf(up, fs), torch.float32, "interp_ipqmf")
    close(host(ip(ys, keepdim=False))[rows], np_ipqmf(host(ys)[rows], fs), torch.float32, "ipqmf")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("K,M,P,s", [(4, 40, 4, 0), (4, 62, 4, 3), (3, 7, 2, 1), (2, 11, 1, 2), (9, 20, 9, 0), (4, 130, 4, 1), (4, 40, 20, 5)])
def test_folded_routes_equal_the_module_chain(K, M, P, s, dtype):
    """fuse(pqmf, Decimation) and fuse(Interpolation, ipqmf) against the modules in sequence: outputs, input gradients and the
    learnable filters' gradients, torch.equal (a skipped tap is an exact zero product)."""
    g = torch.Generator(device=DEV).manual_seed(K * M + P + s)
    x = torch.randn(3, 1001, device=DEV, dtype=dtype, generator=g)
    pq = dsp.PQMF(K, M, learnable=True, device=DEV, dtype=dtype)
    dec = dsp.Decimation(P, s)
    res = []
    for fused in (False, True):
        pq.filters.grad = None
        xg = x.clone().requires_grad_(True)
        y = dsp.fuse(pq, dec)(xg) if fused else dec(pq(xg))
        w = torch.randn(y.shape, device=DEV, dtype=dtype, generator=torch.Generator(device=DEV).manual_seed(1))
        (y * w).sum().backward()
        res.append((y.detach(), xg.grad, pq.filters.grad.clone()))
    for a, b, name in zip(res[0], res[1], ("y", "gx", "gf")):
        assert torch.equal(a, b), ("analysis", name)
    y = torch.randn(3, K, 251, device=DEV, dtype=dtype, generator=g)
    ip = dsp.IPQMF(K, M, learnable=True, device=DEV, dtype=dtype)
    itp = dsp.Interpolation(P, s)
    res = []
    for fused in (False, True):
        ip.filters.grad = None
        yg = y.clone().requires_grad_(True)
        f = dsp.fuse(itp, ip)
        out = f(yg) if fused else ip(itp(yg))
        if fused:
            assert f.last_path == "fused"
        w = torch.randn(out.shape, device=DEV, dtype=dtype, generator=torch.Generator(device=DEV).manual_seed(2))
        (out * w).sum().backward()
        res.append((out.detach(), yg.grad, ip.filters.grad.clone()))
    for a, b, name in zip(res[0], res[1], ("x", "gy", "gf")):
        assert torch.equal(a, b), ("synthesis", name)


def test_gradcheck_float64():
    rng = np.random.default_rng(4)
    K, M, T = 3, 5, 13
    for P, s in ((1, 0), (3, 1), (2, 4)):
        x = dev(rng.standard_normal((2, T))).requires_grad_(True)
        f = dev(rng.standard_normal((K, M + 1))).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x_, f_: ops.PqmfFn.apply(x_, f_, P, s), (x, f), eps=1e-6, atol=1e-8, rtol=1e-6)
        y = dev(rng.standard_normal((2, K, 7))).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda y_, f_: ops.IpqmfFn.apply(y_, f_, P, s), (y, f), eps=1e-6, atol=1e-8, rtol=1e-6)
        z = dev(rng.standard_normal((2, 5, 3))).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda z_: ops.InterpolateFn.apply(z_, P, s, 1), (z,), eps=1e-6, atol=1e-8, rtol=1e-6)
    # the module routes, learnable filters included
    pq = dsp.PQMF(2, 6, learnable=True, device=DEV, dtype=torch.float64)
    ip = dsp.IPQMF(2, 6, learnable=True, device=DEV, dtype=torch.float64)
    x = dev(rng.standard_normal((1, 11))).requires_grad_(True)
    y = dev(rng.standard_normal((1, 2, 5))).requires_grad_(True)
    fa = dsp.fuse(pq, dsp.Decimation(2, 1))
    fs = dsp.fuse(dsp.Interpolation(2, 1), ip)
    for fn, inp in ((lambda x_: pq(x_), x), (lambda x_: fa(x_), x), (lambda y_: ip(y_), y), (lambda y_: fs(y_), y)):
        assert torch.autograd.gradcheck(fn, (inp,), eps=1e-6, atol=1e-8, rtol=1e-6)
    for m, fn in ((pq, lambda: fa(x.detach())), (ip, lambda: fs(y.detach()))):
        w0 = m.filters.detach().clone()

        def of_filters(w, m=m, fn=fn):
            with torch.no_grad():
                m.filters.copy_(w.detach())
            return fn()

        # analytic filter gradient of sum(out * v) against central differences
        m.filters.grad = None
        out = fn()
        v = torch.randn(out.shape, device=DEV, dtype=torch.float64, generator=torch.Generator(device=DEV).manual_seed(3))
        (out * v).sum().backward()
        ga = m.filters.grad.clone()
        num = torch.zeros_like(w0)
        for idx in np.ndindex(*w0.shape):
            wp, wm = w0.clone(), w0.clone()
            wp[idx] += 1e-6
            wm[idx] -= 1e-6
            num[idx] = ((of_filters(wp) * v).sum() - (of_filters(wm) * v).sum()) / 2e-6
        with torch.no_grad():
            m.filters.copy_(w0)
        assert torch.allclose(ga, num, atol=1e-7, rtol=1e-6), (ga - num).abs().max()


def test_batch_invariance_bitwise():
    g = torch.Generator(device=DEV).manual_seed(5)
    B, T, K, M = 1024, 16000, 4, 40
    x = torch.randn(B, T, device=DEV, generator=g)
    pq, ip = dsp.PQMF(K, M, device=DEV), dsp.IPQMF(K, M, device=DEV)
    fa, fs = dsp.fuse(pq, dsp.Decimation(K, 1)), dsp.fuse(dsp.Interpolation(K, 1), ip)
    y = torch.randn(B, K, T // K, device=DEV, generator=g)
    outs = {}
    for name, fn, inp in (("pqmf", pq, x), ("pqmf_dec", fa, x), ("ipqmf", ip, y), ("interp_ipqmf", fs, y)):
        a = inp.clone().requires_grad_(True)
        o = fn(a)
        w = torch.randn(o.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
        (o * w).sum().backward()
        outs[name] = (fn, inp, o.detach(), a.grad, w)
    for name, (fn, inp, o, ga, w) in outs.items():
        for r in (0, 517, 1023):
            a = inp[r:r + 1].clone().requires_grad_(True)
            o1 = fn(a)
            (o1 * w[r:r + 1]).sum().backward()
            assert torch.equal(o1[0], o[r]) and torch.equal(a.grad[0], ga[r]), (name, r)


def test_empty_noncontiguous_and_graph_capture():
    pq, ip = dsp.PQMF(4, 40, device=DEV), dsp.IPQMF(4, 40, device=DEV)
    for dt in (torch.float32, torch.float64):
        pq64, ip64 = dsp.PQMF(4, 40, learnable=True, device=DEV, dtype=dt), dsp.IPQMF(4, 40, learnable=True, device=DEV, dtype=dt)
        x = torch.empty(0, 160, device=DEV, dtype=dt, requires_grad=True)
        y = pq64(x)
        assert y.shape == (0, 4, 160)
        y.sum().backward()
        assert x.grad.shape == x.shape and bool((pq64.filters.grad == 0).all())
        z = torch.empty(0, 4, 40, device=DEV, dtype=dt, requires_grad=True)
        out = dsp.fuse(dsp.Interpolation(4), ip64)(z)
        assert out.shape == (0, 1, 160)
        out.sum().backward()
        assert z.grad.shape == z.shape and bool((ip64.filters.grad == 0).all())
        # an empty subband signal with start > 0: only zero padding is read
        e = torch.empty(2, 4, 0, device=DEV, dtype=dt)
        assert torch.equal(dsp.fuse(dsp.Interpolation(4, 3), ip64)(e), torch.zeros(2, 1, 3, device=DEV, dtype=dt))
        # a decimation start beyond the signal keeps nothing; the gradient is zero
        xs = torch.randn(2, 5, device=DEV, dtype=dt, requires_grad=True)
        yd = dsp.fuse(pq64, dsp.Decimation(4, 7))(xs)
        assert yd.shape == (2, 4, 0)
        yd.sum().backward()
        assert bool((xs.grad == 0).all())
    # non-contiguous inputs equal their contiguous copies
    big = torch.randn(4, 2002, device=DEV)
    xn = big[:, ::2]
    assert not xn.is_contiguous() and torch.equal(pq(xn), pq(xn.contiguous()))
    yn = torch.randn(2, 300, 4, device=DEV).transpose(1, 2)
    assert not yn.is_contiguous() and torch.equal(ip(yn), ip(yn.contiguous()))
    itp = dsp.Interpolation(3, 1, dim=1)
    assert torch.equal(itp(yn), itp(yn.contiguous()))
    # graph capture and replay of the subband round trip
    fa, fs = dsp.fuse(pq, dsp.Decimation(4)), dsp.fuse(dsp.Interpolation(4), ip)
    x = torch.randn(8, 4000, device=DEV)
    gr = dsp.Graphed(lambda v: fs(4 * fa(v)), x)
    x2 = torch.randn(8, 4000, device=DEV)
    assert torch.equal(gr(x2).clone(), fs(4 * fa(x2)))


def test_interpolation_any_dim_and_the_zero_last_sample():
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(3, 5, 7, device=DEV, dtype=torch.float64, generator=g)
    for P, s, dim in ((3, 0, 1), (2, 1, 0), (4, 2, -1), (1, 3, 2)):
        got = dsp.Interpolation(P, s, dim)(x)
        d = dim % 3
        shape = list(x.shape)
        shape[d] = x.shape[d] * P + s
        want = torch.zeros(shape, device=DEV, dtype=torch.float64).index_copy_(d, torch.arange(s, shape[d], P, device=DEV), x)
        assert torch.equal(got, want), (P, s, dim)
        xg = x.clone().requires_grad_(True)
        w = torch.randn(shape, device=DEV, dtype=torch.float64, generator=g)
        (dsp.functional.interpolate(xg, P, s, dim) * w).sum().backward()
        assert torch.equal(xg.grad, w[(slice(None),) * d + (slice(s, None, P),)]), (P, s, dim)
    # for P > 1 the last sample is zero, so the synthesis' replicate pad adds nothing after an interpolation
    y = torch.randn(2, 4, 50, device=DEV, generator=g)
    u = dsp.Interpolation(4, 1)(y)
    assert bool((u[..., -1] == 0).all())
    ip = dsp.IPQMF(4, 40, device=DEV)
    ext = torch.cat([u, torch.zeros(2, 4, 20, device=DEV)], dim=-1)
    assert torch.allclose(ip(u), ip(ext)[..., :u.size(-1)], atol=1e-6)


def test_decimation_returns_a_view():
    x = torch.randn(2, 4, 100, device=DEV)
    y = dsp.Decimation(4, 1)(x)
    assert y._base is x and y.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
    assert torch.equal(y, x[..., 1::4])
    z = dsp.functional.decimate(x, 2, 1, dim=1)
    assert z._base is x and torch.equal(z, x[:, 1::2])


def test_readme_subband_example(golden, tmp_path):
    """README.md:269-295 of the reference with nothing changed but the import and the device."""
    import diffsptk_amd as diffsptk

    pcm = golden("datawav")["pcm"]
    wav = str(tmp_path / "data.wav")
    diffsptk.write(wav, torch.from_numpy(pcm.astype(np.float64) / 32768.0 * (32768.0 / 32767.0)), 16000)   # (exact PCM back)

    K = 4   # Number of subbands.
    M = 40  # Order of filter.
    x, sr = diffsptk.read(wav, device="cuda")
    pqmf = diffsptk.PQMF(K, M, device="cuda")
    decimate = diffsptk.Decimation(K)
    y = decimate(pqmf(x))
    interpolate = diffsptk.Interpolation(K)
    ipqmf = diffsptk.IPQMF(K, M, device="cuda")
    x_hat = ipqmf(interpolate(K * y)).reshape(-1)
    error = (x_hat - x).abs().sum()

    z = golden("pqmf")
    ref = z["readme_x_hat"].astype(np.float64)
    got = host(x_hat)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    assert abs(float(error) - z["readme_error"][0]) <= 0.01 * z["readme_error"][0], (float(error), z["readme_error"][0])
    # the same through the folded routes
    x_hat2 = diffsptk.fuse(interpolate, ipqmf)(K * diffsptk.fuse(pqmf, decimate)(x)).reshape(-1)
    assert torch.equal(x_hat2, x_hat)
