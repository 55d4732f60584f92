"""PLP on the MI355X (csrc/plp.hip after the filter bank): the reference's goldens (tests/golden/plp.npz), its docstring example and
data.wav, the bench-size float32 batch against a float64 restatement on the device, gradcheck, fuse(stft, plp), bitwise batch
invariance, empty / multi-dimensional / non-contiguous inputs, the learnable filter bank and graph replay.

Tolerances, relative to the largest |value| of the compared tensor: outputs 1e-10 (float64) and 2e-5 (float32; the reference's
own float32 result is 2.5e-6 from its float64 one); gradients 1e-8 (float64) and 2e-3 (float32: the Levinson adjoint divides by
the prediction error, which float32 inputs perturb at 1e-7 relative)."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import functional as F, ops
from diffsptk_amd.modules import _learnable
from diffsptk_amd.utils import tables

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT_TOL = {torch.float64: 1e-10, torch.float32: 2e-5}
GRAD_TOL = {torch.float64: 1e-8, torch.float32: 2e-3}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().double().numpy()


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def golden_cases():
    import json
    import os

    api = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "plp_api.json")))
    return api["grid"], api["sample_rate"]


GRID, SR = golden_cases()


def kwargs_of(case):
    L, C, M, n_fft, lifter, cf, floor, gamma, scale, fmt, _ = case
    return dict(fft_length=L, plp_order=M, n_channel=C, sample_rate=SR, compression_factor=cf, lifter=lifter, floor=floor,
                gamma=gamma, scale=scale, n_fft=n_fft, out_format=fmt)


def spectra(rng, F_, K=257, scale=1.0):
    k = np.arange(K)[None, :]
    env = np.exp(1.5 * np.sin(k * rng.uniform(0.02, 0.3, (F_, 1)) + rng.uniform(0, 6, (F_, 1))) - 2.0 * k / K)
    return scale * env * rng.exponential(1.0, (F_, K))


def restate(x, H, table, C, M, N, cf, floor, gamma, fmt):
    """plp.py:312-320 in stock torch operators (float64, differentiable): the filter bank, then steps 2-8 with the same
    tables, Levinson-Durbin as a recursion."""
    y, E = _learnable.fbank_with_weights(x, H, floor, gamma, True)
    J = N // 2 + 1
    q, Q, cs, sn, w, lift = torch.split(table, [C, (C + 2) * (M + 1), (M + 1) * J, (M + 1) * J, J, M + 1])
    Q, cs, sn = Q.view(C + 2, M + 1), cs.view(M + 1, J), sn.view(M + 1, J)
    v = (torch.exp(y) * q) ** cf
    u = torch.cat((v[..., :1], v, v[..., -1:]), dim=-1)
    r = u @ Q
    a, err = [], r[..., 0]
    for m in range(1, M + 1):
        acc = r[..., m]
        for j in range(1, m):
            acc = acc + a[j - 1] * r[..., m - j]
        k = -acc / err
        a = [a[j - 1] + k * a[m - j - 1] for j in range(1, m)] + [k]
        err = err * (1 - k * k)
    if M:
        a = torch.stack(a, dim=-1)
        K = torch.sqrt(r[..., 0] + (r[..., 1:] * a).sum(-1))
        re = 1 + a @ cs[1:]
        im = -(a @ sn[1:])
        L = w * 0.5 * torch.log(re * re + im * im)
        c = torch.cat((torch.log(K)[..., None], L @ cs[1:].T), dim=-1) * lift
    else:
        c = torch.log(torch.sqrt(r[..., :1])) * lift
    parts = [c[..., 1:]] + ([c[..., :1]] if "c" in fmt else []) + ([E] if "E" in fmt else [])
    return torch.cat(parts, dim=-1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", range(len(GRID)), ids=[f"{c[0]}-C{c[1]}-M{c[2]}-N{c[3]}-{c[9]}" for c in GRID])
def test_reference_goldens(golden, i, dtype):
    z = golden("plp")
    kw = kwargs_of(GRID[i])
    x = dev(z[f"c{i}_x"], dtype).requires_grad_(True)
    m = dsp.PLP(**kw, device=DEV, dtype=dtype)
    y = m(x)
    want = z[f"c{i}_out_f64"]
    assert y.shape == want.shape
    e = rel_err(host(y), want)
    assert e <= OUT_TOL[dtype], e
    if dtype == torch.float32:
        assert rel_err(host(y), z[f"c{i}_out_f32"]) <= OUT_TOL[dtype]
    (y * dev(z[f"c{i}_w"], dtype)).sum().backward()
    eg = rel_err(host(x.grad), z[f"c{i}_grad_f64"])
    assert eg <= GRAD_TOL[dtype], eg
    # functional: the same launches
    kw.pop("fft_length")
    yf = F.plp(x.detach(), **kw)
    assert torch.equal(yf, y.detach())


def test_docstring_example(golden):
    z = golden("plp")
    stft = dsp.STFT(frame_length=10, frame_period=10, fft_length=32, device=DEV)
    plp = dsp.PLP(fft_length=32, plp_order=4, n_channel=8, sample_rate=8000, device=DEV)
    y = plp(stft(dev(z["doc_x"], torch.float32)))
    assert rel_err(host(y), z["doc_y"]) <= OUT_TOL[torch.float32]
    np.testing.assert_allclose(host(y), [[-0.2896, -0.2356, -0.0586, -0.0387], [0.4468, -0.5820, 0.0104, -0.0505]], atol=6e-5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_data_wav(golden, dtype):
    z = golden("plp")
    pcm = golden("datawav")["pcm"]
    x = dev(pcm.astype(np.float64) / 32768.0, dtype)
    stft = dsp.STFT(400, 80, 512, device=DEV, dtype=dtype)
    for fmt in ("yc", "ycE"):
        plp = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, lifter=22, out_format=fmt, device=DEV, dtype=dtype)
        assert rel_err(host(plp(stft(x))), z[f"wav_{fmt}_f64"]) <= OUT_TOL[dtype]
        if dtype == torch.float32:
            fused = dsp.fuse(stft, plp)
            y = fused(x)
            assert fused.last_path == ("fused" if fmt == "yc" else "two-stage")
            assert rel_err(host(y), z[f"wav_{fmt}_f64"]) <= 5 * OUT_TOL[dtype]


def test_bench_size_float32_against_a_float64_restatement():
    """204 800 frames (1024 utterances x 1 s at frame period 80), fft 512, C = 20, M = 12, lifter 22: outputs and gradients of
    the float32 kernels against stock float64 torch operators on the device."""
    rng = np.random.default_rng(11)
    Fr, C, M, N = 204800, 20, 12, 512
    x64 = dev(spectra(rng, Fr))
    m32 = dsp.PLP(fft_length=512, plp_order=M, n_channel=C, sample_rate=16000, lifter=22, out_format="ycE", device=DEV,
                  dtype=torch.float32)
    m64 = dsp.PLP(fft_length=512, plp_order=M, n_channel=C, sample_rate=16000, lifter=22, out_format="ycE", device=DEV,
                  dtype=torch.float64)
    x32 = x64.float().requires_grad_(True)
    y32 = m32(x32)
    xr = x64.clone().requires_grad_(True)
    yr = restate(xr, m64.H, m64.table, C, M, N, 0.33, 1e-5, 0.0, "ycE")
    assert rel_err(host(y32), host(yr)) <= OUT_TOL[torch.float32]
    w = dev(rng.standard_normal(tuple(yr.shape)))
    (yr * w).sum().backward()
    (y32 * w.float()).sum().backward()
    gr = host(xr.grad)
    e_rows = np.abs(host(x32.grad) - gr).max(-1) / np.maximum(np.abs(gr).max(-1), 1e-300)
    assert e_rows.max() <= GRAD_TOL[torch.float32], e_rows.max()
    # the float64 kernels against the same restatement
    y64 = m64(x64)
    assert rel_err(host(y64), host(yr)) <= OUT_TOL[torch.float64]


def test_gradcheck_float64():
    rng = np.random.default_rng(3)
    x = dev(spectra(rng, 3, 17)).requires_grad_(True)
    for fmt in ("y", "ycE"):
        torch.autograd.gradcheck(lambda t: F.plp(t, 4, 10, 16000, lifter=3, n_fft=16, out_format=fmt), (x,), eps=1e-6, atol=1e-6)
    # the tail alone, with E as an input
    m = dsp.PLP(fft_length=32, plp_order=5, n_channel=9, sample_rate=16000, n_fft=11, out_format="ycE", device=DEV,
                dtype=torch.float64)
    y, E = ops.FbankFn.apply(x.detach(), m.H, 1e-5, 0.0, True)
    y, E = y.clone().requires_grad_(True), E.clone().requires_grad_(True)
    torch.autograd.gradcheck(lambda a, b: ops.PlpFn.apply(a, b, m.table, 5, 11, 0.33, "ycE"), (y, E), eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("fmt", ["y", "yc", "yE"])
def test_fuse_stft_plp(fmt):
    rng = np.random.default_rng(7)
    stft = dsp.STFT(400, 80, 512, device=DEV)
    plp = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, lifter=22, out_format=fmt, device=DEV)
    fused = dsp.fuse(stft, plp)
    x = dev(rng.standard_normal((4, 16000)) * 0.1, torch.float32)
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    y1 = fused(x1)
    assert fused.last_path == ("two-stage" if "E" in fmt else "fused")
    y2 = plp(stft(x2))
    assert y1.shape == y2.shape
    assert rel_err(host(y1), host(y2)) <= 5 * OUT_TOL[torch.float32]
    w = dev(rng.standard_normal(tuple(y1.shape)), torch.float32)
    (y1 * w).sum().backward()
    (y2 * w).sum().backward()
    assert rel_err(host(x1.grad), host(x2.grad)) <= 5e-3
    with torch.no_grad():
        assert torch.equal(fused(x), y1.detach())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_bitwise_batch_invariance(dtype):
    """The PLP launches (forward and backward) give a frame the same bits whatever the batch around it."""
    rng = np.random.default_rng(9)
    m = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, lifter=22, out_format="ycE", device=DEV, dtype=dtype)
    y, E = ops.FbankFn.apply(dev(spectra(rng, 3000), dtype), m.H, 1e-5, 0.0, True)
    ya_in, Ea_in = y.clone().requires_grad_(True), E.clone().requires_grad_(True)
    ya = ops.PlpFn.apply(ya_in, Ea_in, m.table, 12, 512, 0.33, "ycE")
    w = dev(rng.standard_normal(tuple(ya.shape)), dtype)
    (ya * w).sum().backward()
    for lo, hi in ((0, 1), (5, 69), (2999, 3000)):
        yb_in, Eb_in = y[lo:hi].clone().requires_grad_(True), E[lo:hi].clone().requires_grad_(True)
        yb = ops.PlpFn.apply(yb_in, Eb_in, m.table, 12, 512, 0.33, "ycE")
        (yb * w[lo:hi]).sum().backward()
        assert torch.equal(yb.detach(), ya.detach()[lo:hi])
        assert torch.equal(yb_in.grad, ya_in.grad[lo:hi]) and torch.equal(Eb_in.grad, Ea_in.grad[lo:hi])


def test_empty_leading_dimensions_and_non_contiguous_inputs():
    m = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, out_format="ycE", device=DEV)
    for shape in ((0, 257), (2, 0, 257)):
        x = torch.empty(shape, device=DEV, requires_grad=True)
        y = m(x)
        assert y.shape == (*shape[:-1], 14)
        y.sum().backward()
        assert x.grad.shape == x.shape
    rng = np.random.default_rng(4)
    x = dev(spectra(rng, 24), torch.float32)
    y = m(x)
    assert torch.equal(m(x.view(2, 3, 4, 257)), y.view(2, 3, 4, 14))
    assert torch.equal(m(x[0]), y[0])                      # one frame, no batch dimension
    wide = torch.zeros(257, 24, device=DEV)
    wide.copy_(x.T)
    xt = wide.T                                             # non-contiguous view of the same values
    assert not xt.is_contiguous()
    assert torch.equal(m(xt), y)


def test_learnable_filter_bank_gradient():
    rng = np.random.default_rng(6)
    C, M, N = 20, 12, 512
    x = dev(spectra(rng, 40))
    m = dsp.PLP(fft_length=512, plp_order=M, n_channel=C, sample_rate=16000, lifter=22, out_format="yc", learnable=True,
                device=DEV, dtype=torch.float64)
    y = m(x)
    H = m.H.detach().clone().requires_grad_(True)
    yr = restate(x, H, m.table, C, M, N, 0.33, 1e-5, 0.0, "yc")
    assert rel_err(host(y), host(yr)) <= OUT_TOL[torch.float64]
    w = dev(rng.standard_normal(tuple(y.shape)))
    (y * w).sum().backward()
    (yr * w).sum().backward()
    assert rel_err(host(m.H.grad), host(H.grad)) <= GRAD_TOL[torch.float64]


def test_graph_replay():
    rng = np.random.default_rng(8)
    m = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, lifter=22, out_format="ycE", device=DEV)
    g = dsp.Graphed(m, dev(spectra(rng, 800), torch.float32))
    x2 = dev(spectra(rng, 800), torch.float32)
    assert torch.equal(g(x2).clone(), m(x2))
    stft = dsp.STFT(400, 80, 512, device=DEV)
    plp = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, lifter=22, device=DEV)
    fused = dsp.fuse(stft, plp)
    gf = dsp.Graphed(fused, dev(rng.standard_normal((4, 16000)), torch.float32))
    w2 = dev(rng.standard_normal((4, 16000)), torch.float32)
    assert torch.equal(gf(w2).clone(), fused(w2))


def test_table_dtype_follows_the_module():
    m = dsp.PLP(fft_length=512, plp_order=12, n_channel=20, sample_rate=16000, device=DEV, dtype=torch.float32)
    ref = tables.plp_table(20, 12, 512, 16000)
    assert m.table.dtype == torch.float32 and np.array_equal(host(m.table), ref.astype(np.float32))
