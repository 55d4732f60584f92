"""VectorQuantization, InverseVectorQuantization, LindeBuzoGrayAlgorithm and GaussianMixtureModeling.init_by_lbg on the device.

The codebook design against every golden of the reference (tests/golden/lbg.npz) with the module's `_randn` replaced by the recorded
draws: codebook bits, indices and iteration counts equal; every iteration's distance within 4 E_ref + 2^-24 sqrt(T) max(1, d), E_ref the
reference's own float32 error recorded by the generator and the second term what T float32 roundings of the reference's sum walk to;
kernel names in launch order; one host read per iteration.

The quantiser against a float64 composition of torch on the device.  Its float32 bounds: the loss is a float64 sum of the stored
values, scaled and rounded once: 2 * 2^-24 relative.  gx = g_xq + g_loss 2 (x - xq) / n is four float32 operations per element
(difference, product, quotient, sum; the factor 2 is exact): at most 4 * 2^-24 (|g_xq| + |g_loss 2 (x - xq) / n|)."""
import logging

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import lbg_ref
from conftest import GOLDEN
from diffsptk_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
API, CASES = lbg_ref.golden_cases(GOLDEN)
DESIGNS = [c for c in CASES if not c["warmup"]]
WARMUPS = [c for c in CASES if c["warmup"]]
DTYPES = {"f64": torch.float64, "f32": torch.float32}
EPS = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}


def case_id(c):
    return f"L{c['L']}-K{c['K']}-T{c['T']}-{c['dtype']}-seed{c['seed']}"


def dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def launches(call):
    """(what call() returns, the kernels its launches reported, in order)"""
    names, inner = [], dsp.ops.vq._call

    def recording(*args):
        inner(*args)
        names.append(_lib.last_kernel())

    dsp.ops.vq._call = recording
    try:
        return call(), names
    finally:
        dsp.ops.vq._call = inner


def recorded(draws):
    left = [np.asarray(d) for d in draws]
    return lambda rows, cols: dev(left.pop(0).reshape(rows, cols), torch.float32)


def designer(c, **override):
    init = "mean" if c["init"] is None else torch.tensor(c["init"])
    lbg = dsp.LBG(c["L"] - 1, c["K"], init=init, batch_size=c["batch_size"], device=DEV, **dict(lbg_ref.options(c), **override))
    lbg.vq.codebook.copy_(dev(c["start"], torch.float32))   # what the reference's constructor drew (init rows included)
    lbg._randn = recorded(c["draws"])
    return lbg


def data_of(c):
    x = dev(c["x"], DTYPES[c["dtype"]])
    if c["batch_size"] is None:
        return x
    return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x.cpu()), batch_size=c["batch_size"])


@pytest.mark.parametrize("c", DESIGNS, ids=case_id)
def test_design_matches_the_reference(c):
    lbg, dt, reads = designer(c), c["dtype"], []
    inner = lbg._read
    lbg._read = lambda readback: reads.append(1) or inner(readback)
    (codebook, indices, distance), names = launches(lambda: lbg(data_of(c), return_indices=True))
    assert torch.equal(codebook, dev(c["codebook"], torch.float32)) and codebook is lbg.vq.codebook
    assert torch.equal(indices, dev(c["indices"], torch.int64)) and indices.dtype == torch.int64
    assert [len(d) for d in lbg.distances] == c["iterations"]
    for mine, ref in zip(lbg.distances, c["distances"]):
        for a, b in zip(mine, ref):
            print(f"distance {a!r} reference {b!r} bound {4 * c['e_ref'] + 2.0 ** -24 * np.sqrt(c['T']) * max(1.0, b)!r}")
            assert abs(a - b) <= 4 * c["e_ref"] + 2.0 ** -24 * np.sqrt(c["T"]) * max(1.0, b)
    assert distance.dtype == DTYPES[dt] and distance.dim() == 0 and float(distance) == float(torch.tensor(lbg.distances[-1][-1], dtype=DTYPES[dt]))
    step = [f"vq_search_{dt}", f"vq_accum_{dt}", "vq_update"]
    assert names == (step[1:] if c["init"] is None else []) + step * sum(c["iterations"]) + step[:1]
    assert len(reads) == sum(c["iterations"])   # one host read per iteration
    xq, idx = lbg.transform(dev(c["x"], DTYPES[dt]))
    assert torch.equal(idx, indices) and torch.equal(xq, codebook[indices].to(DTYPES[dt]))


def test_one_host_read_per_iteration(monkeypatch):
    c = DESIGNS[3]
    lbg, x, seen = designer(c), data_of(c), {"tolist": 0, "item": 0, "cpu": 0}
    for name in seen:
        inner = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _n=name, _f=inner, **k: (seen.__setitem__(_n, seen[_n] + 1), _f(self, *a, **k))[1])
    lbg(x)
    monkeypatch.undo()
    assert seen == {"tolist": sum(c["iterations"]), "item": 0, "cpu": 0}


def test_two_runs_give_the_same_bits_and_a_seed_decides_the_draws():
    c = DESIGNS[5]   # (25, 16, 4000): several segments of the accumulation
    x = data_of(c)
    a, b = (dsp.LBG(c["L"] - 1, c["K"], n_iter=5, seed=3, device=DEV) for _ in range(2))
    (ca, ia, da), (cb, ib, db) = a(x, return_indices=True), b(x, return_indices=True)
    assert torch.equal(ca, cb) and torch.equal(ia, ib) and torch.equal(da, db) and a.distances == b.distances
    other = dsp.LBG(c["L"] - 1, c["K"], n_iter=5, seed=4, device=DEV)(x)[0]
    assert not torch.equal(other, ca)
    r1, r2 = designer(c)(x)[0].clone(), designer(c)(x)[0]   # and with the recorded draws
    assert torch.equal(r1, r2)


def test_the_docstring_example():
    """lbg.py:177-189.  Ten points and one split: which optimum K-means reaches depends on the direction of the split's draw.  Over 400
    random directions the restatement ends at distance 2.8337 (190 times), 2.8030 (133), 4.2804 (60: the docstring's) and 4.0865 (17).
    The reference's unseeded CPU generator happens to draw a direction of the third kind; the device generator does so for seed 22
    (and 49, of 0 .. 63), and then every printed decimal is reproduced, rows in the docstring's order."""
    x = torch.tensor([[-0.5, 0.3], [0.0, 0.7], [0.2, -0.1], [3.4, 2.0], [-2.8, 1.0], [2.9, -3.0], [2.2, -2.5], [1.5, -1.6], [1.8, 0.5], [1.3, 0.0]],
                     device=DEV)
    codebook, indices, distance = dsp.LBG(1, 2, seed=22, device=DEV)(x, return_indices=True)
    want = torch.tensor([[1.6250, 0.8000], [0.5833, -0.9833]], device=DEV)
    assert float((codebook - want).abs().max()) < 5e-5 and indices.tolist() == [1, 0, 1, 0, 1, 1, 1, 1, 0, 0] and abs(float(distance) - 4.2804) < 5e-5


def test_metric_and_logging(caplog):
    c = DESIGNS[3]
    lbg = designer(c, n_iter=3)
    lbg.metric, lbg.verbose = "aic", True
    with caplog.at_level(logging.INFO, logger="lbg"):
        lbg._randn = lambda rows, cols: torch.zeros(rows, cols, device=DEV) + 0.5
        lbg(data_of(c))
    text = [r.getMessage() for r in caplog.records]
    assert text[0] == "K = 1" and text[1] == "K = 2" and text[2].startswith("  iter     1: distance = ") and sum(t.startswith("  AIC = ") for t in text) == 3
    bad = designer(c, n_iter=1)
    bad.metric = "bogus"
    with pytest.raises(ValueError, match="metric bogus is not supported."):
        bad(data_of(c))


# ------------------------------------------------------------------ the quantiser and its inverse
def quantised(x, codebook):
    d = ((x.double().unsqueeze(-2) - codebook.double()) ** 2).sum(-1)
    idx = d.argmin(-1)
    return codebook[idx].to(x.dtype), idx


def draws_for(shape, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).to(DEV), torch.randn(K, shape[-1], generator=g).to(DEV)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(5,), (1, 5), (3, 7, 5), (257, 25)], ids=str)
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1000])
def test_vq_and_ivq_match_a_float64_composition(shape, K, dt):
    x, codebook = draws_for(shape, K, DTYPES[dt], 7 * K + len(shape))
    vq = dsp.VectorQuantization(shape[-1] - 1, K, device=DEV).eval()
    (xq, idx, loss), names = launches(lambda: vq(x, codebook=codebook))
    want_xq, want_idx = quantised(x, codebook)
    assert names == [f"vq_search_{dt}"] and torch.equal(vq.codebook, codebook)   # the external codebook is copied in
    assert xq.shape == x.shape and xq.dtype == x.dtype and idx.shape == x.shape[:-1] and idx.dtype == torch.int64
    assert torch.equal(idx, want_idx) and torch.equal(xq, want_xq)
    assert loss.dim() == 0 and float(loss) == 0.0 and not xq.requires_grad
    back, names = launches(lambda: dsp.InverseVectorQuantization()(idx, codebook))
    assert names == ["vq_lookup_f32"] and torch.equal(back, codebook[idx]) and back.shape == x.shape
    assert torch.equal(dsp.InverseVectorQuantization()(idx.int(), codebook), back)
    wide, names = launches(lambda: dsp.ops.vq_lookup(idx, codebook, torch.float64))   # the float64 twin: the same rows, widened exactly
    assert names == ["vq_lookup_f64"] and wide.dtype == torch.float64 and torch.equal(wide, codebook[idx].double())


def test_a_tie_gives_the_first_index():
    codebook = torch.tensor([[9.0, 9.0], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0]], device=DEV)
    x = torch.tensor([[1.5, 2.5], [9.0, 8.0], [0.0, 0.0]], device=DEV, dtype=torch.float64)
    _, idx, _ = dsp.VectorQuantization(1, 4, device=DEV).eval()(x, codebook=codebook)
    assert idx.tolist() == [1, 0, 1]
    wide = torch.zeros(130, 3, device=DEV)   # equal codewords across the search's groups of four and its staged chunks
    wide[:3] = 5.0
    _, idx, _ = dsp.VectorQuantization(2, 130, device=DEV).eval()(torch.zeros(2, 3, device=DEV), codebook=wide)
    assert idx.tolist() == [3, 3]
    nan = dsp.InverseVectorQuantization()(torch.tensor([0, 4, -1], device=DEV), codebook)   # outside the codebook: NaN, no fault
    assert torch.equal(nan[0], codebook[0]) and bool(nan[1:].isnan().all())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,K", [((5,), 3), ((3, 7, 5), 65), ((257, 25), 1000)], ids=str)
def test_training_mode_loss_and_gradient(shape, K, dt):
    x, codebook = draws_for(shape, K, DTYPES[dt], 11 * K)
    g_xq, g_loss = torch.randn_like(x), torch.tensor(1.75, device=DEV, dtype=x.dtype)
    vq = dsp.VectorQuantization(shape[-1] - 1, K, device=DEV).train()
    vq.codebook.copy_(codebook)
    want_xq, want_idx = quantised(x, codebook)
    want_loss = ((x.double() - want_xq.double()) ** 2).mean()
    term = g_loss.double() * 2 * (x.double() - want_xq.double()) / x.numel()
    rel = 1e-12 if dt == "f64" else 2 * EPS["f32"]
    for cot_xq, cot_loss in ((True, True), (True, False), (False, True)):
        xr = x.clone().requires_grad_(True)
        xq, idx, loss = vq(xr)
        assert torch.equal(xq, want_xq) and torch.equal(idx, want_idx) and not idx.requires_grad and torch.equal(vq.codebook, codebook)
        print(f"loss {float(loss.detach())!r} want {float(want_loss)!r}")
        assert loss.dim() == 0 and loss.dtype == x.dtype and abs(float(loss.detach()) - float(want_loss)) <= rel * float(want_loss)
        target = (xq * g_xq).sum() * cot_xq + loss * g_loss * cot_loss
        (gx,), names = launches(lambda: torch.autograd.grad(target, xr))
        want = g_xq.double() * cot_xq + term * cot_loss
        bound = (1e-12 if dt == "f64" else 4 * EPS["f32"]) * float((g_xq.double().abs() * cot_xq + term.abs() * cot_loss).max())
        print(f"gx error {float((gx.double() - want).abs().max())!r} bound {bound!r}")
        assert names == [f"vq_vjp_{dt}"] and float((gx.double() - want).abs().max()) <= bound


# ------------------------------------------------------------------ the accumulation and the update
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("T,K,L,min_data", [(257, 3, 5, 1), (256, 2, 64, 1), (4096, 1000, 25, 5), (1030, 70, 64, 2)], ids=str)
def test_counts_and_centroids_are_exact(T, K, L, min_data, dt):
    """x a multiple of 2^-8: every sum is exact, so the centroids are known to the bit.  (257, ...): one vector past a segment;
    (4096, 1000, 25): 13 chunks of codewords in LDS; (1030, 70, 64): the widest vector, 3 chunks"""
    g = torch.Generator().manual_seed(T + K)
    x = (torch.randint(-2047, 2048, (T, L), generator=g).double() / 256).to(DTYPES[dt]).to(DEV)
    indices = torch.randint(0, K, (T,), generator=g).to(DEV)
    indices[indices == 1] = 0   # an empty cluster
    partial = torch.arange(1.0, 4.0, device=DEV, dtype=torch.float64)
    readback = torch.empty(3, device=DEV, dtype=torch.float64)
    assert _lib.load().dsa_vq_accum_workspace_bytes(T, K, L) // (K * (L + 1) * 8) == (2 if T == 257 else 1 if T == 256 else min(-(-T // 256), 256))
    (pending, n_data), names = launches(lambda: dsp.ops.vq_accum_update(x, indices, partial, K, min_data, readback))
    counts = torch.bincount(indices, minlength=K)
    sums = torch.zeros(K, L, device=DEV, dtype=torch.float64).index_add_(0, indices, x.double())
    want = torch.where((counts >= min_data).unsqueeze(1), (sums / counts.clamp(min=1).unsqueeze(1)).float(), torch.zeros((), device=DEV))
    assert names == [f"vq_accum_{dt}", "vq_update"] and torch.equal(n_data, counts) and torch.equal(pending, want)
    assert readback.tolist() == [6.0 / T, float((counts < min_data).sum()), float((counts == counts.max()).nonzero()[0])]   # the FIRST largest
    again, _ = dsp.ops.vq_accum_update(x, indices, partial, K, min_data, readback)
    assert torch.equal(again, pending)


# ------------------------------------------------------------------ the ceiling on the vector length
def test_the_longest_vector_is_in_and_the_next_is_refused():
    last, T, K = _lib.VQ_MAX_LENGTH, 300, 4
    rng = np.random.default_rng(5)
    centres = rng.normal(size=(K, last)) * 2
    x = np.clip(np.round((centres[rng.integers(0, K, T)] + 0.3 * rng.normal(size=(T, last))) * 256), -2047, 2047) / 256
    draws = [rng.normal(size=(n, last)).astype(np.float32) for n in (1, 2)]
    start = np.zeros((K, last), dtype=np.float32)
    for dt in ("f32", "f64"):
        want = lbg_ref.design(x, start, K, 1, draws, n_iter=6, dtype=dt)
        assert want["gap"] >= 2.0 ** -40
        lbg = dsp.LBG(last - 1, K, n_iter=6, device=DEV)
        lbg._randn = recorded(draws)
        codebook, indices, _ = lbg(dev(x, DTYPES[dt]), return_indices=True)
        assert np.array_equal(codebook.cpu().numpy().view(np.int32), want["codebook"].view(np.int32)) and np.array_equal(indices.cpu().numpy(), want["indices"])
        xq, idx, _ = dsp.VectorQuantization(last - 1, K, device=DEV).eval()(dev(x, DTYPES[dt]), codebook=codebook)
        assert torch.equal(idx, indices) and torch.equal(xq, codebook[indices].to(DTYPES[dt]))
        for module in (dsp.VectorQuantization(last, K, device=DEV), dsp.LBG(last, K, device=DEV)):
            with pytest.raises(ValueError, match=f"DSA_VQ_MAX_LENGTH = {last}"):
                module(torch.zeros(T, last + 1, device=DEV, dtype=DTYPES[dt]))
    long = torch.randn(3, last + 1, device=DEV)   # the lookup has no ceiling
    assert torch.equal(dsp.InverseVectorQuantization()(torch.tensor([2, 0], device=DEV), long), long[[2, 0]])


# ------------------------------------------------------------------ GaussianMixtureModeling.init_by_lbg
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("c", WARMUPS, ids=case_id)
def test_init_by_lbg_matches_the_references_warmup(c, dt, monkeypatch):
    dtype, draws = DTYPES[dt], recorded(c["draws"])
    monkeypatch.setattr(dsp.LindeBuzoGrayAlgorithm, "_randn", lambda self, rows, cols: draws(rows, cols))
    gmm = dsp.GMM(c["L"] - 1, c["K"], device=DEV, dtype=dtype, **c["warmup"])
    x = dev(c["x"], dtype)
    gmm.init_by_lbg(x, n_iter=c["n_iter"], eps=c["eps"], perturb_factor=c["perturb_factor"])
    assert torch.equal(gmm.w, dev(c["w"], dtype)) and torch.equal(gmm.mu, dev(c["mu"], dtype))
    moments = float(np.abs(c["sigma"] + c["mu"][:, :, None] * c["mu"][:, None, :]).max())   # sigma is a difference of moments of this size
    bound = 4 * (c["e_ref_sigma"] if dt == "f32" else 0.0) + EPS[dt] * np.sqrt(c["T"]) * max(1.0, moments)
    error = float((gmm.sigma.double() - dev(c["sigma"])).abs().max())
    print(f"sigma error {error!r} bound {bound!r} E_ref {c['e_ref_sigma']!r}")
    assert error <= bound
    monkeypatch.undo()
    _, loglik = gmm(x)   # a model to train from
    assert bool(torch.isfinite(loglik))
    with pytest.raises(NotImplementedError, match="LindeBuzoGrayAlgorithm"):
        gmm.warmup(x)
