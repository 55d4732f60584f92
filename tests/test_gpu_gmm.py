"""GaussianMixtureModeling on the GPU (csrc/gmm.hip) against the goldens of the reference (tests/golden/gmm.npz, make_golden_gmm.py) and
the float64 restatement tests/gmm_ref.py, which tests/test_gmm_cpu.py pins to the same goldens.

Bounds.  float32: 4 E_ref + floor max(1, max |ref|) per quantity, E_ref the reference's own float32 error on the case and quantity and
floor = 2^-24 (sqrt(T) + sqrt(R) nmax) n_run the roundings any float32 evaluation accumulates (derived in make_golden_gmm.py, from the
shapes and the size of the log-densities alone).  float64: gmm_ref.F64_BOUND max(1, max |ref|), 16 times what the restatement itself
deviates from the reference.  Indices are compared exactly: the generator keeps transform inputs whose winner leads by 1e-2.  Every
test prints its worst share of its bound before it asserts."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import diffsptk_amd as dsp
import gmm_ref
from conftest import GOLDEN
from diffsptk_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = gmm_ref.golden_cases(GOLDEN)
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.double().cpu().numpy()


def model(c, dtype, params=None, **override):
    ubm = None if c["ubm"] is None else tuple(dev(a, dtype) for a in c["ubm"])
    opts = dict(gmm_ref.options(c), **override)
    gmm = dsp.GMM(c["L"] - 1, c["K"], ubm=ubm, device=DEV, dtype=dtype, **opts)
    gmm.set_params(tuple(dev(a, dtype) for a in (c["init"] if params is None else params)))
    return gmm


def launches(call):
    """(what call() returns, the kernels its launches reported, in order)"""
    names, inner = [], dsp.ops.gmm._call

    def recording(*args):
        inner(*args)
        names.append(_lib.last_kernel())

    dsp.ops.gmm._call = recording
    try:
        return call(), names
    finally:
        dsp.ops.gmm._call = inner


def routes(c, dt, n_run, posterior=True):
    r = "diag" if gmm_ref.is_diag(c["var_type"], c["block_size"]) else "full"
    step = [f"gmm_{entry}_{r}_{dt}" for entry in ("prepare", "estep", "accum", "update")]
    return step * n_run + (step[:2] if posterior else [])


def trained(c, dtype):
    gmm = model(c, dtype)
    ((w, mu, sigma), post, ll), names = launches(lambda: gmm(dev(c["x"], dtype), return_posterior=True))
    got = dict(w=host(w), mu=host(mu), sigma=host(sigma), posterior=host(post)[::c["post_stride"]], loglik=float(ll))
    return got, names, gmm


def bound(c, q, dt, ref, floor=None, e_ref=None):
    scale = max(1.0, float(np.abs(ref).max()))
    if dt == "f64":
        return gmm_ref.F64_BOUND * scale
    return 4 * (c["e_ref"][q] if e_ref is None else e_ref) + (gmm_ref.floor32(c) if floor is None else floor) * scale


# ------------------------------------------------------------------ the goldens, every case in both precisions, with the routes
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_golden_parity_and_routes(dt):
    worst, bad = {q: (0.0, None) for q in gmm_ref.QUANTITIES}, []
    for c in CASES:
        got, names, gmm = trained(c, DTYPES[dt])
        cid = gmm_ref.case_id(c)
        if names != routes(c, dt, c["n_run"]):
            bad.append((cid, "kernels", names, routes(c, dt, c["n_run"])))
        assert gmm.w.dtype == DTYPES[dt] and gmm.sigma.shape == (c["K"], c["L"], c["L"])
        for q in gmm_ref.QUANTITIES:
            err, b = float(np.abs(got[q] - c[q]).max()), bound(c, q, dt, c[q])
            if not err <= b:
                bad.append((cid, q, err, b))
            if err / b >= worst[q][0]:
                worst[q] = (err / b, (cid, err, b))
    for q, (share, where) in worst.items():
        print(f"gmm {dt} {q}: worst share of its bound {share:.3g} at {where}")
    assert not bad, bad[:10]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_transform_on_the_goldens(dt):
    dtype = DTYPES[dt]
    worst, bad, seen = (0.0, None), [], 0
    for c in CASES:
        params = tuple(np.asarray(c[q], dtype=np.float32).astype(np.float64) for q in ("w", "mu", "sigma"))
        for j, t in enumerate(c["transforms"]):
            gmm = model(c, dtype, params)
            (y, idx, lp), names = launches(lambda: gmm.transform(dev(c[f"t{j}_x"], dtype)))
            r = "diag" if gmm.is_diag else "full"
            want = [f"gmm_prepare_{r}_{dt}", f"gmm_estep_{r}_{dt}"] + ([f"gmm_regress_{dt}"] if t["Lx"] < c["L"] else []) + [f"gmm_transform_{dt}"]
            cid = f"{gmm_ref.case_id(c)}-Lx{t['Lx']}"
            seen += 1
            if names != want:
                bad.append((cid, "kernels", names, want))
            if idx.dtype != torch.int64 or not np.array_equal(idx.cpu().numpy(), c[f"t{j}_indices"]):
                bad.append((cid, "indices"))
            if (y is None) != (t["Lx"] == c["L"]):
                bad.append((cid, "y is None", y is None))
            pairs = [("log_prob", host(lp), c[f"t{j}_log_prob"], t["e_log_prob"])] + ([] if y is None else [("y", host(y), c[f"t{j}_y"], t["e_y"])])
            for q, a, ref, e_ref in pairs:
                err, b = float(np.abs(a - ref).max()), bound(c, q, dt, ref, gmm_ref.floor32_transform(c, t), e_ref)
                if not err <= b:
                    bad.append((cid, q, err, b))
                if err / b >= worst[0]:
                    worst = (err / b, (cid, q, err, b))
    print(f"gmm transform {dt}: {seen} runs, worst share of its bound {worst[0]:.3g} at {worst[1]}")
    assert seen >= 10 and not bad, bad[:10]


def test_transform_on_the_diagonal_route_inverts_the_block_as_it_is():
    """the diagonal route trains the diagonal only; transform inverts what set_params left beside it, symmetric or not"""
    rng = np.random.default_rng(7)
    K, L, Lx = 3, 5, 2
    w, mu = np.full(K, 1 / K), rng.normal(size=(K, L)) * 2
    sigma = np.tile(np.eye(L) * 1.5, (K, 1, 1)) + 0.2 * rng.normal(size=(K, L, L))
    x = mu[rng.integers(0, K, 80), :Lx] + 0.3 * rng.normal(size=(80, Lx))
    y_ref, idx_ref, lp_ref, gap = gmm_ref.transform(x, w, mu, sigma, True)
    gmm = dsp.GMM(L - 1, K, device=DEV, dtype=torch.float64)
    gmm.set_params((dev(w), dev(mu), dev(sigma)))
    y, idx, lp = gmm.transform(dev(x))
    err = max(np.abs(host(y) - y_ref).max(), np.abs(host(lp) - lp_ref).max())
    b = gmm_ref.F64_BOUND * max(1.0, np.abs(y_ref).max(), np.abs(lp_ref).max())
    print(f"gmm transform diag f64: error {err:.3g}, bound {b:.3g}, smallest gap {gap.min():.3g}")
    assert gap.min() > 1e-3 and np.array_equal(idx.cpu().numpy(), idx_ref) and err <= b


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("var_type", ["diag", "full"])
def test_one_vector_one_component_lands_on_the_variance_floor(dt, var_type):
    dtype = DTYPES[dt]
    x = dev([[0.5, -1.25, 2.0]], dtype)
    gmm = dsp.GMM(2, 1, n_iter=2, var_type=var_type, var_floor=1e-3, device=DEV, dtype=dtype)
    gmm.set_params((None, dev([[0.0, 0.0, 0.0]], dtype), None))
    (w, mu, sigma), post, ll = gmm(x, return_posterior=True)
    assert w.tolist() == [1.0] and torch.equal(mu, x) and post.tolist() == [[1.0]]
    assert torch.equal(sigma[0], torch.eye(3, device=DEV, dtype=dtype) * dtype_value(1e-3, dtype))
    want = -0.5 * (3 * gmm_ref.LOG_2PI + 3 * np.log(float(dtype_value(1e-3, dtype))))   # the second E-step: x on the mean
    assert abs(float(ll) - want) <= (1e-12 if dt == "f64" else 1e-5) * abs(want)


def dtype_value(v, dtype):
    return torch.tensor(v, dtype=dtype).item()


@pytest.mark.parametrize("var_type", ["diag", "full"])
def test_single_column_and_single_component(var_type):
    """L = 1 with K = 3, and K = 1 with L = 4, float64 against the restatement"""
    rng = np.random.default_rng(11)
    for L, K, T in ((1, 3, 70), (4, 1, 40)):
        x = rng.normal(size=(T, L)) + 3.0 * rng.integers(0, K, (T, 1))
        init = (np.full(K, 1.0 / K), 3.0 * np.arange(K)[:, None] + np.zeros((K, L)), np.tile(np.eye(L), (K, 1, 1)))
        ref = gmm_ref.train(x, *init, n_iter=3, eps=0.0, var_type=var_type)
        gmm = dsp.GMM(L - 1, K, n_iter=3, eps=0.0, var_type=var_type, device=DEV, dtype=torch.float64)
        gmm.set_params(tuple(dev(a) for a in init))
        (w, mu, sigma), post, ll = gmm(dev(x), return_posterior=True)
        got = dict(w=host(w), mu=host(mu), sigma=host(sigma), posterior=host(post), loglik=float(ll))
        share = max(np.abs(got[q] - ref[q]).max() / (gmm_ref.F64_BOUND * max(1.0, np.abs(ref[q]).max())) for q in gmm_ref.QUANTITIES)
        print(f"gmm {var_type} L={L} K={K} f64: worst share of the bound {share:.3g}")
        assert share <= 1.0


# ------------------------------------------------------------------ the same bits: twice, any layout, any stream, a loader
def pick(var_type, L):
    return next(c for c in CASES if c["var_type"] == var_type and c["L"] == L and not c["block_size"] and not c["alpha"] and c["T"] >= 257)


def offset_view(t, k=1):
    """the same values, k elements into a fresh buffer: element-aligned and no more"""
    flat = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    flat[k:] = t.reshape(-1)
    return flat[k:].view(t.shape)


def outputs(c, dtype, x):
    (w, mu, sigma), post, ll = model(c, dtype)(x, return_posterior=True)
    return w, mu, sigma, post, ll


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("var_type,L", [("diag", 25), ("full", 5), ("full", 50)])
def test_bits_do_not_depend_on_the_run_the_layout_the_stream_or_the_loader(dt, var_type, L):
    dtype, c = DTYPES[dt], pick(var_type, L)
    x = dev(c["x"], dtype)
    base = outputs(c, dtype, x)
    assert all(bool(torch.isfinite(t).all()) for t in base)
    wide = torch.zeros(c["T"], L + 4, dtype=dtype, device=DEV)
    wide[:, 3:3 + L] = x
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        streamed = outputs(c, dtype, x)
    torch.cuda.current_stream().wait_stream(stream)
    loader = DataLoader(TensorDataset(x.cpu()), batch_size=100, shuffle=False)   # batches of host data: moved and joined once
    others = {"again": outputs(c, dtype, x), "offset": outputs(c, dtype, offset_view(x)), "column slice": outputs(c, dtype, wide[:, 3:3 + L]),
              "row stride": outputs(c, dtype, x.repeat_interleave(2, dim=0)[::2]), "stream": streamed, "loader": outputs(c, dtype, loader)}
    for name, other in others.items():
        assert all(torch.equal(a, b) for a, b in zip(base, other)), name
    gmm = model(c, dtype, batch_size=7)   # accepted for parity, changes nothing
    assert all(torch.equal(a, b) for a, b in zip(base[:3], gmm(x)[0]))
    posterior, per_vector = gmm._e_step(x, reduction="none")
    assert torch.equal(posterior, base[3]) and per_vector.shape == (c["T"],)
    total = gmm._e_step(x)[1]
    assert total.shape == () and abs(float(total) - float(per_vector.double().sum())) <= 1e-6 * abs(float(total))


# ------------------------------------------------------------------ a covariance that is not positive definite
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bad_covariance_raises_and_the_next_call_works(dt):
    dtype = DTYPES[dt]
    c = next(c for c in CASES if c["var_type"] == "full" and c["L"] == 2 and c["K"] == 2)
    x = dev(c["x"], dtype)
    gmm = model(c, dtype)
    sigma = dev(c["init"][2], dtype)
    sigma[1] = dev([[1.0, 2.0], [2.0, 1.0]], dtype)
    gmm.set_params((None, None, sigma))
    before = [t.clone() for t in (gmm.w, gmm.mu, gmm.sigma)]
    with pytest.raises(torch.linalg.LinAlgError, match="component 1 is not positive-definite"):
        gmm(x)
    assert _lib.last_kernel() == f"gmm_update_full_{dt}"   # every launch of the iteration was made and finished
    assert all(torch.equal(a, b) for a, b in zip(before, (gmm.w, gmm.mu, gmm.sigma)))   # ... and the update left the parameters alone
    posterior, _ = gmm._e_step(x, reduction="none")   # no host read, no raise: the failed component has no share
    assert float(posterior[:, 1].abs().max()) == 0.0 and bool(torch.isfinite(posterior).all())
    good = outputs(c, dtype, x)   # the next call on the same device works
    assert np.abs(host(good[1]) - c["mu"]).max() <= bound(c, "mu", dt, c["mu"])
    diag = dsp.GMM(1, 2, device=DEV, dtype=dtype)   # the diagonal route reads the diagonal only: the same matrix is fine there
    diag.set_params((None, dev(c["init"][1], dtype), sigma))
    assert bool(torch.isfinite(diag(x)[1]))


# ------------------------------------------------------------------ the size ceiling
@pytest.mark.parametrize("dt,L", [("f64", 63), ("f32", 69)])
@pytest.mark.parametrize("var_type", ["full", "diag"])
def test_last_size_inside_the_lds_ceiling(dt, L, var_type):
    """2048 (L + 1) + L (L + 1) sizeof + 64 <= DSA_GMM_MAX_LDS_BYTES < the same at L + 1: K = 1, one iteration, against the restatement"""
    dtype, size = DTYPES[dt], 8 if dt == "f64" else 4
    assert dsp.ops.gmm_lds_bytes(L, size) <= _lib.GMM_MAX_LDS_BYTES < dsp.ops.gmm_lds_bytes(L + 1, size)
    rng = np.random.default_rng(L)
    T = L + 300
    x = np.round((rng.normal(size=(T, L)) @ (np.eye(L) + 0.3 * rng.normal(size=(L, L)) / np.sqrt(L))) * 256) / 256
    init = (np.ones(1), np.zeros((1, L)), np.eye(L)[None] * 1.25)
    ref = gmm_ref.train(x, *init, n_iter=1, var_type=var_type)
    gmm = dsp.GMM(L - 1, 1, n_iter=1, var_type=var_type, device=DEV, dtype=dtype)
    gmm.set_params(tuple(dev(a, dtype) for a in init))
    (w, mu, sigma), post, ll = gmm(dev(x, dtype), return_posterior=True)
    assert _lib.last_kernel() == f"gmm_estep_{var_type}_{dt}"
    got = dict(w=host(w), mu=host(mu), sigma=host(sigma), posterior=host(post), loglik=float(ll))
    c = dict(L=L, T=T, var_type=var_type, block_size=None, nmax=ref["nmax"], n_run=1)
    share = max(np.abs(got[q] - ref[q]).max() / bound(c, q, dt, np.asarray(ref[q]), e_ref=0.0) for q in gmm_ref.QUANTITIES)
    print(f"gmm ceiling {var_type} L={L} {dt}: worst share of the bound {share:.3g}")
    assert share <= 1.0


@pytest.mark.parametrize("dt,L", [("f64", 64), ("f32", 70)])
def test_first_size_outside_the_lds_ceiling_raises_by_name(dt, L):
    dtype = DTYPES[dt]
    x = torch.zeros(8, L, dtype=dtype, device=DEV)
    gmm = dsp.GMM(L - 1, 1, var_type="full", device=DEV, dtype=dtype)
    for call in (lambda: gmm(x), lambda: gmm.transform(x), lambda: gmm._e_step(x)):
        with pytest.raises(ValueError, match="DSA_GMM_MAX_LDS_BYTES = 163840"):
            call()
    lib, code, p = _lib.load(), _lib.F32 if dt == "f32" else _lib.F64, x.data_ptr()
    for rc in (lib.dsa_gmm_prepare(p, p, 1, L, L, 0, code, p, p, p, None),
               lib.dsa_gmm_estep(p, p, p, p, p, 8, 1, L, L, 0, code, p, p, p, None, None, None),
               lib.dsa_gmm_accum(p, p, 8, 1, L, 0, code, p, None),
               lib.dsa_gmm_update(p, None, None, None, None, p, 8, 1, L, 0, 0.0, 0.0, 0.0, code, p, p, p, None),
               lib.dsa_gmm_regress(p, 1, L + 1, L, code, p, None),
               lib.dsa_gmm_transform(p, p, p, p, 8, 1, L + 1, L, code, p, p, None)):
        assert rc == _lib.ERR_INVALID_ARGUMENT and "DSA_GMM_MAX_LDS_BYTES (163840 bytes" in lib.dsa_last_error().decode()
    y, idx, lp = gmm.transform(x[:, :L - 1])   # one column fewer is inside
    assert y.shape == (8, 1) and idx.tolist() == [0] * 8 and bool(torch.isfinite(lp).all())
