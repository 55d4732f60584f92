"""DynamicTimeWarping on the GPU (csrc/dtw.hip) against the goldens of the reference (tests/golden/dtw.npz, make_golden_dtw.py) and the
float64 restatement tests/dtw_ref.py, which tests/test_dtw_cpu.py pins to the same goldens.

Bounds.  float32: 4 E_ref + 1e-6 on the distance and 4 E_gref + 1e-6 on the gradients, E_ref / E_gref the reference's own float32 error
on the case (recorded by the generator, which also sizes the inputs so that the 1e-6 covers the roundings any float32 evaluation
accumulates).  float64: 1e-10 max(1, max |ref|) -- at most a few thousand accumulated roundings of 1e-16 on values up to about 1e3.
Paths are compared exactly: the generator keeps only inputs whose path the reference itself finds in both precisions, with every
decision on it won by more than 1e-4 R[end].  Every test prints its worst figure beside the bound before it asserts."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import dtw_ref
from conftest import GOLDEN
from diffsptk_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = dtw_ref.golden_cases(GOLDEN)
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def route(entry, T1, dt):
    """the kernel a shape is meant to take: one wave up to 64 rows, a workgroup beyond"""
    kind = "" if entry == "path" else ("wave_" if T1 <= 64 else "block_")
    return {"fwd": "dtw_", "bwd": "dtw_vjp_", "path": "dtw_path_"}[entry] + kind + dt


def run(x, y, lengths=None, *, metric=1, p=4, gamma=1e-3, paths=True, cot=None):
    """(distance, gx, gy, paths, (forward kernel, backward kernel or None, path kernel or None)) of one call on device tensors"""
    x, y = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    names = {}
    with torch.no_grad():   # the distance alone: the forward's kernel, before the path's launch hides it
        plain = dsp.functional.dtw(x, y, lengths, metric=metric, p=p, softness=gamma)
    names["fwd"] = _lib.last_kernel()
    hook = x.register_hook(lambda g: names.update(bwd=_lib.last_kernel()))   # the backward runs on autograd's thread: read it there
    out = dsp.functional.dtw(x, y, lengths, return_indices=paths, metric=metric, p=p, softness=gamma)
    distance, found = out if paths else (out, None)
    if paths and distance.numel():
        names["path"] = _lib.last_kernel()
    assert torch.equal(plain, distance.detach()) or bool(torch.isnan(plain).any())   # with and without the tables: the same bits
    gx = gy = None
    if distance.numel() and bool(torch.isfinite(distance).any()):
        gx, gy = torch.autograd.grad(distance, (x, y), torch.ones_like(distance) if cot is None else cot)
    else:
        gx, gy = torch.zeros_like(x), torch.zeros_like(y)
    hook.remove()
    return distance.detach(), gx, gy, found, (names["fwd"], names.get("bwd"), names.get("path"))


def run_case(c, dtype):
    as1d = c.get("docstring")
    x, y = dev(c["x"][:, 0] if as1d else c["x"][None], dtype), dev(c["y"][:, 0] if as1d else c["y"][None], dtype)
    lengths = None if c["lengths"] is None else torch.tensor([c["lengths"]], device=DEV)
    d, gx, gy, paths, names = run(x, y, lengths, metric=c["metric"], p=c["p"], gamma=c["gamma"])
    return float(d[0]), gx.double().cpu().numpy().reshape(c["x"].shape), gy.double().cpu().numpy().reshape(c["y"].shape), paths[0].cpu().numpy(), names


# ------------------------------------------------------------------ the goldens, every case in both precisions, with the routes
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_golden_parity_paths_and_routes(dt):
    dtype = DTYPES[dt]
    worst = {"distance": (0.0, None), "gradient": (0.0, None)}
    bad = []
    for c in CASES:
        d, gx, gy, path, names = run_case(c, dtype)
        cid = dtw_ref.case_id(c)
        want = (route("fwd", c["T1"], dt), None if c.get("unreachable") else route("bwd", c["T1"], dt), route("path", c["T1"], dt))
        if names != want:
            bad.append((cid, "kernels", names, want))
        if not np.array_equal(path, c["path"]):
            bad.append((cid, "path", path.tolist(), c["path"].tolist()))
        if c.get("unreachable"):
            if not (d == np.inf and not gx.any() and not gy.any() and path.tolist() == [[(c["lengths"] or [c["T1"], c["T2"]])[0] - 1,
                                                                                        (c["lengths"] or [c["T1"], c["T2"]])[1] - 1]]):
                bad.append((cid, "unreachable end", d, float(np.abs(gx).max()), float(np.abs(gy).max()), path.tolist()))
            continue
        gmax = max(np.abs(c["gx"]).max(), np.abs(c["gy"]).max())
        bd = 4 * c["e_ref"] + 1e-6 if dt == "f32" else 1e-10 * max(1.0, abs(c["distance"]))
        bg = 4 * c["e_gref"] + 1e-6 if dt == "f32" else 1e-10 * max(1.0, gmax)
        ed = abs(d - c["distance"])
        eg = max(np.abs(gx - c["gx"]).max(), np.abs(gy - c["gy"]).max())
        for key, err, bound in (("distance", ed, bd), ("gradient", eg, bg)):
            if not err <= bound:
                bad.append((cid, key, err, bound))
            if err / bound >= worst[key][0]:
                worst[key] = (err / bound, (cid, err, bound))
    for key, (share, where) in worst.items():
        print(f"dtw {dt} {key}: worst share of its bound {share:.3g} at {where}")
    assert not bad, bad[:10]


def test_unreachable_ends_in_a_batch():
    """p = 2 cannot advance j without i, p = 5 keeps to the 1:2 slope: inf, zero gradients, the one-row path -- beside a pair that arrives"""
    rng = np.random.default_rng(3)
    for dt, dtype in DTYPES.items():
        x, y = dev(rng.standard_normal((3, 4, 2)), dtype), dev(rng.standard_normal((3, 6, 2)), dtype)
        lengths = torch.tensor([[3, 4], [4, 4], [2, 6]], device=DEV)
        for p, reach in ((2, [False, True, False]), (5, [True, True, False])):
            d, gx, gy, paths, _ = run(x, y, lengths, p=p, gamma=0.1)
            print(f"dtw unreachable {dt} p={p}: distances {d.tolist()}")
            assert torch.isfinite(d).tolist() == reach and all(float(v) == np.inf for v, r in zip(d, reach) if not r)
            for b, r in enumerate(reach):
                end = (lengths[b] - 1).tolist()
                assert paths[b][-1].tolist() == end and (len(paths[b]) > 1) == r and (paths[b][0].tolist() == [0, 0]) == r
                assert bool(gx[b].any()) == r and bool(gy[b].any()) == r
            assert bool(torch.isfinite(gx).all() and torch.isfinite(gy).all())


# ------------------------------------------------------------------ a batch: per-pair lengths on the device
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shapes", [((7, 5), (5, 7), (33, 60), (3, 4), (33, 70)), ((70, 33), (65, 40), (7, 5), (63, 40), (64, 40))], ids=["wave", "block"])
def test_batch_equals_the_pairs_alone_bit_for_bit(dt, shapes):
    dtype = DTYPES[dt]
    picked = [next(c for c in CASES if (c["T1"], c["T2"]) == s and c["D"] == 5 and c["metric"] != "symmetric-kl" and not c["lengths"]) for s in shapes]
    T1, T2 = max(s[0] for s in shapes), max(s[1] for s in shapes)
    x, y = torch.zeros(5, T1, 5, dtype=dtype, device=DEV), torch.zeros(5, T2, 5, dtype=dtype, device=DEV)
    for b, c in enumerate(picked):
        x[b, :c["T1"]], y[b, :c["T2"]] = dev(c["x"], dtype), dev(c["y"], dtype)
    x[1, picked[1]["T1"]:], y[3, picked[3]["T2"]:] = float("nan"), float("inf")   # what lies beyond a pair's lengths is not read
    lengths = torch.tensor([list(s) for s in shapes], device=DEV)
    cot = dev(np.linspace(0.5, 2.0, 5), dtype)
    opts = dict(metric="euclidean", p=1, gamma=0.1)
    d, gx, gy, paths, names = run(x, y, lengths, cot=cot, **opts)
    assert names == (route("fwd", T1, dt), route("bwd", T1, dt), route("path", T1, dt))
    d2, gx2, gy2, paths2, _ = run(x, y, lengths, cot=cot, **opts)
    assert torch.equal(d, d2) and torch.equal(gx, gx2) and torch.equal(gy, gy2) and all(torch.equal(a, b) for a, b in zip(paths, paths2))
    worst = 0.0
    for b, c in enumerate(picked):
        d1, gx1, gy1, p1, _ = run(x[b:b + 1], y[b:b + 1], lengths[b:b + 1], cot=cot[b:b + 1], **opts)
        assert torch.equal(d1[0], d[b]) and torch.equal(p1[0], paths[b])
        assert torch.equal(gx1[0, :c["T1"]], gx[b, :c["T1"]]) and torch.equal(gy1[0, :c["T2"]], gy[b, :c["T2"]])
        assert not gx[b, c["T1"]:].any() and not gy[b, c["T2"]:].any()
        ref = dtw_ref.dtw(c["x"], c["y"], 1, 1, 0.1, gdistance=float(cot[b]))
        assert np.array_equal(paths[b].cpu().numpy(), ref["path"])
        if dt == "f32":   # (the goldens judge float32 values; here its bits and its paths)
            continue
        bound = 1e-10 * max(1.0, abs(ref["distance"]))
        err = max(abs(float(d[b]) - ref["distance"]), np.abs(gx[b, :c["T1"]].double().cpu().numpy() - ref["gx"]).max(),
                  np.abs(gy[b, :c["T2"]].double().cpu().numpy() - ref["gy"]).max())
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
    print(f"dtw batch {dt}: worst share of the bound {worst:.3g}")


def test_lengths_outside_the_tensors_give_nan_and_nothing_else():
    rng = np.random.default_rng(5)
    x, y = dev(rng.standard_normal((3, 4, 2))), dev(rng.standard_normal((3, 5, 2)))
    d, gx, gy, paths, _ = run(x, y, torch.tensor([[4, 5], [5, 5], [0, 3]], device=DEV), p=1, gamma=0.1)
    assert torch.isnan(d).tolist() == [False, True, True] and len(paths[0]) >= 5 and len(paths[1]) == len(paths[2]) == 0
    assert bool(gx[0].any()) and not gx[1:].any() and not gy[1:].any()


# ------------------------------------------------------------------ the size ceiling
@pytest.mark.parametrize("T1,D", [(64, 308), (1575, 1)], ids=["wave", "block"])
def test_last_shape_inside_the_lds_ceiling(T1, D):
    """T1 (D + 12) 8 bytes = DSA_DTW_MAX_LDS_BYTES less at most one row: float64, against the restatement"""
    assert T1 * (D + 12) * 8 <= _lib.DTW_MAX_LDS_BYTES < (T1 + 1) * (D + 12) * 8 and (T1 > 64 or 64 * (D + 13) * 8 > _lib.DTW_MAX_LDS_BYTES)
    rng = np.random.default_rng(T1)
    x, y = 0.1 * rng.standard_normal((T1, D)), 0.1 * rng.standard_normal((3, D))
    ref = dtw_ref.dtw(x, y, 1, 1, 0.1)
    d, gx, gy, paths, names = run(dev(x[None]), dev(y[None]), metric=1, p=1, gamma=0.1)
    assert names == (route("fwd", T1, "f64"), route("bwd", T1, "f64"), "dtw_path_f64")
    bound = 1e-10 * max(1.0, abs(ref["distance"]), np.abs(ref["gx"]).max(), np.abs(ref["gy"]).max())
    err = max(abs(float(d[0]) - ref["distance"]), np.abs(gx[0].cpu().numpy() - ref["gx"]).max(), np.abs(gy[0].cpu().numpy() - ref["gy"]).max())
    print(f"dtw ceiling ({T1}, 3, {D}) f64: error {err:.3g}, bound {bound:.3g}")
    assert err <= bound and np.array_equal(paths[0].cpu().numpy(), ref["path"])


@pytest.mark.parametrize("T1,D,dt", [(64, 309, "f64"), (1576, 1, "f64"), (64, 629, "f32"), (3151, 1, "f32")])
def test_first_shape_outside_the_lds_ceiling_raises_by_name(T1, D, dt):
    x, y = torch.zeros(1, T1, D, dtype=DTYPES[dt], device=DEV), torch.zeros(1, 3, D, dtype=DTYPES[dt], device=DEV)
    with pytest.raises(ValueError, match="DSA_DTW_MAX_LDS_BYTES = 163840"):
        dsp.functional.dtw(x, y)
    out = torch.zeros(1, dtype=DTYPES[dt], device=DEV)
    code = _lib.F32 if dt == "f32" else _lib.F64
    for rc in (_lib.load().dsa_dtw(x.data_ptr(), y.data_ptr(), None, 1, T1, 3, D, 1, 4, 1e-3, code, None, None, out.data_ptr(), None),
               _lib.load().dsa_dtw_vjp(None, None, None, None, None, None, 0, T1, 3, D, 1, 4, 1e-3, code, None, None, None),
               _lib.load().dsa_dtw_path(None, None, None, None, None, 0, T1, 3, D, 1, 4, code, None, None, None)):
        assert rc == _lib.ERR_INVALID_ARGUMENT and "DSA_DTW_MAX_LDS_BYTES (163840 bytes" in _lib.load().dsa_last_error().decode()
    inside = torch.zeros(1, T1 - 1, D, dtype=DTYPES[dt], device=DEV)
    assert float(dsp.functional.dtw(inside, y[:, :1], p=0)[0]) == 0.0


# ------------------------------------------------------------------ odds and ends
@pytest.mark.parametrize("p", [1, 4, 5])
def test_gradcheck(p):
    rng = np.random.default_rng(p)
    x, y = dev(rng.standard_normal((2, 6, 3))).requires_grad_(True), dev(rng.standard_normal((2, 5, 3))).requires_grad_(True)
    lengths = torch.tensor([[6, 5], [5, 4]], device=DEV)
    for metric in (1, 2):
        assert torch.autograd.gradcheck(lambda a, b: ops.DtwFn.apply(a, b, lengths, metric, p, 0.1, False)[0], (x, y))
    assert _lib.last_kernel() in ("dtw_wave_f64", "dtw_vjp_wave_f64")
    xp, yp = (x.detach().abs() + 0.5).requires_grad_(True), (y.detach().abs() + 0.5).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ops.DtwFn.apply(a, b, None, 3, p, 0.1, False)[0], (xp, yp))


def offset_view(t, k=1):
    """the same values, k elements into a fresh buffer: element-aligned and no more"""
    flat = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    flat[k:] = t.reshape(-1)
    return flat[k:].view(t.shape)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("T1", [33, 70])
def test_element_aligned_and_non_contiguous_tensors(dt, T1):
    rng = np.random.default_rng(T1)
    dtype = DTYPES[dt]
    x, y = dev(rng.standard_normal((3, T1, 5)), dtype), dev(rng.standard_normal((3, 41, 5)), dtype)
    lengths = torch.tensor([[T1, 41], [T1 - 2, 38], [20, 35]], device=DEV)
    base = run(x, y, lengths, p=6, gamma=0.1)
    assert bool(torch.isfinite(base[0]).all()) and base[4][0] == route("fwd", T1, dt)
    off = run(offset_view(x), offset_view(y), offset_view(lengths), p=6, gamma=0.1, cot=offset_view(torch.ones(3, dtype=dtype, device=DEV)))
    strided = run(x.transpose(1, 2).contiguous().transpose(1, 2), y.repeat_interleave(2, dim=1)[:, ::2], lengths, p=6, gamma=0.1)
    wide = torch.zeros(3, T1, 9, dtype=dtype, device=DEV)
    wide[..., 2:7] = x
    sliced = run(wide[..., 2:7], y, lengths, p=6, gamma=0.1)
    for other in (off, strided, sliced):
        assert torch.equal(other[0], base[0]) and torch.equal(other[1], base[1]) and torch.equal(other[2], base[2])
        assert all(torch.equal(a, b) for a, b in zip(other[3], base[3])) and other[4] == base[4]


def test_unbatched_shapes():
    rng = np.random.default_rng(11)
    x, y = dev(rng.standard_normal((9, 1)), torch.float32), dev(rng.standard_normal((7, 1)), torch.float32)
    full = run(x[None], y[None], p=1, gamma=0.1)
    for a, b in ((x, y), (x[:, 0], y[:, 0])):   # (T, D) and (T,)
        got = run(a, b, p=1, gamma=0.1)
        assert got[0].shape == (1,) and torch.equal(got[0], full[0]) and got[1].shape == a.shape and got[2].shape == b.shape
        assert torch.equal(got[1].reshape(-1), full[1].reshape(-1)) and torch.equal(got[2].reshape(-1), full[2].reshape(-1))
        assert torch.equal(got[3][0], full[3][0]) and got[3][0].dtype == torch.int64 and got[3][0].shape[1] == 2
    z = dsp.functional.dtw_merge(x, y, full[3][0])
    assert z.shape == (len(full[3][0]), 2) and torch.equal(z[0], torch.cat([x[0], y[0]])) and torch.equal(z[-1], torch.cat([x[-1], y[-1]]))


def test_empty_batch():
    x, y = torch.zeros(0, 4, 3, device=DEV, requires_grad=True), torch.zeros(0, 5, 3, device=DEV, requires_grad=True)
    d, paths = dsp.DynamicTimeWarping()(x, y, return_indices=True)
    assert d.shape == (0,) and paths == []
    d.sum().backward()
    assert x.grad.shape == x.shape and y.grad.shape == y.shape
    lib = _lib.load()   # a zero count is a no-op before any pointer is looked at
    assert lib.dsa_dtw(None, None, None, 0, 4, 5, 3, 1, 4, 1e-3, _lib.F32, None, None, None, None) == 0
    assert lib.dsa_dtw_vjp(None, None, None, None, None, None, 0, 4, 5, 3, 1, 4, 1e-3, _lib.F32, None, None, None) == 0
    assert lib.dsa_dtw_path(None, None, None, None, None, 0, 4, 5, 3, 1, 4, _lib.F32, None, None, None) == 0


def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(13)
    dtw = dsp.DynamicTimeWarping(p=4, softness=0.1)
    (x1, y1), (x2, y2) = ((dev(rng.standard_normal((4, 70, 5)), torch.float32), dev(rng.standard_normal((4, 50, 5)), torch.float32)) for _ in range(2))
    g = dsp.Graphed(lambda a, b: dtw(a, b), x1, y1)
    out = g(x2, y2).clone()
    eager = dtw(x2, y2)
    assert out.shape == (4,) and torch.equal(out, eager) and bool(torch.isfinite(out).all()) and not torch.equal(out, dtw(x1, y1))


@pytest.mark.parametrize("T1", [3, 65], ids=["wave", "block"])
def test_more_pairs_than_the_grid_has_workgroups(T1):
    """beyond 65 536 pairs a workgroup takes several in turn: the same bits as the pairs in two smaller batches"""
    B = (1 << 16) + 5
    g = torch.Generator(device=DEV).manual_seed(T1)
    x, y = torch.randn(B, T1, 1, device=DEV, generator=g), torch.randn(B, 4, 1, device=DEV, generator=g)
    lengths = torch.stack([torch.randint(1, T1 + 1, (B,), device=DEV, generator=g), torch.randint(1, 5, (B,), device=DEV, generator=g)], 1)
    whole = run(x, y, lengths, p=1, gamma=0.1)
    assert bool(torch.isfinite(whole[0]).all()) and whole[4][0] == route("fwd", T1, "f32")
    cut = 40000
    for sl in (slice(0, cut), slice(cut, B)):
        part = run(x[sl], y[sl], lengths[sl], p=1, gamma=0.1)
        assert torch.equal(part[0], whole[0][sl]) and torch.equal(part[1], whole[1][sl]) and torch.equal(part[2], whole[2][sl])
        assert all(torch.equal(a, b) for a, b in zip(part[3][::997], whole[3][sl][::997]))
