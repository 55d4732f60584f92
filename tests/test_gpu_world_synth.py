"""WorldSynthesis on the GPU against the reference's goldens (tests/golden/make_golden_world_synth.py; the cases and their inputs:
tests/world_synth_cases.py).  The noise is injected through the module's `_randn`, so both sides see the same numbers.

Bounds.  float64: 64 D_ulp max(1, max |ref|), D_ulp the change of the reference's own float64 result when every input moves one unit in
its last place (the kernels round at every operation of the transforms, the perturbation once).  float32: 4 E_ref (E_gsp, E_gap), the
reference's own float32 error, the largest over the cases that share an fft_length; mixed_even, whose float32 pulse list differs from
its float64 one, is compared with the reference's float32 results under the figure of mixed_odd.  Every test prints its worst figure
beside its bound before it asserts."""
import functools

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import world_synth_cases as W
from conftest import GOLDEN
from diffsptk_amd import _lib, ops

pytestmark = pytest.mark.gpu

API, Z = W.load(GOLDEN)
CASE = {c["name"]: c for c in API["cases"]}
DT = {"float32": torch.float32, "float64": torch.float64}
RUNS = [(name, dt) for name in W.CASES for dt in W.dtypes_of(name)]
KEYS = (("y", "E_ref", "D_ulp_y"), ("gsp", "E_gsp", "D_ulp_gsp"), ("gap", "E_gap", "D_ulp_gap"))


def figures(name):
    """the case whose measured figures bound `name`: mixed_even has none of its own"""
    return CASE["mixed_odd" if name == "mixed_even" else name]


def bound(name, dt, key, e_key, d_key):
    if dt == "float64":
        return 64 * figures(name)[d_key] * max(1.0, CASE[name]["max_" + key])
    if name == "mixed_even":
        return 4 * CASE["mixed_odd"][e_key]
    L = W.CASES[name]["L"]
    return 4 * max(c[e_key] for n, c in CASE.items() if W.CASES[n]["L"] == L and e_key in c)


def golden(name, dt, key):
    if name == "mixed_even" and dt == "float32":
        return Z[f"{name}_{key}32"].astype(np.float64)
    return Z[f"{name}_{key}"]


def module_of(name, dt, inject=True):
    args, kw = W.options(name)
    m = dsp.WorldSynthesis(*args, **kw, device="cuda", dtype=DT[dt])
    if inject:
        m._randn = lambda rows, cols: torch.as_tensor(W.noise(name, rows, cols)).to("cuda", DT[dt])
    return m


def tensors(name, dt, arrays=None):
    f0, ap, sp = (torch.as_tensor(a).to("cuda", DT[dt]) for a in W.shaped(name, *(arrays or W.inputs(name))))
    return f0, ap.requires_grad_(True), sp.requires_grad_(True)


def call(name, dt, m=None, t=None):
    """(y, gsp, gap, the forward's last kernel) of one forward and backward (autograd runs the backward on a thread of its own, whose
    record of the last kernel this thread does not see: test_every_launch_names_its_kernel calls those entries itself)"""
    c = W.CASES[name]
    m = m or module_of(name, dt)
    f0, ap, sp = t or tensors(name, dt)
    y = m(f0, ap, sp, **({"out_length": c["out_length"]} if "out_length" in c else {}))
    fwd = _lib.last_kernel()
    y.backward(torch.as_tensor(W.cotangent(name, tuple(y.shape))).to("cuda", DT[dt]))
    return y.detach(), sp.grad, ap.grad, fwd


@functools.lru_cache(maxsize=None)
def result(name, dt):
    return call(name, dt)


@pytest.mark.parametrize("name,dt", RUNS)
def test_pulse_lists_are_the_references(name, dt):
    c = W.CASES[name]
    f0 = torch.as_tensor(W.inputs(name)[0]).to("cuda", DT[dt])
    offsets, irec, frec, pulses = ops.world_pulses(f0, c["P"], c["sr"], c["L"], c["default_f0"])
    assert _lib.last_kernel() == "world_synth_pulses_" + ("f32" if dt == "float32" else "f64")
    suffix = "32" if dt == "float32" else ""
    index, shift = Z[f"{name}_index{suffix}"], Z[f"{name}_shift{suffix}"].astype(np.float64)
    got = irec.cpu().numpy()
    assert pulses == len(index) and np.array_equal(got[:, [1, 0]], index), (got[:, [1, 0]].tolist(), index.tolist())
    assert offsets.tolist() == [int((index[:, 0] < b).sum()) for b in range(f0.shape[0] + 1)]
    # the shift in samples; the float32 list is compared with the reference's float32 shifts
    worst = float(np.abs(frec[:, 0].double().cpu().numpy() - shift).max() * c["sr"]) if pulses else 0.0
    limit = 64 * figures(name)["D_ulp_y"] if dt == "float64" else 4 * figures(name)["E_ref"]
    print(f"{name} {dt}: {pulses} pulses, shift off by {worst:.3g} of a sample, bound {limit:.3g}")
    assert worst <= limit
    frames = got[:, 0] * (c["sr"] / c["P"]) / c["sr"]
    assert np.all(got[:, 2] <= frames + 1e-3) and np.all(got[:, 3] >= np.minimum(frames, f0.shape[1] - 1) - 1e-3) and got[:, 3].max() <= f0.shape[1] - 1
    assert set(np.unique(frec[:, 2].cpu().numpy())) <= {0.0, 1.0}


@pytest.mark.parametrize("name,dt", RUNS)
def test_parity_with_the_reference(name, dt):
    y, gsp, gap, kernels = result(name, dt)
    tag = "f32" if dt == "float32" else "f64"
    assert kernels == "world_synth_overlap_add_" + tag
    assert y.shape == golden(name, dt, "y").shape and gsp.shape == golden(name, dt, "gsp").shape
    bad = []
    for (key, e_key, d_key), got in zip(KEYS, (y, gsp, gap)):
        err = float(np.abs(got.double().cpu().numpy() - golden(name, dt, key)).max())
        lim = bound(name, dt, key, e_key, d_key)
        print(f"{name} {dt} {key}: {err:.3g}, bound {lim:.3g}")
        if not err <= lim:
            bad.append((key, err, lim))
    assert not bad, bad


def test_every_launch_names_its_kernel():
    name = "unbatched"
    c = W.CASES[name]
    p = ops._p
    for dt, code, tag in (("float32", _lib.F32, "f32"), ("float64", _lib.F64, "f64")):
        f0, ap, sp = (torch.as_tensor(a).to("cuda", DT[dt]) for a in W.inputs(name))
        offsets, irec, frec, pulses = ops.world_pulses(f0, c["P"], c["sr"], c["L"], c["default_f0"])
        m = module_of(name, dt)
        noise, tw = m._randn(pulses, c["L"]), dsp.modules.spec.device_twiddle(c["L"], f0.device, f0.dtype)
        response = torch.empty(pulses, c["L"], device="cuda", dtype=DT[dt])
        grows = torch.empty(pulses, 2, c["L"] // 2 + 1, device="cuda", dtype=DT[dt])
        gy = torch.ones(1, 600, device="cuda", dtype=DT[dt])
        ops._call("dsa_world_synth_responses", p(ap), p(sp), p(noise), p(irec), p(frec), p(offsets), p(m.dc_remover), p(tw), 1, 8, c["sr"], c["L"],
                  pulses, code, p(response), ops._stream())
        assert _lib.last_kernel() == "world_synth_responses_" + tag
        ops._call("dsa_world_synth_vjp_pulses", p(gy), p(ap), p(sp), p(noise), p(irec), p(frec), p(offsets), p(m.dc_remover), p(tw), 1, 8, 600,
                  c["sr"], c["L"], pulses, code, p(grows), ops._stream())
        assert _lib.last_kernel() == "world_synth_vjp_pulses_" + tag
        gap, gsp = torch.empty_like(ap), torch.empty_like(sp)
        ops._call("dsa_world_synth_vjp_frames", p(grows), p(ap), p(sp), p(irec), p(frec), p(offsets), 1, 8, c["L"], pulses, code, p(gap), p(gsp),
                  ops._stream())
        assert _lib.last_kernel() == "world_synth_vjp_frames_" + tag and torch.isfinite(gap).all() and torch.isfinite(gsp).all()
        y = torch.empty(1, 600, device="cuda", dtype=DT[dt])
        ops._call("dsa_world_synth_overlap_add", p(response), p(irec), p(offsets), 1, 600, c["L"], pulses, code, p(y), ops._stream())
        assert _lib.last_kernel() == "world_synth_overlap_add_" + tag
        assert torch.isfinite(response).all() and torch.isfinite(grows).all()


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_runs_agree_bitwise_and_an_utterance_is_its_own(dt):
    name = "mixed_odd"
    first, again = result(name, dt), call(name, dt)
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(a, b)
    arrays = W.inputs(name)
    index = Z[f"{name}_index" + ("32" if dt == "float32" else "")]
    rows = W.noise(name, len(index), W.CASES[name]["L"])
    for b in range(arrays[0].shape[0]):   # the utterance alone, given its own noise rows
        m = module_of(name, dt)
        own = rows[index[:, 0] == b]
        m._randn = lambda r, c, own=own: torch.as_tensor(own).to("cuda", DT[dt])
        f0, ap, sp = tensors(name, dt, [a[b:b + 1] for a in arrays])
        y = m(f0, ap, sp)
        y.backward(torch.as_tensor(W.cotangent(name, tuple(first[0].shape))[b:b + 1]).to("cuda", DT[dt]))
        assert torch.equal(y.detach(), first[0][b:b + 1]) and torch.equal(sp.grad, first[1][b:b + 1]) and torch.equal(ap.grad, first[2][b:b + 1])


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_clipped_inputs_get_exactly_zero_and_f0_no_gradient(dt):
    name = "mixed_odd"
    _, gsp, gap, _ = result(name, dt)
    _, ap, sp = W.inputs(name)
    eps, top = (float(np.float32(W.EPS)), float(np.float32(1 - W.EPS))) if dt == "float32" else (W.EPS, 1 - W.EPS)   # the clip in the dtype
    a = ap.astype(np.float64)
    low_sp, out_ap = torch.as_tensor(sp.astype(np.float64) < eps), torch.as_tensor((a < eps) | (a > top))
    assert low_sp.any() and out_ap.any()
    assert not gsp.cpu()[low_sp].any() and not gap.cpu()[out_ap].any()
    assert (gsp.cpu()[~low_sp] != 0).float().mean() > 0.5 and (gap.cpu()[~out_ap] != 0).float().mean() > 0.5   # and only there
    f0, ap_t, sp_t = tensors(name, dt)
    f0.requires_grad_(True)
    module_of(name, dt)(f0, ap_t, sp_t).sum().backward()
    assert f0.grad is None and sp_t.grad is not None


def test_views_give_the_contiguous_result():
    name, dt = "unbatched", "float64"
    want = result(name, dt)
    f0, ap, sp = (torch.as_tensor(a).to("cuda", DT[dt]) for a in W.shaped(name, *W.inputs(name)))
    wide_ap = torch.zeros(ap.shape[0], 2 * ap.shape[1] + 1, device="cuda", dtype=DT[dt])
    wide_ap[:, 1::2] = ap
    tall_sp = torch.zeros(sp.shape[1], sp.shape[0], device="cuda", dtype=DT[dt])
    tall_sp.copy_(sp.t())
    flat = torch.zeros(f0.numel() + 1, device="cuda", dtype=DT[dt])
    flat[1:] = f0   # an element-aligned slice: 8 bytes off a 16-byte boundary
    views = (flat[1:], wide_ap[:, 1::2].requires_grad_(True), tall_sp.t().requires_grad_(True))
    assert not views[1].is_contiguous() and not views[2].is_contiguous()
    got = call(name, dt, t=views)
    for a, b in zip(want[:3], got[:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_empty_and_degenerate_calls(dt):
    m = dsp.WorldSynthesis(75, 16000, 1024, device="cuda", dtype=DT[dt])
    before = _lib.last_kernel()
    for B, N in ((0, 8), (2, 0)):
        y = m(torch.zeros(B, N, device="cuda", dtype=DT[dt]), torch.zeros(B, N, 513, device="cuda", dtype=DT[dt]),
              torch.ones(B, N, 513, device="cuda", dtype=DT[dt]))
        assert y.shape == (B, N * 75) and _lib.last_kernel() == before   # no launch
    # no pulse anywhere: the reference raises inside its FFT; here zeros, with zero gradients
    assert API["no_pulse"] == "RuntimeError"
    m5 = dsp.WorldSynthesis(5, 16000, 1024, device="cuda", dtype=DT[dt])
    ap = torch.full((1, 1, 513), 0.5, device="cuda", dtype=DT[dt], requires_grad=True)
    sp = torch.ones(1, 1, 513, device="cuda", dtype=DT[dt], requires_grad=True)
    y = m5(torch.zeros(1, 1, device="cuda", dtype=DT[dt]), ap, sp)
    assert y.shape == (1, 5) and not y.any()
    y.sum().backward()
    assert not ap.grad.any() and not sp.grad.any()


@pytest.mark.parametrize("dt,last", [("float32", 8192), ("float64", 4096)])
def test_ceilings(dt, last):
    size = 4 if dt == "float32" else 8
    assert ops.world_lds_bytes(last, size) <= _lib.WORLD_MAX_LDS_BYTES < ops.world_lds_bytes(2 * last, size)
    assert W.CASES["ceiling_" + ("f32" if dt == "float32" else "f64")]["L"] == last   # its parity: test_parity_with_the_reference
    with pytest.raises(ValueError, match=f"DSA_WORLD_MAX_LDS_BYTES = {_lib.WORLD_MAX_LDS_BYTES}"):
        dsp.WorldSynthesis(75, 16000, 2 * last, device="cuda", dtype=DT[dt])
    lib = _lib.load()
    code = _lib.F32 if dt == "float32" else _lib.F64
    assert lib.dsa_world_synth_responses(None, None, None, None, None, None, None, None, 1, 4, 16000, 2 * last, 3, code, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "world_synth" in lib.dsa_last_error().decode() and "DSA_WORLD_MAX_LDS_BYTES" in lib.dsa_last_error().decode()


def test_own_noise_follows_the_device_seed():
    name, dt = "voiced_unvoiced", "float32"
    m = module_of(name, dt, inject=False)
    f0, ap, sp = (torch.as_tensor(a).to("cuda") for a in W.inputs(name))

    def run(seed, ap=ap):
        torch.manual_seed(seed)
        return m(f0, ap, sp)

    a, b, c = run(1), run(1), run(2)
    assert torch.equal(a, b) and not torch.equal(a[1], c[1])   # the unvoiced utterance is all noise
    # with ap at its floor the voiced utterance is periodic up to ap^2 = 1e-12 of the envelope: another seed changes it by less than
    # the float32 bound
    floor_ap = torch.full_like(ap, 1e-6)
    d = float((run(1, floor_ap)[0] - run(2, floor_ap)[0]).abs().max())
    lim = bound(name, dt, "y", "E_ref", "D_ulp_y")
    print(f"the all-voiced utterance at ap = 1e-6 moves by {d:.3g} with the seed, bound {lim:.3g}")
    assert d <= lim
