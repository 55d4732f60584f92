"""Every capped grid-stride loop of tests/grid_strides.py::CAPPED run past its cap on the MI355X.

A launcher clamps its grid to a constant; a batch above it sends a workgroup (or a wave) through the kernel's loop body again, where
LDS of the row before, a register carry, a barrier behind a `continue`, a flag or a narrow index can go wrong unseen by every batch
that fits the grid.  Each case takes 251 distinct rows (utterances) from the family's own benign generator, runs the public call on
them -- one trip for every workgroup -- and on B = rows(cap) + 3 rows gathered with idx[f] = f % 251 (251 is prime and divides no
cap: the two rows a workgroup takes in consecutive trips differ), and asserts

  bits      every one of the B output rows, and of the B gradient rows, equals row idx[f] of the 251-row call (one torch.equal against
            small[idx]); where the header promises nothing about the batch, the big call equals two calls on slices under the cap,
            its first and last 502 rows are held to the float64 reference themselves, and the equality with small[idx] is asserted too
  float64   the 251-row result against the family's float64 reference at the family's own bound (both imported from the family's
            test file or tests/*_ref.py: no tolerance is defined here)
  flags     for a device flag (lpc2lsp `failed`; lpccheck, mlsacheck `unstable`): the only offending row in a second trip is seen
            (warn_type="exit" raises; lpc2lsp's row is NaN and the flag set), and a batch without one raises nothing
  route     `_lib.last_kernel()` -- for a backward on autograd's thread -- names the case's kernel route

and prints kernel, cap, B, trips and rows compared before it asserts."""
import math
import time

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
import diffsptk_amd.functional as DF
from diffsptk_amd import _lib, ops
from diffsptk_amd.utils import tables
from oracle import oracle as O
from oracle import torch_port as TP

import grid_strides as GS
import istft_ref
import kernel_routes as KR
import paramgen_ref
import routes_ref as R
import test_gpu_excite as TE
import test_gpu_istft as TI
import test_gpu_lpc_fused as TL
import test_gpu_lsp as TS
import test_gpu_mlsacheck as TM
import test_gpu_paramgen as TG
import test_gpu_parcor as TC
import test_gpu_routes as TR
from test_gpu_parity import spec_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f64": torch.float64, "f32": torch.float32}
EPS32 = float(np.finfo(np.float32).eps)
N0 = GS.PRIME


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def rel(got, ref):
    """largest |got - ref| of the tensor, relative to its largest |ref|"""
    return amax(got.double().cpu() - ref.double()) / max(amax(ref.double()), 1e-300)


def rel_rows(got, ref):
    ref = ref.double()
    return float(((got.double().cpu() - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-300)).max())


class Prepared:
    """one case in one dtype: `inputs` (host tensors of 251 rows; the first `n_grad` get a gradient in a backward case), `call` on
    the device tensors -> tensor or tuple, `cots` (host cotangents of 251 rows, one per output), `judge(outs, grads)` -> [(what, error,
    bound)] of the 251-row result (host tensors), `judge_rows(idx, outs, grads)` -> the same for gathered rows (unpromised families)"""

    def __init__(self, inputs, call, judge, cots=None, n_grad=1, flag=None, entry=None):
        self.inputs, self.call, self.judge, self.cots, self.n_grad, self.flag, self.entry = inputs, call, judge, cots, n_grad, flag, entry


# ------------------------------------------------------------------ the families
def fam_mlsacheck(shape, dt, when):
    M, mode, n_fft = shape["M"], shape["mode"], shape["n_fft"]
    rng = np.random.default_rng(5000 + 7 * M + n_fft)
    allrows = torch.tensor(TM.rough_mc(rng, 3 * N0, M, TM.ALPHA, TM.THR, mode, n_fft))   # every third row is moved by the check
    x = allrows[:N0].to(dt)
    w = torch.tensor(rng.standard_normal((N0, M + 1)).astype(np.float16).astype(np.float64)).to(dt)

    def call(t, warn="ignore"):
        return DF.mlsacheck(t, alpha=TM.ALPHA, threshold=TM.THR, n_fft=n_fft, warn_type=warn, **TM.MODES[mode])

    def judge(outs, grads):
        xr = x.double().clone().requires_grad_()
        y = TM.re_mlsacheck(xr, TM.ALPHA, TM.THR, mode, n_fft)
        (y * w.double()).sum().backward()
        out_tol, grad_tol = (TM.OUT64, TM.GRAD64) if dt == torch.float64 else (2 * EPS32, 2 * EPS32)
        rows = [("out", rel(outs[0], y.detach()), out_tol)]
        return rows + ([("grad", rel(grads[0], xr.grad), grad_tol)] if grads else [])

    moved = torch.tensor(TM.moved_rows(allrows.numpy(), TM.ALPHA, TM.THR, mode, n_fft))
    assert bool(moved[::3].all()) and not bool(moved[1::3].any()) and not bool(moved[2::3].any())
    flag = dict(good=allrows[~moved][:N0].to(dt), bad=allrows[0].to(dt), run=lambda t: call(t, "exit"), text="Detected unstable MLSA filter.")
    return Prepared([x], call, judge, [w], flag=flag)


def excite_float64(p, P):
    """csrc/excite.hip's head comment restated: per voiced frame the pitch goes linearly to the next frame's (its own where that
    is unvoiced or missing), the phase is the running sum of 1 / pitch from the first sample of the voiced run, out = sin(2 pi phase)"""
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros((p.shape[0], p.shape[1] * P))
    for u in range(p.shape[0]):
        phase = 0.0
        for n in range(p.shape[1]):
            a = p[u, n]
            if a == 0:
                phase = 0.0
                continue
            nx = p[u, n + 1] if n + 1 < p.shape[1] else 0.0
            b = nx if nx != 0 else a
            for j in range(P):
                phase += 1.0 / (a + (j / P) * (b - a))
                out[u, n * P + j] = math.sin(2 * math.pi * phase)
    return out


def fam_excite(shape, dt, when):
    N, P = shape["N"], shape["P"]
    rng = np.random.default_rng(81)
    p = np.stack([TE.track(rng, N) for _ in range(N0)])
    p[:, -1] = np.where(p[:, -1] == 0, rng.uniform(20.0, 400.0, N0).astype(np.float32), p[:, -1])   # ends voiced: the run's sum is not zero
    p[::2, 0] = np.where(p[::2, 0] == 0, rng.uniform(20.0, 400.0, (N0 + 1) // 2).astype(np.float32), p[::2, 0])   # ... and begins voiced
    assert (p == 0).any() and ((p[:, 1:-1] == 0).any(-1) & (p[:, 0] != 0)).any()   # unvoiced gaps inside voiced utterances too
    x = torch.tensor(p).to(dt)

    def call(t):
        return DF.excite(t, P, voiced_region="sinusoidal", unvoiced_region="zeros", polarity="bipolar", init_phase=0.0)

    def judge(outs, grads):
        ref = excite_float64(x.double().numpy(), P)
        y = outs[0].double().numpy()
        if dt == torch.float32:   # tests/test_gpu_excite.py: 4 E_ref + 1e-6 with E_ref the reference's own float32 error -- here taken as 0
            return [("out", float(np.abs(y - ref).max()), 1e-6)]
        return [("out", float((np.abs(y - ref) / (1e-8 + 1e-5 * np.abs(ref))).max()), 1.0)]   # (its allclose(rtol=1e-5, atol=1e-8), as a share)

    return Prepared([x], call, judge)


def fam_lpc2lsp(shape, dt, when):
    M = shape["M"]
    rng = np.random.default_rng(2000 + M)
    a = TS.re_lsp2lpc(torch.tensor(TS.benign_lsp(rng, N0, M))).to(dt)
    w = torch.tensor(rng.standard_normal((N0, M + 1)).astype(np.float16).astype(np.float64)).to(dt)

    def judge(outs, grads):
        lsp = torch.tensor(TS.re_lpc2lsp(a.double().numpy()))
        assert not torch.isnan(lsp).any()
        scale = torch.maximum(lsp[:, :1].abs().amax(-1), torch.tensor(math.pi))
        rows = [("out", float(((outs[0].double() - lsp).abs().amax(-1) / scale).max()), TS.OUT64 if dt == torch.float64 else 2 * EPS32)]
        if grads and dt == torch.float64:   # (float32 gradients: finite, as tests/test_gpu_lsp.py::test_tile_and_dispatch_edges)
            rows.append(("grad", rel(grads[0], TS.re_lpc2lsp_grad(lsp, w.double())), TS.GRAD64))
        elif grads:
            assert bool(torch.isfinite(grads[0]).all())
        return rows

    bad = a[0].clone()
    bad[1:] = torch.tensor([0.0, 3.0], dtype=dt)   # 1 + 3 z^-2: roots outside the unit circle, no minimum-phase predictor
    return Prepared([a], lambda t: DF.lpc2lsp(t), judge, [w], flag=dict(good=a, bad=bad, detect=lambda t: ops.lpc2lsp(t, detect=True)))


def fam_parcor(shape, dt, when):
    op, M = shape["op"], shape["M"]
    rng = np.random.default_rng(1000 + M)
    a_bad, k_bad = TC.benign_rows(rng, N0, M, unstable_every=3)
    stable = torch.tensor(TC.benign_rows(rng, N0, M)[0]).to(dt)
    x = {"lpc2par": stable, "par2lpc": torch.tensor(k_bad).to(dt), "lpccheck": torch.tensor(a_bad).to(dt)}[op]
    w = torch.tensor(rng.standard_normal((N0, M + 1)).astype(np.float16).astype(np.float64)).to(dt)
    calls = {"lpc2par": lambda t: DF.lpc2par(t, gamma=0.9), "par2lpc": lambda t: DF.par2lpc(t, gamma=0.9), "lpccheck": lambda t: DF.lpccheck(t, 0.01, "ignore")}
    refs = {"lpc2par": lambda t: TC.re_step_down(t, 0.9), "par2lpc": lambda t: TC.re_step_up(t, 0.9), "lpccheck": lambda t: TC.re_check(t, 0.99, dt)}

    def judge(outs, grads):
        xr = x.double().clone().requires_grad_()
        y = refs[op](xr)
        (y * w.double()).sum().backward()
        rows = [("out", rel_rows(outs[0], y.detach()), TC.OUT64 if dt == torch.float64 else 2 * EPS32)]
        if grads and dt == torch.float64:   # (float32 gradients: finite, as tests/test_gpu_parcor.py::test_tile_and_dispatch_edges)
            rows.append(("grad", rel(grads[0], xr.grad), TC.GRAD64))
        elif grads:
            assert bool(torch.isfinite(grads[0]).all())
        return rows

    flag = dict(good=stable, bad=torch.tensor(a_bad[0]).to(dt), run=lambda t: DF.lpccheck(t, 0.01, "exit"), text="Detected unstable LPC coefficients.")
    return Prepared([x], calls[op], judge, [w], flag=flag if op == "lpccheck" else None)


def fam_mcpf(shape, dt, when):
    M, o = shape["M"], (shape["alpha"], shape["beta"], shape["onset"], shape["ir_length"])
    rng = np.random.default_rng(7)
    decay = (0.5 * np.exp(-np.arange(M + 1) / 6.0)).astype(np.float32)   # the cepstrum-like rows of tests/golden/make_golden_paramgen.py
    mc = rng.standard_normal((N0, M + 1)).astype(np.float32) * decay
    mc[..., 0] = 2 + 0.3 * mc[..., 0] / decay[0]
    g = rng.standard_normal((N0, M + 1)).astype(np.float32)
    x, w = torch.tensor(mc).to(dt), torch.tensor(g).to(dt)

    def judge(outs, grads):
        b = TG.bound(dt, 0.0)   # (4 E_ref + 1e-6 with the reference's own float32 error E_ref taken as 0; float64: 1e-10)
        rows = [("out", float(np.abs(outs[0].double().numpy() - paramgen_ref.mcpf(mc, *o)).max()), b)]
        return rows + ([("grad", float(np.abs(grads[0].double().numpy() - paramgen_ref.mcpf_grad(mc, g, *o)).max()), b)] if grads else [])

    return Prepared([x], lambda t: DF.mcpf(t, *o), judge, [w])


def fam_stft(shape, dt, when):
    L, P, nfft, T = shape["L"], shape["P"], shape["nfft"], shape["T"]
    g = torch.Generator().manual_seed(L + P + T)
    x = torch.randn(N0, T, generator=g)
    cot = torch.randn(N0, (T - 1) // P + 1, nfft // 2 + 1, generator=g)
    st = dsp.STFT(L, P, nfft, device=DEV)
    bound = 2e-6 if nfft == 512 else 3e-6   # tests/test_gpu_stft_bwd.py; tests/test_gpu_stft_big.py (test_gpu_alignment.py cites both)

    def judge_rows(idx, outs, grads):
        xs, cs = x[idx], cot[idx]
        spec_close(outs[0].numpy(), O.stft(xs.double().numpy(), L, P, nfft))   # (asserts: tests/test_gpu_parity.py's rule for spectra)
        if not grads:
            return [("out", 0.0, 0.0)]
        xr = xs.double().clone().requires_grad_(True)
        (TP.stft_power(xr, L, P, nfft) * cs.double()).sum().backward()
        if nfft == 512:
            return [("grad", float(((grads[0].double() - xr.grad).abs().amax(-1) / xr.grad.abs().amax(-1)).max()), bound)]
        return [("grad", rel(grads[0], xr.grad), bound)]

    p = Prepared([x], lambda t: st(t), lambda outs, grads: judge_rows(torch.arange(N0), outs, grads), [cot])
    p.judge_rows = judge_rows
    return p


def fam_unframe(shape, dt, when):
    L, P, N = shape["L"], shape["P"], shape["N"]
    y = istft_ref.frames(L + P, N0, N, L).to(dt)
    unf = dsp.Unframe(L, P, window="blackman", norm="power", device=DEV, dtype=dt)

    def judge_rows(idx, outs, grads):
        ref, d = istft_ref.reference_unframe(y[idx].double(), P, True, "blackman", "power", None)
        return [("out", istft_ref.weighted_ratio(outs[0], ref, d), TI.bounds(dt, istft_ref.GENERIC)[0])]

    p = Prepared([y], lambda t: unf(t), lambda outs, grads: judge_rows(torch.arange(N0), outs, grads))
    p.judge_rows = judge_rows
    return p


def fam_window(shape, dt, when):
    L = shape["L"]
    g = torch.Generator().manual_seed(L)
    x, gy = torch.randn(N0, L, generator=g, dtype=torch.float64).to(dt), torch.randn(N0, L, generator=g, dtype=torch.float64).to(dt)
    win = dsp.Window(L, device=DEV, dtype=dt)
    w = win.window.detach().cpu()

    def judge_rows(idx, outs, grads):
        # one product per element: the float64 product rounded once (tests/test_gpu_alignment.py::test_window_forward_and_backward)
        assert torch.equal(outs[0], (x[idx].double() * w.double()).to(dt))
        if grads:
            assert torch.equal(grads[0], (gy[idx].double() * w.double()).to(dt))
        return [("out", 0.0, 0.0)]

    p = Prepared([x], lambda t: win(t), lambda outs, grads: judge_rows(torch.arange(N0), outs, grads), [gy])
    p.judge_rows = judge_rows
    return p


def fam_frame(shape, dt, when):
    L, P, T = shape["L"], shape["P"], shape["T"]
    x = torch.randn(N0, T, generator=torch.Generator().manual_seed(T)).to(dt)
    fr = dsp.Frame(L, P)

    def judge_rows(idx, outs, grads):   # framing copies: exact (tests/test_gpu_parity.py::test_frame_big_matches_oracle)
        assert np.array_equal(outs[0].numpy().astype(np.float64), O.frame(x[idx].double().numpy(), L, P))
        return [("out", 0.0, 0.0)]

    p = Prepared([x], lambda t: fr(t), lambda outs, grads: judge_rows(torch.arange(N0), outs, grads))
    p.judge_rows = judge_rows
    return p


def fam_griffin(shape, dt, when):
    N, n_iter = shape["N"], shape["n_iter"]
    y = torch.tensor(np.random.default_rng(9).exponential(1.0, (N0, N, 257))).to(dt)
    gl = dsp.GriffinLim(400, 80, 512, n_iter=n_iter, init_phase="zeros", device=DEV, dtype=dt)
    tol = 1e-9 if dt == torch.float64 else 2e-3   # tests/test_gpu_parity.py::test_griffin_lim_golden: of the waveform's peak

    def judge_rows(idx, outs, grads):
        ref = torch.tensor(O.griffin(y[idx].double().numpy(), 400, 80, 512, out_length=N * 80, n_iter=n_iter))
        return [("out", float(((outs[0].double() - ref).abs().amax(-1) / ref.abs().amax(-1)).max()), tol)]

    p = Prepared([y], lambda t: gl(t, out_length=N * 80), lambda outs, grads: judge_rows(torch.arange(N0), outs, grads), entry="dsa_griffin_update")
    p.judge_rows = judge_rows
    return p


def fam_lpc_exact(shape, dt, when):
    T = shape["T"]
    x = torch.randn(N0, T, generator=torch.Generator().manual_seed(T + 1))
    fl = dsp.fuse(*TL._mods(400, 80), exact_lag_sums=True)

    def call(t):
        with torch.no_grad():
            return fl(t)

    def judge_rows(idx, outs, grads):   # tests/test_gpu_alignment.py::test_fused_lpc_forward_and_backward: 2e-5 of max(1, largest)
        y64 = TL._chain64(x[idx].to(DEV), 400, 80)[0].cpu()
        return [("out", amax(outs[0].double() - y64) / max(1.0, amax(y64)), 2e-5)]

    p = Prepared([x], call, lambda outs, grads: judge_rows(torch.arange(N0), outs, grads))
    p.judge_rows = judge_rows
    return p


_KR_CASES = {}


def kr_case(case_id):
    if not _KR_CASES:
        _KR_CASES.update({KR.case_id(route, c): (route, c) for route, c in KR.all_cases()})
    return _KR_CASES[case_id]


def fam_routes(shape, dt, when):
    """a case of tests/kernel_routes.py at 251 rows: its call (tests/test_gpu_routes.py::CALLS), its inputs and float64 restatement
    (tests/routes_ref.py) and its bound (kernel_routes.tolerance)"""
    if "spec" in shape:   # a shape no case of that table has, under a family's own bound (a name of tests/kernel_routes.py)
        call_name, tol_name, spec_args = shape["spec"]
        route, c0 = None, KR.case(call_name, when, (("f32",) if dt == torch.float32 else ("f64",)), wrt=tuple(shape["rows"]) if when == "bwd" else (),
                                  **getattr(KR, tol_name), **dict(spec_args))
    else:
        route, c0 = kr_case(shape["like"])
    args = dict(c0["args"], **({shape["batch"]: N0} if shape["batch"] else {}))
    c = dict(c0, args=args, when=when, wrt=c0["wrt"] if when == "bwd" else ())
    assert when == "bwd" or c0["when"] == "fwd" or c0["tol_from"] != KR.MEAS, "a measured bound of gradients says nothing about the outputs"
    given = R.inputs_of(c, dt) if shape["batch"] else {"x": R.gauss(77, N0, args["T"], 5).to(dt)}
    names = list(shape["rows"]) + [k for k in given if k not in shape["rows"]]   # per-row tensors first, the shared ones behind
    assert tuple(names[:len(c["wrt"])]) == tuple(c["wrt"]) or when == "fwd", (names, c["wrt"])
    shared = {k: given[k].to(DEV) for k in names[len(shape["rows"]):]}

    def call(*rows):
        t = dict(shared, **dict(zip(shape["rows"], rows)))
        a = dict(args, **({shape["batch"]: rows[0].size(0)} if shape["batch"] else {}))
        return TR.CALLS[c["call"]](t, **a)

    tol = KR.tolerance(route, c0, "f32" if dt == torch.float32 else "f64")

    def judge(outs, grads):
        ref = R.evaluate(c, {k: v.double() for k, v in given.items()})
        got = grads if when == "bwd" else outs
        assert len(got) == len(ref)
        return [(f"{'grad' if when == 'bwd' else 'out'}{i}", R.error(g, r, c["metric"]), tol) for i, (g, r) in enumerate(zip(got, ref))]

    cots = None
    if when == "bwd":
        with torch.no_grad():
            out = call(*[given[k].to(DEV) for k in shape["rows"]])
        cots = [g.to(dt) for g in R.cotangents(list(out) if isinstance(out, (tuple, list)) else [out], dt)]
    return Prepared([given[k] for k in shape["rows"]], call, judge, cots, n_grad=len(c["wrt"]))


def fam_mgcep_step_h(shape, dt, when):
    """the step's adjoint on binary16 images (dsa_mgcep_step_bwd_h) against the float64 restatement of the step (tests/routes_ref.py)
    at the bound tests/test_gpu_configs.py::test_mgcep_step_adjoint_on_binary16_splits_against_the_float32_kernel holds it to"""
    c = KR.case("mgcep_step", "bwd", KR.F32, wrt=("x", "b1"), tol=(None, 3e-6), tol_from="-", nfft=512, M=24, gamma=-0.5, F=N0)
    given = R.inputs_of(c, dt)
    mg = dsp.MelGeneralizedCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, gamma=-0.5, n_iter=1, device=DEV)
    images = TR.on_device(tables.mgcep_step_images(512, 24, 0.42), torch.zeros(1, device=DEV))

    def call(x, b1):
        return ops.MgcepStepFn.apply(x, b1, images, mg.step_images_bwd, -0.5)

    def judge(outs, grads):
        ref = R.evaluate(c, {k: v.double() for k, v in given.items()})
        return [(f"grad{i}", rel_rows(g, r), 3e-6) for i, (g, r) in enumerate(zip(grads, ref))]

    with torch.no_grad():
        out = call(given["x"].to(DEV), given["b1"].to(DEV))
    return Prepared([given["x"], given["b1"]], call, judge, [g.to(dt) for g in R.cotangents(list(out), dt)], n_grad=2)


FAMILIES = {"mlsacheck": fam_mlsacheck, "excite": fam_excite, "lpc2lsp": fam_lpc2lsp, "parcor": fam_parcor, "mcpf": fam_mcpf, "stft": fam_stft,
            "unframe": fam_unframe, "window": fam_window, "frame": fam_frame, "griffin": fam_griffin, "lpc_exact": fam_lpc_exact,
            "routes": fam_routes, "mgcep_step_h": fam_mgcep_step_h}


# ------------------------------------------------------------------ one run of a call: outputs, gradients, route names
class _Recorder:
    """the loaded library, noting the name of every entry that is looked up on it (as tests/test_gpu_alignment.py)"""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        if name.startswith("dsa_"):
            self.names.add(name)
        return getattr(self._lib, name)


def run(p, when, inputs, cots):
    """(outputs, gradients, forward route, backward route) on the device; the backward's name is read on autograd's thread"""
    xs = [t.requires_grad_(when == "bwd" and i < p.n_grad) for i, t in enumerate(inputs)]
    if when == "fwd":
        with torch.no_grad():
            out = p.call(*xs)
        return (list(out) if isinstance(out, (tuple, list)) else [out]), [], _lib.last_kernel(), None
    names = []
    hook = xs[0].register_hook(lambda g: names.append(_lib.last_kernel()))
    out = p.call(*xs)
    fwd = _lib.last_kernel()
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    grads = torch.autograd.grad(outs, xs[:p.n_grad], cots)
    hook.remove()
    return [o.detach() for o in outs], list(grads), fwd, names[0]


def gather(tensors, idx):
    return [t.to(DEV)[idx] for t in tensors]


CASES = [pytest.param(kernel, c, dt, id=GS.case_id(kernel, c) + "-" + dt) for kernel, e in GS.CAPPED.items() for c in e["cases"] for dt in c["dtypes"]]


@pytest.mark.parametrize("kernel,c,dt", CASES)
def test_second_trip_gives_the_first_trip_s_bits_and_meets_float64(kernel, c, dt):
    entry, when, t0 = GS.CAPPED[kernel], c["when"], time.perf_counter()
    p = FAMILIES[c["family"]](c["shape"], DT[dt], when)
    want = c["route"].format(dt=dt)
    lib = _lib.load()
    rec = _Recorder(lib)
    _lib._lib = rec
    try:
        small = run(p, when, [t.to(DEV) for t in p.inputs], [t.to(DEV) for t in p.cots] if when == "bwd" else None)
        bigs = []
        for B in GS.batches(entry, c):
            idx = torch.arange(B, device=DEV) % N0
            big = run(p, when, gather(p.inputs, idx), gather(p.cots, idx) if when == "bwd" else None)
            n_rows = GS.rows_of_cap(entry, c)
            # the report first: whatever is asserted from here on (inside the families' judges too) fails below this line
            print(f"{kernel} [{GS.case_id(kernel, c)}-{dt}]: cap {entry['cap']} x {entry['trip']} {entry['unit']} = {n_rows} rows, B = {B}, "
                  f"trips {-(-B // n_rows)}, rows compared {B} x {len(big[0]) + len(big[1])} tensors, routes {big[2]} / {big[3]}")
            if c["promised"]:
                same = [torch.equal(b, s[idx]) for b, s in zip(big[0] + big[1], small[0] + small[1])]
            else:   # no promise about the batch: two calls on slices that stay under the cap, and every row to float64 below
                cut = B // 2
                assert cut < n_rows and B - cut < n_rows
                parts = [run(p, when, gather(p.inputs, idx[sl]), gather(p.cots, idx[sl]) if when == "bwd" else None) for sl in (slice(0, cut), slice(cut, B))]
                same = [torch.equal(b, torch.cat([lo, hi])) for b, lo, hi in zip(big[0] + big[1], parts[0][0] + parts[0][1], parts[1][0] + parts[1][1])]
            bigs.append((B, idx, big, same))
    finally:
        _lib._lib = lib
    figures = p.judge([o.cpu() for o in small[0]], [g.cpu() for g in small[1]])
    for B, idx, big, same in bigs:
        if not c["promised"]:   # rows of the big call itself against float64: both ends of the batch (the last rows are a later trip's)
            rows = torch.cat([torch.arange(0, min(B, 2 * N0)), torch.arange(B - 2 * N0, B)]) if B > 4 * N0 else torch.arange(B)
            figures += p.judge_rows(idx.cpu()[rows], [o[rows].cpu() for o in big[0]], [g[rows].cpu() for g in big[1]])
            figures.append(("rows equal to small[idx] as well", 0.0 if all(torch.equal(b, s[idx]) for b, s in zip(big[0] + big[1], small[0] + small[1])) else 1.0, 0.0))
    print(f"    [{GS.case_id(kernel, c)}-{dt}] " + ", ".join(f"{what} {err:.3g} (bound {bound:.3g})" for what, err, bound in figures)
          + f"; {time.perf_counter() - t0:.3f} s")
    for B, idx, big, same in bigs:
        assert all(same), (B, same)
        assert big[2] == (c.get("fwd_route", big[2]) if when == "bwd" else want), big[2]
        assert when == "fwd" or big[3] == want, big[3]
        assert all(bool(torch.isfinite(t).all()) for t in big[0] + big[1])
    if p.entry:
        assert p.entry in rec.names, sorted(rec.names)
    for what, err, bound in figures:
        assert err <= bound, (what, err, bound)
    if c.get("flag"):
        check_flag(entry, c, p)


def check_flag(entry, c, p):
    """the device flag with the only offending row in a second trip, and without one"""
    n_rows = GS.rows_of_cap(entry, c)
    B = n_rows + 3
    idx = torch.arange(B, device=DEV) % N0
    good = p.flag["good"].to(DEV)[idx]
    bad = good.clone()
    bad[n_rows + 1] = p.flag["bad"].to(DEV)
    if c["flag"] == "failed":   # lpc2lsp: the row comes back as NaN behind its gain, the flag is set, and no other row moves
        y0, quiet = p.flag["detect"](good)
        y1, failed = p.flag["detect"](bad)
        print(f"    flag: failed {int(quiet)} without and {int(failed)} with the offending row at {n_rows + 1} of {B}")
        assert int(quiet) == 0 and int(failed) == 1 and bool(torch.isfinite(y0).all())
        assert bool(torch.isnan(y1[n_rows + 1, 1:]).all()) and bool(y1[n_rows + 1, 0] == bad[n_rows + 1, 0])
        keep = torch.arange(B, device=DEV) != n_rows + 1
        assert torch.equal(y1[keep], y0[keep])
        ym = DF.lpc2lsp(bad)   # the functional, as a caller has it: no error, no warning, the row NaN behind its gain (modules/lpc2lsp.py)
        assert torch.equal(ym[keep], y0[keep]) and bool(torch.isnan(ym[n_rows + 1, 1:]).all()) and bool(ym[n_rows + 1, 0] == bad[n_rows + 1, 0])
        return
    assert torch.equal(p.flag["run"](good), p.call(good))   # warn_type="exit" raises nothing
    with pytest.raises(RuntimeError, match=f"^{p.flag['text']}$"):
        p.flag["run"](bad)
    print(f"    flag: warn_type=\"exit\" is quiet without and raises with the offending row at {n_rows + 1} of {B}")
