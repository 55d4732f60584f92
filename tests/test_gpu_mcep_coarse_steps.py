"""The coarse Newton steps of the tuned mel-cepstral forward (csrc/mcep_mfma_f16.h): step k (1-based) runs
its two matrix chains on ONE binary16 product instead of three when k <= clamp(n_iter - 6, 0, 2); no frame stops on such a step.
ops.full_precision_chains() (DSA_ALGO_FULL_CHAINS, DSA_MCEP_FULL_CHAINS=1) keeps every step on three terms: the arithmetic before.

All at fft_length 512 / cep_order 24 / alpha 0.42, on the small inputs of tests/test_gpu_mcep_early_stop.py.  The schedule is read
from the public Newton history; the gate's edges (n_iter 6, 7, 8, 10) are held to the float64 oracle of the same n_iter at the suite's
tolerance; the default result is held elementwise to a quarter of that tolerance around the full-chains result (the bound the project
set for the stopping rule; measured 0.02 - 0.05 on these inputs, 0.10 on an all-zero utterance); the steps a frame takes must not
grow; and a frame's bits must not depend on path, batch or tile at the gate's edges either."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, ops
from test_gpu_mcep_early_stop import (DEV, INPUTS, MC32, _bits, _freeze_step, _input, _mixed_batch, _modules, _oracle,
                                      _oracle_spectrogram)

pytestmark = pytest.mark.gpu
GATE = [6, 7, 8, 10]   # n_coarse 0, 1, 2, 2


def _history(mods, x, fixed=False, full=False):
    """the raw one-launch call with the Newton history, (n_iter + 1, F, 25) iterates, under the two switches"""
    stft, mcep, _ = mods
    T = x.size(-1)
    B = x.numel() // T
    N = ops.num_frames(T, 80)
    mc = torch.empty(B, N, 25, device=DEV)
    hist = torch.full((mcep.n_iter + 1, B * N, 25), float("nan"), device=DEV)
    images = ops.mcep_images(mcep.G, mcep.D, mcep.E, 512, 24)
    scratch = torch.zeros(_lib.SCRATCH_BYTES, dtype=torch.uint8, device=DEV)
    algo = _lib.ALGO_AUTO | (_lib.ALGO_FIXED_STEPS if fixed else 0) | (_lib.ALGO_FULL_CHAINS if full else 0)
    ops._call("dsa_stft_mcep_fwd", x.data_ptr(), B, T, 400, 80, 512, stft.window.data_ptr(), stft.twiddle.data_ptr(), 1, float(stft.eps),
              24, mcep.n_iter, mcep.G.data_ptr(), mcep.D.data_ptr(), mcep.E.data_ptr(), mcep.alpha_vector.data_ptr(), _lib.F32,
              algo, images.data_ptr(), scratch.data_ptr(), mc.data_ptr(), hist.data_ptr(), None, ops._stream())
    assert _lib.last_kernel() == "stft512_mcep_fused_fwd"
    return mc, hist


def _frac(a, full, what):
    a, f = a.cpu().numpy().astype(np.float64), full.cpu().numpy().astype(np.float64)
    frac = np.abs(a - f) / (5e-6 + 1e-4 * np.abs(f))
    print(f"{what}: largest |default - full chains| {np.abs(a - f).max():.3g}, as a fraction of 5e-6 + 1e-4 |full|: {frac.max():.3g}")
    return float(frac.max())


@pytest.mark.parametrize("n_iter", [0, 1, 2, 3, 6, 7, 8, 10])
def test_the_schedule_is_what_it_says(n_iter):
    """Fixed steps, with and without the switch: no coarse step up to n_iter 6 (same bits), one at 7, two from 8 on.  The start value
    hist[0] is never touched; a coarse step's iterate differs from the full one's, and so does every iterate after it."""
    mods = _modules(n_iter)
    x = _input("randn").to(DEV)
    mc, hist = _history(mods, x, fixed=True)
    mcf, histf = _history(mods, x, fixed=True, full=True)
    assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(histf).all())
    assert torch.equal(_bits(hist[0]), _bits(histf[0]))
    if n_iter <= 6:
        assert torch.equal(_bits(hist), _bits(histf)) and torch.equal(_bits(mc), _bits(mcf))
        return
    # n_iter 7: one coarse step, and every iterate from hist[1] on differs; 8 and 10: the first two steps are coarse
    for s in range(1, n_iter + 1 if n_iter == 7 else 3):
        assert not torch.equal(_bits(hist[s]), _bits(histf[s])), s
    n_coarse = min(n_iter - 6, 2)
    print(f"n_iter {n_iter}: largest |coarse - full| of the iterate after step {n_coarse}: {float((hist[n_coarse] - histf[n_coarse]).abs().max()):.3g} "
          f"(largest entry {float(histf[n_coarse].abs().max()):.3g}); of the last iterate: {float((hist[-1] - histf[-1]).abs().max()):.3g}")


@pytest.mark.parametrize("n_iter", GATE)
@pytest.mark.parametrize("name", ["randn", "speech", "two_sines"])
def test_gate_edges_against_the_oracle(name, n_iter):
    """n_iter at and around the gate, fixed steps and early stop, against O.mcep of the same n_iter at the suite's tolerance: randn and
    speech through the one launch and the two kernels, two sines through the spectrogram entry (tests/test_gpu_mcep_early_stop.py
    explains why: the float32 STFT of that input cannot meet the oracle, whatever the mel-cepstral kernel does)."""
    stft, mcep, fused = _modules(n_iter)
    ref = _oracle(name, n_iter)
    outs = {}
    with torch.no_grad():
        if name == "two_sines":
            X = torch.from_numpy(_oracle_spectrogram(name).astype(np.float32)).to(DEV)
            outs["early, spectrogram in"] = mcep(X)
            assert _lib.last_kernel() == "mcep_mfma_fwd"
            with ops.fixed_newton_steps():
                outs["fixed, spectrogram in"] = mcep(X)
        else:
            x = _input(name).to(DEV)
            outs["early, one launch"] = fused(x)
            assert fused.last_path == "fused" and _lib.last_kernel() == "stft512_mcep_fused_fwd"
            outs["early, two kernels"] = mcep(stft(x))
            with ops.fixed_newton_steps():
                outs["fixed, one launch"] = fused(x)
                outs["fixed, two kernels"] = mcep(stft(x))
    for what, y in outs.items():
        y = y.cpu().numpy()
        print(f"{name}, n_iter {n_iter}, {what}: largest error as a fraction of the tolerance "
              f"{(np.abs(y - ref) / (5e-6 + 1e-4 * np.abs(ref))).max():.3g}")
    for what, y in outs.items():
        np.testing.assert_allclose(y.cpu().numpy(), ref, err_msg=what, **MC32)


@pytest.mark.parametrize("name", INPUTS)
def test_default_against_full_chains(name):
    """n_iter 10, default against full_precision_chains(), elementwise at 0.25 (5e-6 + 1e-4 |full|): early stop and fixed steps, the
    one launch (equal to the two kernels bit for bit) and the spectrogram entry."""
    x = _input(name).to(DEV)
    stft, mcep, fused = _modules()
    X = torch.from_numpy(_oracle_spectrogram(name).astype(np.float32)).to(DEV)
    with torch.no_grad():
        d1, d2, ds = fused(x), mcep(stft(x)), mcep(X)
        with ops.fixed_newton_steps():
            df = fused(x)
        with ops.full_precision_chains():
            f1, f2, fs = fused(x), mcep(stft(x)), mcep(X)
            with ops.fixed_newton_steps():
                ff = fused(x)
    assert torch.equal(_bits(d1), _bits(d2)) and torch.equal(_bits(f1), _bits(f2))
    fr = [_frac(d1, f1, name + ", waveform in"), _frac(ds, fs, name + ", float64 spectrogram in"), _frac(df, ff, name + ", waveform in, fixed steps")]
    assert max(fr) <= 0.25, fr


@pytest.mark.parametrize("name", INPUTS)
def test_steps_do_not_grow(name):
    """The first repeated step per frame of the early-stop history (the step a frame stopped at), default against full chains: at most
    1 % of an input's frames may stop later, and none stops before step 3 -- steps 1 and 2 are coarse and do not stop."""
    mods = _modules()
    x = _input(name).to(DEV)
    _, hist = _history(mods, x)
    _, histf = _history(mods, x, full=True)
    fs, fsf = _freeze_step(hist), _freeze_step(histf)
    later = int((fs > fsf).sum())
    print(f"{name}: frames per first repeated step, default {np.bincount(fs, minlength=11).tolist()}, full chains "
          f"{np.bincount(fsf, minlength=11).tolist()}; {later} of {fs.size} frames stop later, {int((fs < fsf).sum())} earlier")
    assert (fs >= 3).all(), np.bincount(fs, minlength=11)
    assert later <= 0.01 * fs.size, (later, fs.size)
    if name == "two_sines":   # the frames that ARE two sines still need (nearly) every step
        assert (fs[3:198] >= 9).all(), np.bincount(fs, minlength=11)


@pytest.mark.parametrize("n_iter", [7, 8, 10])
@pytest.mark.parametrize("T", [481, 1281])   # 7 and 17 frames per utterance: tiles straddle utterances
def test_bits_do_not_depend_on_company_at_the_gate(T, n_iter):
    x = _mixed_batch(T).to(DEV)
    stft, mcep, fused = mods = _modules(n_iter)
    with torch.no_grad():
        one = fused(x)
        assert fused.last_path == "fused"
        two = mcep(stft(x))
    assert bool(torch.isfinite(one).all())
    assert torch.equal(_bits(one), _bits(two))                                    # fused == two-kernel
    xg = x.clone().requires_grad_(True)
    assert torch.equal(_bits(fused(xg).detach()), _bits(one))                     # with a gradient (history and rt rows kept)
    Xg = stft(x).detach().requires_grad_(True)
    assert torch.equal(_bits(mcep(Xg).detach()), _bits(one))
    mch, hist = _history(mods, x)
    assert torch.equal(_bits(mch), _bits(one)) and torch.equal(_bits(hist[-1].view_as(one)), _bits(one))
    idx = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    with torch.no_grad():
        assert torch.equal(_bits(fused(x[idx])), _bits(one[idx]))
        for b in range(5):
            assert torch.equal(_bits(fused(x[b:b + 1])), _bits(one[b:b + 1]))


@pytest.mark.parametrize("name", ["all_zero", "near_silent"])
def test_no_frame_stops_on_a_coarse_step(name):
    """An all-zero utterance of 17 frames (a whole tile of padding-like frames, which stopped after step 1 - 2 before) and near-silent
    input: finite, within the 0.25 bound of the full-chains result, and no first repeat at step <= 2 in the early-stop history."""
    x = (torch.zeros(1, 1281) if name == "all_zero" else _input(name)).to(DEV)
    stft, mcep, fused = mods = _modules()
    with torch.no_grad():
        y = fused(x)
        with ops.full_precision_chains():
            yf = fused(x)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(yf).all())
    assert _frac(y, yf, name) <= 0.25
    mch, hist = _history(mods, x)
    assert torch.equal(_bits(mch), _bits(y))
    fs = _freeze_step(hist)
    _, histf = _history(mods, x, full=True)
    print(f"{name}: frames per first repeated step {np.bincount(fs, minlength=11).tolist()}, full chains "
          f"{np.bincount(_freeze_step(histf), minlength=11).tolist()}")
    assert (fs >= 3).all(), np.bincount(fs, minlength=11)


def test_a_nan_stays_in_its_frames_and_the_rest_keeps_its_bits():
    stft, mcep, fused = _modules()
    clean = _mixed_batch(481).to(DEV)
    dirty = _mixed_batch(481, nan_at=(1, 200)).to(DEV)
    with torch.no_grad():
        ref = fused(clean)
        one = fused(dirty)
        two = mcep(stft(dirty))
    bad = ~torch.isfinite(one).all(-1)
    assert 0 < int(bad.sum()) <= 6 and bool(bad[1].any()) and not bool(bad[[0, 2, 3, 4]].any())
    assert torch.equal(~torch.isfinite(two).all(-1), bad)
    assert torch.equal(_bits(one[~bad]), _bits(ref[~bad])) and torch.equal(_bits(two[~bad]), _bits(ref[~bad]))
    xg = dirty.clone().requires_grad_(True)
    yg = fused(xg).detach()
    assert torch.equal(~torch.isfinite(yg).all(-1), bad) and torch.equal(_bits(yg[~bad]), _bits(ref[~bad]))


def test_the_route_switch_parses(monkeypatch):
    """The environment form and the context manager give the same bits, through both entries; the mel-cepstral launch bits stay out of
    the LPC entry: fuse(frame, window, lpc) runs under ops.full_precision_chains()."""
    x = _input("randn").to(DEV)
    stft, mcep, fused = _modules()
    with torch.no_grad():
        default, default2 = fused(x), mcep(stft(x))
        with ops.full_precision_chains():
            full, full2 = fused(x), mcep(stft(x))
        monkeypatch.setenv("DSA_MCEP_FULL_CHAINS", "1")
        env, env2 = fused(x), mcep(stft(x))
        monkeypatch.setenv("DSA_MCEP_FULL_CHAINS", "0")
        off = fused(x)
        monkeypatch.delenv("DSA_MCEP_FULL_CHAINS")
        after = fused(x)
    assert torch.equal(_bits(env), _bits(full)) and torch.equal(_bits(env2), _bits(full2)) and torch.equal(_bits(full), _bits(full2))
    assert not torch.equal(_bits(default), _bits(full))
    assert torch.equal(_bits(off), _bits(default)) and torch.equal(_bits(after), _bits(default)) and torch.equal(_bits(default2), _bits(default))
    flpc = dsp.fuse(dsp.Frame(400, 80), dsp.Window(400, device=DEV), dsp.LPC(400, 24, eps=1e-5, device=DEV))
    with torch.no_grad():
        a = flpc(x)
        with ops.full_precision_chains():
            b = flpc(x)
    assert flpc.last_path.startswith("fused") and bool(torch.isfinite(b).all()) and torch.equal(_bits(a), _bits(b))
