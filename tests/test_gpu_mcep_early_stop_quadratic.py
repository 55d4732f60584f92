"""The second clause of the tuned mel-cepstral forward's stopping rule (csrc/mcep_mfma_f16.h).  With
u_k = |x_k|_inf / max(1, |mc_(k-1)|_inf) of step k's update x_k, tau = 2^-20 and the factor 16, a frame stops after step k if

    u_k <= tau,   or   u_k <= 16 tau  and  u_k <= u_(k-1) / 16       (the second is false at step 1)

All at fft_length 512 / cep_order 24 / alpha 0.42 / n_iter 10 on the small inputs of tests/test_gpu_mcep_early_stop.py.

The rule is recomputed in float64 from the fixed-step Newton history (every step run, every update applied).  The history holds the
iterates, not the updates: its difference d = fl(mc + x) - mc is the kernel's x up to the float32 rounding of that one addition, at
most half an ulp of the sum per coefficient.  At the first threshold that is 2^-24 |mc| against x = 2^-20 |mc|, a sixteenth -- more
than a fixed relative margin of 2^-6 covers.  So every comparison is made twice, once widened and once narrowed by the factor
1 +- 2^-6 AND with |x|_inf taken at the two ends of the interval max_i (d_i -+ half an ulp of the sum); a frame whose two predicted
stopping steps agree must stop at exactly that step in the early-stop history, and at most 10 % of an input's frames may disagree."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, ops

from test_gpu_mcep_early_stop import _bits, _freeze_step, _history, _input, _mixed_batch, _modules

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAU = 2.0 ** -20
FACTOR = 16.0
EPS = 2.0 ** -6
RULE_INPUTS = ["randn", "speech", "near_silent", "two_sines"]
_hist_cache = {}


def _histories(name):
    """(early-stop history, fixed-step history) of an input, each (11, F, 25): computed once, shared, never written to"""
    if name not in _hist_cache:
        mods = _modules()
        x = _input(name).to(DEV)
        _, early = _history(mods, x)
        _, fixed = _history(mods, x, fixed=True)
        _hist_cache[name] = (early, fixed)
    return _hist_cache[name]


def _predict(fixed):
    """From a fixed-step history: per frame the stopping step (1-based; n_iter where the rule never holds) under the widened and under
    the narrowed comparisons, and per frame and step the truth of each clause under both."""
    h = fixed.double().cpu().numpy()                                  # (n_iter + 1, F, 25)
    n_iter = h.shape[0] - 1
    d = np.abs(h[1:] - h[:-1])                                        # exact in float64
    half_ulp = 0.5 * np.spacing(np.abs(fixed[1:].cpu().numpy())).astype(np.float64)
    x_lo = np.maximum(d - half_ulp, 0.0).max(-1)                      # (n_iter, F): |x|_inf lies in [x_lo, x_hi]
    x_hi = (d + half_ulp).max(-1)
    m = np.maximum(1.0, np.abs(h[:-1]).max(-1))
    u_lo, u_hi = x_lo / m, x_hi / m
    up_lo = np.concatenate([np.zeros_like(u_lo[:1]), u_lo[:-1]])       # u of the step before; none before step 1: 0
    up_hi = np.concatenate([np.zeros_like(u_hi[:1]), u_hi[:-1]])
    wide = dict(c1=u_lo <= TAU * (1 + EPS), c2=(u_lo <= FACTOR * TAU * (1 + EPS)) & (u_lo <= up_hi / FACTOR * (1 + EPS)))
    narrow = dict(c1=u_hi <= TAU * (1 - EPS), c2=(u_hi <= FACTOR * TAU * (1 - EPS)) & (u_hi <= up_lo / FACTOR * (1 - EPS)))
    wide["c2"][0] = narrow["c2"][0] = False                            # no u_0
    steps = np.arange(1, n_iter + 1)[:, None]
    stop_w = np.where(wide["c1"] | wide["c2"], steps, n_iter).min(0)
    stop_n = np.where(narrow["c1"] | narrow["c2"], steps, n_iter).min(0)
    assert (stop_w <= stop_n).all()
    return stop_w, stop_n, wide, narrow, dict(u_lo=u_lo, u_hi=u_hi, up_lo=up_lo, up_hi=up_hi)


@pytest.mark.parametrize("name", RULE_INPUTS)
def test_the_rule_is_the_rule(name):
    early, fixed = _histories(name)
    fs = _freeze_step(early)
    stop_w, stop_n, wide, narrow, _ = _predict(fixed)
    sure = stop_w == stop_n
    F = fs.size
    print(f"{name}: {F} frames, ambiguous {int((~sure).sum())}; frames per first repeated step {np.bincount(fs, minlength=11).tolist()}; "
          f"predicted {np.bincount(stop_n[sure], minlength=11).tolist()}")
    assert (~sure).sum() <= 0.10 * F, int((~sure).sum())
    wrong = np.nonzero(sure & (fs != stop_n))[0]
    assert wrong.size == 0, (wrong[:10], fs[wrong[:10]], stop_n[wrong[:10]])
    # through which clause: at its stopping step k the frame certainly satisfies the second clause and certainly not the first
    # (today's rule alone would have gone on), and the first clause certainly holds at step k + 1 of the fixed-step run
    k = np.clip(stop_n - 1, 0, 9)
    cols = np.arange(F)
    stopped = sure & (stop_n < 10) | (sure & (narrow["c1"][9] | narrow["c2"][9]))
    by_second = stopped & narrow["c2"][k, cols] & ~wide["c1"][k, cols]
    by_first = stopped & narrow["c1"][k, cols]
    one_early = by_second & (k < 9) & narrow["c1"][np.minimum(k + 1, 9), cols]
    print(f"{name}: stopped through the first clause {int(by_first.sum())}, through the second alone {int(by_second.sum())}, "
          f"of those one step before the first clause would have {int(one_early.sum())} ({one_early.sum() / F:.1%} of the frames)")
    if name in ("randn", "speech"):
        assert one_early.sum() >= 0.15 * F, (int(one_early.sum()), F)


def test_slow_convergers_are_untouched():
    """The frames that ARE two sines (3 .. 197) converge linearly: a small update there is not a small error."""
    early, fixed = _histories("two_sines")
    fs = _freeze_step(early)
    print("two sines: frames per first repeated step", np.bincount(fs, minlength=11).tolist())
    for s in range(11):   # up to and including the step at which a frame stops, the two runs are the same computation
        sel = torch.from_numpy((fs >= s) & (np.arange(fs.size) >= 3) & (np.arange(fs.size) < 198)).to(DEV)
        assert torch.equal(_bits(early[s][sel]), _bits(fixed[s][sel])), s
    _, _, wide, _, v = _predict(fixed)
    for f in range(3, 198):
        if fs[f] < 10:      # stopped after step k = fs[f] (index k - 1): not while certainly contracting slower than 16 and certainly above tau
            k = fs[f] - 1
            slow = v["u_lo"][k, f] > v["up_hi"][k, f] / FACTOR * (1 + EPS)
            assert not (slow and not wide["c1"][k, f]), (f, fs[f], v["u_lo"][k, f], v["up_hi"][k, f])


def _options_modules(T):
    """the options instantiation of the one launch: any padding but zeros.  Reflection needs more samples than it pads (200), so the
    one-sample utterances repeat their sample instead"""
    stft = dsp.STFT(400, 80, 512, mode="reflect" if T > 200 else "replicate", device=DEV)
    mcep = dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=10, device=DEV)
    return stft, mcep, dsp.fuse(stft, mcep)


@pytest.mark.parametrize("mode", ["constant", "reflect"])
@pytest.mark.parametrize("T", [1, 481, 1281])   # 1, 7 and 17 frames per utterance: tiles straddle utterances
def test_geometry_edges_in_every_path(T, mode):
    """One launch (plain and options instantiation), two kernels, with and without a history: the same bits, whatever the batch and the
    tile a frame sits in."""
    x = _mixed_batch(T).to(DEV)
    stft, mcep, fused = _modules() if mode == "constant" else _options_modules(T)
    with torch.no_grad():
        one = fused(x)
        assert fused.last_path == "fused" and _lib.last_kernel() == "stft512_mcep_fused_fwd"
        two = mcep(stft(x))
        assert _lib.last_kernel() == "mcep_mfma_fwd"
    assert bool(torch.isfinite(one).all())
    assert torch.equal(_bits(one), _bits(two))                                    # path
    xg = x.clone().requires_grad_(True)
    assert torch.equal(_bits(fused(xg).detach()), _bits(one))                     # history kept (every step run, updates masked)
    assert fused.last_path == "fused"
    Xg = stft(x).detach().requires_grad_(True)
    assert torch.equal(_bits(mcep(Xg).detach()), _bits(one))
    if mode == "constant":
        mch, hist = _history((stft, mcep, fused), x)
        assert torch.equal(_bits(mch), _bits(one)) and torch.equal(_bits(hist[-1].view_as(one)), _bits(one))
    with torch.no_grad():
        idx = torch.tensor([3, 0, 4, 2, 1], device=DEV)
        assert torch.equal(_bits(fused(x[idx])), _bits(one[idx]))                 # batch
        for b in range(5):
            assert torch.equal(_bits(fused(x[b:b + 1])), _bits(one[b:b + 1]))
        assert torch.equal(_bits(fused(x[1:])), _bits(one[1:]))                   # tile: every frame in another slot of another tile
        assert torch.equal(_bits(mcep(stft(x[1:]))), _bits(one[1:]))


@pytest.mark.parametrize("n_iter", [0, 1, 2])
def test_nothing_stops_within_two_steps(n_iter):
    """randn: after two steps no frame's update is near 2^-16, let alone 2^-20 -- nothing can have stopped, early and fixed steps are
    the same bits in every path."""
    x = _input("randn").to(DEV)
    stft, mcep, fused = _modules(n_iter)
    with torch.no_grad():
        early = fused(x)
        early2 = mcep(stft(x))
        with ops.fixed_newton_steps():
            fixed = fused(x)
    xg = x.clone().requires_grad_(True)
    assert torch.equal(_bits(early), _bits(fixed)) and torch.equal(_bits(early2), _bits(fixed))
    assert torch.equal(_bits(fused(xg).detach()), _bits(fixed))


@pytest.mark.parametrize("name", RULE_INPUTS)
def test_step_one_never_stops_through_the_second_clause(name):
    """There is no u_0: whatever stops at step 1 has an update of at most 2^-20 itself."""
    early, fixed = _histories(name)
    fs = _freeze_step(early)
    _, _, wide, _, _ = _predict(fixed)
    print(f"{name}: {int((fs <= 1).sum())} frames stop at step 1")
    assert wide["c1"][0][fs <= 1].all()
