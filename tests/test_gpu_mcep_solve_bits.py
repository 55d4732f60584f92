"""The forward Newton solve of the tuned mel-cepstral kernels (blk_elim_all_r24 in csrc/mcep_solve.h) on shapes and inputs the
other tests leave out.  The fused launch (stft512_mcep_fused_fwd) and the two-kernel path (stft512_fwd + mcep_mfma_fwd) run the same
solve code, so their mel-cepstra must agree bit for bit: on a ragged last tile of 16 frames, on a single frame and around frames
made non-finite by their samples.  On badly conditioned inputs -- near-silent utterances, a quiet stretch inside an utterance -- the
fused result is held to the float64 oracle at the tolerance of tests/test_gpu_fused_mcep.py."""
import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
MC32 = dict(rtol=1e-4, atol=5e-6)


def _modules():
    stft = dsp.STFT(400, 80, 512, device=DEV)
    mcep = dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=10, device=DEV)
    return stft, mcep, dsp.fuse(stft, mcep)


def _both(x):
    stft, mcep, fused = _modules()
    with torch.no_grad():
        two = mcep(stft(x))
        one = fused(x)
    assert fused.last_path == "fused" and _lib.last_kernel() == "stft512_mcep_fused_fwd"
    return one, two


def _bits(t):
    return t.contiguous().view(torch.int32)


# frames per utterance: 17 and 33 leave a last tile of 1 frame, 31 a tile of 15, 1 a lone frame; 5 x 7 = 35 frames in all
@pytest.mark.parametrize("B,T", [(1, 1281), (1, 2561), (1, 2401), (1, 1), (1, 80), (5, 481), (3, 16000)])
def test_fused_and_two_kernel_solves_agree_bit_for_bit(B, T):
    x = torch.randn(B, T, generator=torch.Generator().manual_seed(B * 31 + T)).to(DEV)
    one, two = _both(x)
    assert one.shape == two.shape and bool(torch.isfinite(one).all())
    assert torch.equal(_bits(one), _bits(two))


def test_non_finite_frames_stay_in_their_frames_and_the_rest_agree_bit_for_bit():
    x = torch.randn(3, 4000, generator=torch.Generator().manual_seed(5))
    x[0, 1000] = float("nan")
    x[1, 3999] = float("inf")
    x[2, 40] = float("-inf")
    x[2, 2500] = float("nan")
    one, two = _both(x.to(DEV))
    bad = ~torch.isfinite(two).all(-1)
    assert torch.equal(~torch.isfinite(one).all(-1), bad)
    assert 0 < int(bad.sum()) < 24
    assert torch.equal(_bits(one[~bad]), _bits(two[~bad]))


@pytest.mark.parametrize("case", ["near_silent", "quiet_stretch", "silent_gap"])
def test_badly_conditioned_inputs_against_the_oracle(case):
    x = torch.randn(2, 8000, generator=torch.Generator().manual_seed(17))
    if case == "near_silent":
        x *= 1e-3
    elif case == "quiet_stretch":
        x[:, 3000:5000] *= 1e-3
    else:
        x[0, 2000:2800] *= 1e-4
        x[1, 6000:] *= 1e-3
    one, two = _both(x.to(DEV))
    assert torch.equal(_bits(one), _bits(two))
    X_ref = O.stft(x.double().numpy(), 400, 80, 512)
    np.testing.assert_allclose(one.cpu().numpy(), O.mcep(X_ref, 24, 0.42, 10), **MC32)
