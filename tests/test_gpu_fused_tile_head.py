"""The tile head of the fused STFT -> mel-cepstrum launch (csrc/mcep_mfma_f16.h).  A lane's frame is
addressed once per tile: pass 0 of the four STFT passes derives (utterance, frame in it) with a division, passes 1 - 3 step that
pair by four frames with the wrap at N frames per utterance; tiles that are clamped against the frame count, and utterances of
fewer than four frames, derive every pass as before.  What stepping can break is WHICH samples a frame reads, so everything here
is compared bit for bit: the one launch with mcep(stft(x)) -- whose frames never share a tile head -- and every utterance run
alone with its rows in the batch.

Shapes (frame length 400, period 80, so N = (T - 1) // 80 + 1 frames per utterance): N = 1, 1, 4, 5, 7, 17 with utterance
boundaries inside a pass and, from N = 4 on, inside stepped tiles; 200 frames per utterance for whole stepped tiles; every total
is off a multiple of 16, so the last tile is clamped and takes the deriving path next to stepped ones; T < 416 puts every frame on
the padded fetch."""
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 80


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch(B, T, seed=0):
    """noise at a different level per utterance, with a slow ramp: no two frames of the batch are alike"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + T)
    x = torch.randn(B, T, generator=g) * torch.logspace(-2, 0, B).unsqueeze(1)
    return (x * torch.linspace(0.5, 1.5, T)).to(DEV)


def _modules(**stft_options):
    stft = dsp.STFT(400, P, 512, device=DEV, **stft_options)
    mcep = dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=10, device=DEV)
    return stft, mcep, dsp.fuse(stft, mcep)


def _one_launch(fused, x):
    y = fused(x)
    assert fused.last_path == "fused" and _lib.last_kernel() == "stft512_mcep_fused_fwd"
    return y


def _check(x, stft, mcep, fused):
    """the one launch against the two kernels, and every utterance alone against its rows in the batch"""
    B, T = x.shape
    with torch.no_grad():
        one = _one_launch(fused, x)
        two = mcep(stft(x))
        assert _lib.last_kernel() == "mcep_mfma_fwd"
        assert one.shape == (B, (T - 1) // P + 1, 25) and bool(torch.isfinite(one).all())
        assert torch.equal(_bits(one), _bits(two))
        for b in range(B):
            assert torch.equal(_bits(_one_launch(fused, x[b:b + 1])), _bits(one[b:b + 1])), b
    return one


@pytest.mark.parametrize("B,T", [(5, 1), (5, 80), (5, 481), (5, 1281), (3, 16000), (9, 320), (7, 400)])
def test_constant_padding(B, T):
    """(5, 1), (5, 80): one frame per utterance, four utterances per pass; (5, 481), (5, 1281): 7 and 17 frames, 35 and 85 in all;
    (3, 16000): 600 frames, 37 stepped tiles and a clamped one; (9, 320): N = 4, a step wraps onto the frame it left in the next
    utterance; (7, 400): N = 5, stepped tiles whose every frame reaches over an end of its utterance."""
    assert ((T - 1) // P + 1) * B % 16 != 0
    _check(_batch(B, T), *_modules())


@pytest.mark.parametrize("mode,B", [("reflect", 2), ("replicate", 2), ("circular", 2), ("reflect", 5)])
def test_options_instantiation(mode, B):
    """reflect / replicate / circular padding: the options instantiation.  B = 2: 14 frames, one clamped tile; B = 5: 35 frames,
    the stepped path in that instantiation as well."""
    _check(_batch(B, 481, seed=1), *_modules(mode=mode))


def test_with_a_gradient():
    """a gradient is wanted: the instantiation that keeps every step's iterate and rt row.  Same forward bits; the backward runs."""
    stft, mcep, fused = _modules()
    x = _batch(5, 481, seed=2)
    one = _check(x, stft, mcep, fused)
    xg = x.clone().requires_grad_(True)
    y = _one_launch(fused, xg)
    assert torch.equal(_bits(y.detach()), _bits(one))
    y.square().mean().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    Xg = stft(x).detach().requires_grad_(True)
    assert torch.equal(_bits(mcep(Xg).detach()), _bits(one))


def test_overlapped_launches():
    """ops.overlapped_launches() changes which wave takes a tile, never the tile: the same bits, below one round of tiles and above
    (600 and 34 000 frames: 2 125 tiles on 2 048 wave slots, a short last round)."""
    stft, mcep, fused = _modules()
    for B, T in ((3, 16000), (170, 16000)):
        x = _batch(B, T, seed=3)
        with torch.no_grad():
            ref = _one_launch(fused, x)
            two = mcep(stft(x))
            with ops.overlapped_launches():
                got = _one_launch(fused, x)
        assert torch.equal(_bits(ref), _bits(two)) and torch.equal(_bits(got), _bits(ref)), (B, T)
