"""WORLD synthesis (csrc/world_synth.hip): the pulse list of every utterance, a response per pulse, the overlap-add as a gather, and the
adjoint down to the spectral envelope and the aperiodicity."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ._core import _call, _dtype_code, _p, _require_device, _same_dtype, _stream


def world_lds_bytes(L: int, size: int) -> int:
    """DSA_WORLD_LDS_BYTES(L, size) of include/diffsptk_amd.h, section a24: one complex transform of L points, the two half spectra it
    carries (4 (L / 2 + 1) values) and 256 bytes of reduction exchange -- what the per-pulse workgroup holds in LDS"""
    return (4 * L + 4) * size + 256


def check_world_length(L: int, size: int) -> None:
    """The two limits of the kernels, by the name of their constant; needs no device."""
    if L < 2 or L & (L - 1):
        raise ValueError(f"world_synth: fft_length must be a power of two, got {L}: the transforms run in LDS on "
                         f"DSA_WORLD_LDS_BYTES(L, size) <= DSA_WORLD_MAX_LDS_BYTES = {_lib.WORLD_MAX_LDS_BYTES} bytes, radix 2")
    need = world_lds_bytes(L, size)
    if need > _lib.WORLD_MAX_LDS_BYTES:
        raise ValueError(f"world_synth: fft_length {L} takes DSA_WORLD_LDS_BYTES = {need} bytes per pulse: the transform and the two half "
                         f"spectra must fit DSA_WORLD_MAX_LDS_BYTES = {_lib.WORLD_MAX_LDS_BYTES} bytes of LDS")


def world_pulses(f0: torch.Tensor, P: int, sample_rate: int, L: int, default_f0: float):
    """f0:(B, N) -> (offsets:(B + 1) int64 on the device, irec:(pulses, 4) int64, frec:(pulses, 3), pulses).  Two launches of
    dsa_world_synth_pulses with the operator's one host read between them: the B counts."""
    check_world_length(L, f0.element_size())
    code = _dtype_code(f0)
    _require_device(f0)
    fc = f0.detach().contiguous()
    B, N = fc.shape
    counts = torch.zeros(B, dtype=torch.int64, device=fc.device)
    offsets = torch.zeros(B + 1, dtype=torch.int64, device=fc.device)
    if B == 0 or N == 0:
        return offsets, torch.empty(0, 4, dtype=torch.int64, device=fc.device), torch.empty(0, 3, dtype=fc.dtype, device=fc.device), 0
    with torch.cuda.device(fc.device):
        _call("dsa_world_synth_pulses", _p(fc), B, N, P, sample_rate, L, float(default_f0), None, code, _p(counts), None, None, _stream())
        host = counts.cpu()   # the one read
        pulses = int(host.sum())
        offsets[1:] = torch.cumsum(host, 0).to(fc.device)
        irec = torch.empty(pulses, 4, dtype=torch.int64, device=fc.device)
        frec = torch.empty(pulses, 3, dtype=fc.dtype, device=fc.device)
        if pulses:
            _call("dsa_world_synth_pulses", _p(fc), B, N, P, sample_rate, L, float(default_f0), _p(offsets), code, _p(counts), _p(irec), _p(frec),
                  _stream())
    return offsets, irec, frec, pulses


class WorldResponsesFn(torch.autograd.Function):
    """(ap, sp):(B, N, D) -> y:(B, T) for the pulse records of world_pulses, noise:(pulses, L), the module's dc_remover and the twiddle table of
    L points.  Saved for the backward: the inputs, the noise and the records; the (pulses, L) responses are not."""

    @staticmethod
    def forward(ctx, ap, sp, noise, offsets, irec, frec, remover, twiddle, sample_rate, L, T):
        _same_dtype(sp, ap, noise, frec, remover, twiddle)
        code = _dtype_code(sp)
        _require_device(ap, sp, noise, offsets, irec, frec, remover, twiddle)
        apc, spc, nc = ap.contiguous(), sp.contiguous(), noise.contiguous()
        B, N, _ = spc.shape
        pulses = irec.size(0)
        y = torch.empty(B, T, device=spc.device, dtype=spc.dtype)
        if B and T:
            with torch.cuda.device(spc.device):
                response = torch.empty(pulses, L, device=spc.device, dtype=spc.dtype)
                if pulses:
                    _call("dsa_world_synth_responses", _p(apc), _p(spc), _p(nc), _p(irec), _p(frec), _p(offsets), _p(remover), _p(twiddle), B, N,
                          sample_rate, L, pulses, code, _p(response), _stream())
                _call("dsa_world_synth_overlap_add", _p(response), _p(irec), _p(offsets), B, T, L, pulses, code, _p(y), _stream())
        ctx.cfg = (sample_rate, L, T)
        ctx.save_for_backward(apc, spc, nc, offsets, irec, frec, remover, twiddle)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        apc, spc, nc, offsets, irec, frec, remover, twiddle = ctx.saved_tensors
        sample_rate, L, T = ctx.cfg
        B, N, D = spc.shape
        pulses = irec.size(0)
        code = _dtype_code(spc)
        gc = gy.contiguous()
        gap, gsp = torch.empty_like(apc), torch.empty_like(spc)
        if B and N:
            with torch.cuda.device(spc.device):
                grows = torch.empty(pulses, 2, D, device=spc.device, dtype=spc.dtype)
                if pulses:
                    _call("dsa_world_synth_vjp_pulses", _p(gc), _p(apc), _p(spc), _p(nc), _p(irec), _p(frec), _p(offsets), _p(remover), _p(twiddle),
                          B, N, T, sample_rate, L, pulses, code, _p(grows), _stream())
                _call("dsa_world_synth_vjp_frames", _p(grows), _p(apc), _p(spc), _p(irec), _p(frec), _p(offsets), B, N, L, pulses, code, _p(gap),
                      _p(gsp), _stream())
        return gap, gsp, None, None, None, None, None, None, None, None, None
