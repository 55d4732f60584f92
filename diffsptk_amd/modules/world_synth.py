"""WORLD synthesis (reference: world_synth.py): F0, aperiodicity and spectral envelope to a waveform.  Three launches forward
(csrc/world_synth.hip): the time base and pulse list of every utterance, one response per pulse -- both minimum-phase spectra, the
fractional shift, the noise spectrum and the two inverse transforms without leaving LDS --, and the overlap-add as a gather; two
backward, to `sp` and `ap`.  No gradient flows to `f0` (the reference detaches it).

Departures from the reference (include/diffsptk_amd.h, section a24):
  * fft_length must be a power of two (the reference accepts any length >= 1024; WORLD itself only uses powers of two), and the per-pulse
    workgroup must fit DSA_WORLD_LDS_BYTES(L, size) <= DSA_WORLD_MAX_LDS_BYTES = 163840: fft_length <= 8192 in float32, <= 4096 in
    float64.  Anything else raises ValueError naming the constant -- at construction for the power of two and the module's dtype, in
    forward for the dtype of the data;
  * noise_size of the last pulse of EVERY utterance is 0.  The reference takes diff over the flattened batch, which for an utterance
    that is not the last gives max(0, first index of the next utterance - last index of this one): a value that depends on the
    neighbour in the batch.  Here an utterance's bits are those of the utterance run alone, given the same noise rows;
  * the noise comes from `self._randn(rows, cols)`: torch's generator on the module's device.  The same seed gives different noise from
    the reference's CPU generator;
  * a call in which no pulse falls anywhere returns zeros (the reference fails there inside its FFT with RuntimeError);
  * ap and sp must have fft_length / 2 + 1 bins (ValueError; the reference fails in a broadcast);
  * between the two launches of the pulse list the host reads the B pulse counts and allocates -- the operator's only read; the
    reference's `nonzero` has it too.  WorldSynthesis is therefore not capturable by Graphed.

The decisions -- where a pulse falls, whether it is voiced -- are discontinuous in the arithmetic, so the pulse list follows the
reference operation by operation in the data's dtype; float32 and float64 can choose different lists, as the reference's own do
(with an even frame_period the interpolated voicing flag is exactly 1/2 in the middle of every voiced / unvoiced transition).

One thing kept from the reference: torch.sqrt of its int64 noise_size is a float32 tensor whatever the data's dtype, so the float64
periodic response is scaled by a square root rounded to 24 bits, here too.

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py; there is no
functional form because the reference has none."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from ..utils.private import to
from .spec import device_twiddle

TAU = 6.283185307179586   # math.tau


class WorldSynthesis(nn.Module):
    """(f0:(B, N) or (N,), ap, sp:(B, N, L/2+1) or (N, L/2+1)) -> (B, N P) or (N P,) (world_synth.py:122-321).  frame_period >= 1,
    sample_rate >= 8000, fft_length >= 1024 and a power of two; default_f0: the F0 of unvoiced samples."""

    def __init__(
        self,
        frame_period: int,
        sample_rate: int,
        fft_length: int,
        *,
        default_f0: float = 500,
        device: torch.device | None = None,
        dtype: torch.dtype | None = None,
    ) -> None:
        super().__init__()

        if frame_period <= 0:
            raise ValueError("frame_period must be positive.")
        if sample_rate < 8000:
            raise ValueError("sample_rate must be at least 8000 Hz.")
        if fft_length < 1024:
            raise ValueError("fft_length must be at least 1024.")
        ops.check_world_length(fft_length, torch.empty(0, dtype=dtype).element_size())

        self.frame_period = frame_period
        self.sample_rate = sample_rate
        self.fft_length = fft_length
        self.default_f0 = default_f0

        self.register_buffer("ramp", torch.arange(fft_length, device=device), persistent=False)

        # the DC remover (world_synth.py:112-120): a Hann-like half window of L / 2 points, normalised so that both halves sum to 1, then
        # mirrored; in float64 with the reference's order of operations, so that the buffer has its bits
        half = fft_length // 2
        k = torch.arange(1, half + 1, device=device, dtype=torch.double)
        hann = 0.5 - 0.5 * torch.cos(TAU / (1 + fft_length) * k)
        hann = hann / (2 * torch.sum(hann))
        self.register_buffer("dc_remover", to(torch.cat([hann, hann.flip(-1)], dim=-1), dtype=dtype), persistent=False)

    def _randn(self, rows: int, cols: int) -> torch.Tensor:
        """Every random draw of `forward`: (rows, cols) standard normal numbers of the buffers' dtype from torch's generator of the
        module's device (torch.manual_seed seeds it)."""
        return torch.randn(rows, cols, device=self.dc_remover.device, dtype=self.dc_remover.dtype)

    def forward(self, f0: torch.Tensor, ap: torch.Tensor, sp: torch.Tensor, out_length: int | None = None) -> torch.Tensor:
        batched = f0.ndim == 2
        if not batched:
            f0, ap, sp = f0.unsqueeze(0), ap.unsqueeze(0), sp.unsqueeze(0)

        # the reference's checks, in its order and with its texts (world_synth.py:172-182)
        if f0.dim() != 2:
            raise ValueError("f0 must be 1D or 2D tensor.")
        if ap.dim() != 3 or sp.dim() != 3:
            raise ValueError("ap and sp must be 2D or 3D tensor.")
        if not f0.shape[0] == ap.shape[0] == sp.shape[0]:
            raise ValueError("f0, ap, and sp must have the same batch size.")
        if not f0.shape[1] == ap.shape[1] == sp.shape[1]:
            raise ValueError("f0, ap, and sp must have the same length.")
        if ap.shape[2] != sp.shape[2]:
            raise ValueError("ap and sp must have the same dimension.")
        L = self.fft_length
        if sp.shape[2] != L // 2 + 1:
            raise ValueError(f"ap and sp must have fft_length / 2 + 1 = {L // 2 + 1} bins.")
        ops.check_world_length(L, sp.element_size())
        ops._same_dtype(sp, f0, ap, self.dc_remover)
        ops._dtype_code(sp)
        ops._require_device(f0, ap, sp, self.dc_remover)

        B, N, _ = sp.shape
        T = N * self.frame_period
        Tout = T if out_length is None else max(0, min(int(out_length), T))
        offsets, irec, frec, pulses = ops.world_pulses(f0, self.frame_period, self.sample_rate, L, self.default_f0)
        noise = self._randn(pulses, L) if pulses else torch.empty(0, L, device=sp.device, dtype=sp.dtype)
        y = ops.WorldResponsesFn.apply(ap, sp, noise.to(sp.dtype), offsets, irec, frec, self.dc_remover, device_twiddle(L, sp.device, sp.dtype),
                                       self.sample_rate, L, Tout)
        return y if batched else y.squeeze(0)
