"""Aperiodicity (reference: ap.py): a waveform and its F0 to the band aperiodicity of TANDEM-STRAIGHT, interpolated onto the bins of an
FFT when fft_length is given.  Forward (csrc/ap.hip): one launch per level of the QMF pyramid, then ONE launch for every (band, frame)
least-squares fit with the interpolation, the clip and the output format; backward: the fits' adjoint, an overlap-add written as a gather,
and the pyramid's transpose.  The gradient flows to `x`; none to `f0` (the reference detaches it).

Departures from the reference (include/diffsptk_amd.h, section a25):
  * algorithm="d4c" raises ValueError saying that only "tandem" is built (D4C rests on the third_party/world helpers, which this
    package does not have); an unknown name keeps the reference's "is not supported" text;
  * the regulariser escalates PER FIT.  The reference tries eps m, m = 1, 10, ..., on the whole batch until no Cholesky factorisation
    in it fails, with a host read per trial, so a frame's result depends on its neighbours in the batch.  Here every (band, frame) fit takes
    the first m at which its own pivots are positive and finite, inside the kernel, and a fit that no m <= 10^8 factors returns
    upper_bound for that band with a zero gradient where the reference raises RuntimeError.  The sums, the factorisation and the two
    standard deviations run in float64 for both dtypes, and so do the band signals of the pyramid, with the library's float64 taps (the hHP
    and hLP buffers hold the same values in the module's dtype, as the reference's do): on a clean periodic signal the aperiodicity is
    the bands' rounding noise.  A float32 fit therefore escalates only where a float64 one would, and a float32 call returns the float64
    result rounded; wherever the reference's first trial succeeds everywhere the two agree;
  * a waveform too short for the pyramid raises ValueError naming the smallest admissible length, 20 * 2^(n_band - 2) + 1 (every
    level's input needs 21 samples; the reference fails inside ReflectionPad1d);
  * x and f0 must agree on the batch size (ValueError);
  * a band whose aperiodicity is exactly 0 (a silent segment) makes the bins it reaches 0 before the clip, so lower_bound after it,
    with a zero gradient; a zero-variance denominator gives a zero gradient (the reference returns NaN from log 0 when it interpolates);
  * the segments must fit the per-frame workgroup: DSA_AP_LDS_BYTES(sum(J), n_band) <= DSA_AP_MAX_LDS_BYTES = 163840 (with
    window_length_ms = 30: any sample_rate up to 135699 Hz), else ValueError naming the constant, at construction;
  * there is no host read anywhere, so the module is capturable by Graphed.

The integers t0, index_bias and curr_pos decide which samples a fit reads; they are formed in the data's dtype with the reference's
operations in its order, so float32 and float64 can differ where the reference's own do (an odd frame_period makes curr_pos of the deep
bands an exact integer before truncation).

The class is exported from the package root, not from diffsptk_amd.modules, for the reason given in modules/mlsacheck.py; there is no
functional form because the reference has none."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import ops
from ..utils.private import to

# The QMF pair of TANDEM-STRAIGHT's band splitting (Kawahara et al. 2010; the values WORLD's first aperiodicity estimator ships): both
# filters are symmetric, so the first half and the centre tap are listed: 41 taps high-pass, 37 taps low-pass.
_QMF_HIGH = (+0.00041447996898231424, +0.00078125051417292477, -0.0010917236836275842, -0.0019867925675967589, +0.0020903896961562292,
             +0.0040940570272849346, -0.0034025808529816698, -0.0074961541272056016, +0.0049722633399330637, +0.012738791249119802,
             -0.0066960326895749113, -0.020694051570247052, +0.0084324365650413451, +0.033074383758700532, -0.010018936738799522,
             -0.054231361405808247, +0.011293988915051487, +0.10020081367388213, -0.012120546202484579, -0.31630021039095702,
             +0.51240682580627639)
_QMF_LOW = (-0.00065488170077483048, +0.00007561994958159384, +0.0020408456937895227, -0.00074680535322030437, -0.0043502235688264931,
            +0.0025966428382642732, +0.0076396022827566962, -0.0064904118901497852, -0.011765804538954506, +0.013649908479276255,
            +0.01636866479016021, -0.026075976030529347, -0.020910294856659444, +0.048260725032316647, +0.024767846611048111,
            -0.096178467583360641, -0.027359756709866623, +0.31488052161630042, +0.52827343594055032)


def _symmetric(half) -> np.ndarray:
    h = np.asarray(half, dtype=np.float64)
    return np.concatenate([h, h[-2::-1]])


class AperiodicityExtractionByTANDEM(nn.Module):
    """The buffers of the reference's extractor (ap.py:212-292), under the same names and shapes, all non-persistent."""

    def __init__(self, frame_period, sample_rate, fft_length=None, *, window_length_ms=30, eps=1e-5, device=None, dtype=None):
        super().__init__()

        if window_length_ms <= 0:
            raise ValueError("window_length_ms must be positive.")
        if eps <= 0:
            raise ValueError("eps must be positive.")
        ops.check_ap_segments(sample_rate, window_length_ms)

        self.frame_period = frame_period
        self.sample_rate = sample_rate
        self.window_length_ms = window_length_ms
        self.eps = eps
        self.n_band, self.cutoff_list, self.segment_length = ops.ap_bands(sample_rate, window_length_ms)
        self.default_f0 = 150
        self.n_trial = 10

        if fft_length is not None:
            segment, weight = ops.ap_interp_tables(sample_rate, fft_length, self.n_band)
            self.register_buffer("interp_indices", to(segment.reshape(1, 1, -1), device=device, dtype=torch.long), persistent=False)
            self.register_buffer("interp_weights", to(weight.reshape(1, 1, -1), device=device, dtype=dtype), persistent=False)

        self.register_buffer("ramp", torch.arange(-1, self.segment_length[0] + 1, device=device).view(1, 1, -1), persistent=False)
        self.register_buffer("eye", torch.eye(6, device=device, dtype=dtype) * eps, persistent=False)
        self.register_buffer("hHP", to(_symmetric(_QMF_HIGH), device=device, dtype=dtype).view(1, 1, -1), persistent=False)
        self.register_buffer("hLP", to(_symmetric(_QMF_LOW), device=device, dtype=dtype).view(1, 1, -1), persistent=False)

        self.register_buffer("window", to(ops.ap_windows(self.segment_length), device=device, dtype=dtype), persistent=False)
        self.register_buffer("window_sqrt", self.window.sqrt(), persistent=False)


class Aperiodicity(nn.Module):
    """(x:(B, T) or (T,), f0:(B, N) or (N,) in Hz) -> (B, N, L/2+1) or (N, L/2+1); (.., n_band + 1) band values when fft_length is None
    (ap.py:77-171).  frame_period >= 1, sample_rate >= 8000, fft_length >= 16 or None, algorithm "tandem", out_format "a", "p", "a/p" or
    "p/a" (or 0 .. 3), 0 <= lower_bound < upper_bound <= 1; keywords window_length_ms, eps, device, dtype."""

    def __init__(
        self,
        frame_period: int,
        sample_rate: int,
        fft_length: int | None = None,
        algorithm: str = "tandem",
        out_format: str | int = "a",
        lower_bound: float = 0.001,
        upper_bound: float = 0.999,
        **kwargs,
    ) -> None:
        super().__init__()

        if frame_period <= 0:
            raise ValueError("frame_period must be positive.")
        if sample_rate < 8000:
            raise ValueError("sample_rate must be at least 8000 Hz.")
        if fft_length is not None and fft_length < 16:
            raise ValueError("fft_length must be at least 16.")
        if not 0 <= lower_bound < upper_bound <= 1:
            raise ValueError("Invalid lower_bound and upper_bound.")

        self.lower_bound = lower_bound
        self.upper_bound = upper_bound

        if algorithm == "tandem":
            self.extractor = AperiodicityExtractionByTANDEM(frame_period, sample_rate, fft_length, **kwargs)
        elif algorithm == "d4c":
            raise ValueError("algorithm d4c is not built: diffsptk_amd has only the tandem algorithm.")
        else:
            raise ValueError(f"algorithm {algorithm} is not supported.")

        if out_format not in ops.AP_FORMATS or isinstance(out_format, bool):
            raise ValueError(f"out_format {out_format} is not supported.")
        self.out_format = ops.AP_FORMATS[out_format]

    def forward(self, x: torch.Tensor, f0: torch.Tensor) -> torch.Tensor:
        batched = x.dim() != 1
        x, f0 = (t.unsqueeze(0) if t.dim() == 1 else t for t in (x, f0))
        if x.dim() != 2:
            raise ValueError("Input must be 1D or 2D tensor.")
        if f0.dim() != 2:
            raise ValueError("F0 must be 1D or 2D tensor.")

        e = self.extractor
        cfg = (e.frame_period, e.sample_rate, e.window_length_ms, e.eps, self.lower_bound, self.upper_bound, self.out_format)
        ap = ops.AperiodicityFn.apply(x, f0, e.window, e.window_sqrt, getattr(e, "interp_indices", None),
                                      getattr(e, "interp_weights", None), cfg)
        return ap if batched else ap.squeeze(0)
