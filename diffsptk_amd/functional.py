"""Functional API: one free function per module, each delegating to ``Module._func``
(reference: diffsptk/functional.py:23,797,859,905,1659,1700,1956,2916,2963,3142)."""
from __future__ import annotations

import functools

from torch import Tensor

from . import modules as nn
from .modules.excite import ExcitationGeneration   # (not a name of modules.__all__ yet, as the next one)
from .modules.mlsacheck import MLSADigitalFilterStabilityCheck   # (not a name of modules.__all__ yet: modules/mlsacheck.py)
from .modules.imdct import InverseModifiedDiscreteCosineTransform, InverseModifiedDiscreteSineTransform   # (the same)
from .modules.mdct import ModifiedDiscreteCosineTransform, ModifiedDiscreteSineTransform
from .modules.delta import Delta
from .modules.dtw import DynamicTimeWarping
from .modules.mcpf import MelCepstrumPostfiltering
from .modules.mlpg import MaximumLikelihoodParameterGeneration
from .modules.yingram import Yingram


def acorr(x: Tensor, acr_order: int, out_format: str | int = "naive") -> Tensor:
    """Autocorrelation of framed waveforms x:(..., L) -> (..., M+1)."""
    return nn.Autocorrelation._func(x, acr_order=acr_order, out_format=out_format)


def fftr(x: Tensor, fft_length: int | None = None, out_format: str | int = "complex") -> Tensor:
    """Real FFT x:(..., L) -> (..., fft_length/2+1)."""
    return nn.RealValuedFastFourierTransform._func(x, fft_length=fft_length, out_format=out_format)


def frame(x: Tensor, frame_length: int = 400, frame_period: int = 80, center: bool = True,
          zmean: bool = False, mode: str = "constant") -> Tensor:
    """Framing x:(..., T) -> (..., T/P, L)."""
    return nn.Frame._func(x, frame_length, frame_period, center=center, zmean=zmean, mode=mode)


def dct(x: Tensor, dct_type: int = 2) -> Tensor:
    """Discrete cosine transform x:(..., L) -> (..., L)."""
    return nn.DiscreteCosineTransform._func(x, dct_type=dct_type)


def fbank(x: Tensor, n_channel: int, sample_rate: int, f_min: float = 0, f_max: float | None = None,
          floor: float = 1e-5, gamma: float = 0, scale: str = "htk", erb_factor: float | None = None,
          use_power: bool = False, out_format: str | int = "y"):
    """Mel filter-bank analysis of power spectra x:(..., L/2+1) -> (..., C) (and log energy)."""
    return nn.MelFilterBankAnalysis._func(x, n_channel=n_channel, sample_rate=sample_rate, f_min=f_min, f_max=f_max,
                                          floor=floor, gamma=gamma, scale=scale, erb_factor=erb_factor,
                                          use_power=use_power, out_format=out_format)


def mfcc(x: Tensor, mfcc_order: int, n_channel: int, sample_rate: int, lifter: int = 1, f_min: float = 0,
         f_max: float | None = None, floor: float = 1e-5, gamma: float = 0, scale: str = "htk",
         erb_factor: float | None = None, out_format: str | int = "y") -> Tensor:
    """MFCC analysis of power spectra x:(..., L/2+1) -> (..., M) (+ C0 / energy)."""
    return nn.MelFrequencyCepstralCoefficientsAnalysis._func(
        x, mfcc_order=mfcc_order, n_channel=n_channel, sample_rate=sample_rate, lifter=lifter, f_min=f_min,
        f_max=f_max, floor=floor, gamma=gamma, scale=scale, erb_factor=erb_factor, out_format=out_format)


def freqt(c: Tensor, out_order: int, alpha: float = 0) -> Tensor:
    """Frequency transform c:(..., M1+1) -> (..., M2+1)."""
    return nn.FrequencyTransform._func(c, out_order=out_order, alpha=alpha)


def ifftr(y: Tensor, out_length: int | None = None) -> Tensor:
    """Inverse FFT of a half spectrum y:(..., L/2+1) complex -> (..., out_length) real."""
    return nn.RealValuedInverseFastFourierTransform._func(y, out_length=out_length)


def istft(y: Tensor, *, out_length: int | None = None, frame_length: int = 400, frame_period: int = 80,
          fft_length: int = 512, center: bool = True, window: str | int = "blackman", norm: str | int = "power",
          symmetric: bool = True) -> Tensor:
    """Inverse STFT y:(..., T/P, N/2+1) complex -> (..., T)."""
    return nn.InverseShortTimeFourierTransform._func(y, out_length, frame_length=frame_length, frame_period=frame_period,
                                                     fft_length=fft_length, center=center, window=window, norm=norm,
                                                     symmetric=symmetric)


def fftcep(x: Tensor, cep_order: int, accel: float = 0, n_iter: int = 0) -> Tensor:
    """Cepstral analysis of power spectra x:(..., L/2+1) -> (..., M+1)."""
    return nn.CepstralAnalysis._func(x, cep_order=cep_order, accel=accel, n_iter=n_iter)


def griffin(y: Tensor, *, out_length: int | None = None, frame_length: int = 400, frame_period: int = 80,
            fft_length: int = 512, center: bool = True, mode: str = "constant", window: str | int = "blackman",
            norm: str | int = "power", symmetric: bool = True, n_iter: int = 100, alpha: float = 0.99,
            beta: float = 0.99, gamma: float = 1.1, init_phase: str = "random", verbose: bool = False) -> Tensor:
    """Griffin-Lim phase reconstruction y:(..., T/P, N/2+1) power spectrogram -> (..., T)."""
    return nn.GriffinLim._func(y, out_length, frame_length=frame_length, frame_period=frame_period, fft_length=fft_length,
                               center=center, mode=mode, window=window, norm=norm, symmetric=symmetric, n_iter=n_iter,
                               alpha=alpha, beta=beta, gamma=gamma, init_phase=init_phase, verbose=verbose)


def unframe(y: Tensor, out_length: int | None = None, *, frame_period: int = 80, center: bool = True,
            window: str | int = "rectangular", norm: str | int = "none", symmetric: bool = True) -> Tensor:
    """Overlap-add framed waveforms y:(..., T/P, L) -> (..., T)."""
    return nn.Unframe._func(y, out_length, frame_period=frame_period, center=center, window=window, norm=norm,
                            symmetric=symmetric)


def levdur(r: Tensor, eps: float | None = None) -> Tensor:
    """Solve the Yule-Walker system r:(..., M+1) -> gain and LPC coefficients (..., M+1)."""
    return nn.LevinsonDurbin._func(r, eps=eps)


def lpc(x: Tensor, lpc_order: int, eps: float | None = None) -> Tensor:
    """LPC analysis of framed waveforms x:(..., L) -> (..., M+1)."""
    return nn.LinearPredictiveCodingAnalysis._func(x, lpc_order=lpc_order, eps=eps)


def mcep(x: Tensor, cep_order: int, alpha: float = 0, n_iter: int = 0) -> Tensor:
    """Mel-cepstral analysis of power spectra x:(..., L/2+1) -> (..., M+1)."""
    return nn.MelCepstralAnalysis._func(x, cep_order=cep_order, alpha=alpha, n_iter=n_iter)


def spec(b: Tensor | None = None, a: Tensor | None = None, *, fft_length: int = 512, eps: float = 0,
         relative_floor: float | None = None, out_format: str | int = "power") -> Tensor:
    """Spectrum of K B(z)/A(z): (..., M+1), (..., N+1) -> (..., L/2+1)."""
    return nn.Spectrum._func(b, a, fft_length=fft_length, eps=eps, relative_floor=relative_floor,
                             out_format=out_format)


def stft(x: Tensor, *, frame_length: int = 400, frame_period: int = 80, fft_length: int = 512,
         center: bool = True, zmean: bool = False, mode: str = "constant", window: str | int = "blackman",
         norm: str | int = "power", symmetric: bool = True, eps: float = 1e-9,
         relative_floor: float | None = None, out_format: str | int = "power") -> Tensor:
    """Short-time Fourier transform x:(..., T) -> (..., T/P, N/2+1)."""
    return nn.ShortTimeFourierTransform._func(
        x, frame_length=frame_length, frame_period=frame_period, fft_length=fft_length, center=center,
        zmean=zmean, mode=mode, window=window, norm=norm, symmetric=symmetric, eps=eps,
        relative_floor=relative_floor, out_format=out_format)


def window(x: Tensor, out_length: int | None = None, *, window: str | int = "blackman",
           norm: str | int = "power", symmetric: bool = True) -> Tensor:
    """Windowing x:(..., L1) -> (..., L2)."""
    return nn.Window._func(x, out_length, window=window, norm=norm, symmetric=symmetric)


# ----------------------------------------------------------------------------- SURVEY 8(f) rows 3-4
def mc2b(mc: Tensor, alpha: float = 0) -> Tensor:
    """Mel-cepstrum -> MLSA digital filter coefficients (functional.py:1936)."""
    return nn.MelCepstrumToMLSADigitalFilterCoefficients._func(mc, alpha=alpha)


def b2mc(b: Tensor, alpha: float = 0) -> Tensor:
    """MLSA digital filter coefficients -> mel-cepstrum (functional.py:86)."""
    return nn.MLSADigitalFilterCoefficientsToMelCepstrum._func(b, alpha=alpha)


def gnorm(x: Tensor, gamma: float = 0, c: int | None = None) -> Tensor:
    """Gain normalisation of a generalized cepstrum (functional.py:961)."""
    return nn.GeneralizedCepstrumGainNormalization._func(x, gamma=gamma, c=c)


def ignorm(y: Tensor, gamma: float = 0, c: int | None = None) -> Tensor:
    """Inverse gain normalisation (functional.py:1387)."""
    return nn.GeneralizedCepstrumInverseGainNormalization._func(y, gamma=gamma, c=c)


def mgc2mgc(mc: Tensor, out_order: int, in_alpha: float = 0, out_alpha: float = 0, in_gamma: float = 0,
            out_gamma: float = 0, in_norm: bool = False, out_norm: bool = False, in_mul: bool = False,
            out_mul: bool = False, n_fft: int = 512) -> Tensor:
    """Mel-generalized cepstrum conversion (functional.py:2186)."""
    return nn.MelGeneralizedCepstrumToMelGeneralizedCepstrum._func(
        mc, out_order=out_order, in_alpha=in_alpha, out_alpha=out_alpha, in_gamma=in_gamma, out_gamma=out_gamma,
        in_norm=in_norm, out_norm=out_norm, in_mul=in_mul, out_mul=out_mul, n_fft=n_fft)


def mgc2sp(mc: Tensor, fft_length: int, alpha: float = 0, gamma: float = 0, norm: bool = False, mul: bool = False,
           n_fft: int = 512, out_format: str | int = "power") -> Tensor:
    """Mel-generalized cepstrum -> spectrum (functional.py:2257)."""
    return nn.MelGeneralizedCepstrumToSpectrum._func(mc, fft_length=fft_length, alpha=alpha, gamma=gamma, norm=norm,
                                                     mul=mul, n_fft=n_fft, out_format=out_format)


def mgcep(x: Tensor, cep_order: int, alpha: float = 0, gamma: float = 0, c: int | None = None, n_iter: int = 0) -> Tensor:
    """Mel-generalized cepstral analysis of power spectra (functional.py: mgcep).  A module underneath (the reference's
    is a BaseNonFunctionalModule too): the composed matrices are cached per configuration by tables.mgcep_matrices."""
    return _mgcep_module(2 * x.size(-1) - 2, cep_order, float(alpha), float(gamma), c, n_iter, x.device, x.dtype)(x)


@functools.lru_cache(maxsize=16)
def _mgcep_module(fft_length, cep_order, alpha, gamma, c, n_iter, device, dtype):
    # one module per (configuration, device, dtype): a call does not upload the composed matrices again
    return nn.MelGeneralizedCepstralAnalysis(fft_length=fft_length, cep_order=cep_order, alpha=alpha, gamma=gamma, c=c,
                                             n_iter=n_iter, device=device, dtype=dtype)


def zerodf(x: Tensor, b: Tensor, frame_period: int = 80, ignore_gain: bool = False, zeroth_index: int = 0,
           mode: str = "direct") -> Tensor:
    """Time-variant all-zero filter (functional.py:3250-3294: zerodf)."""
    return nn.AllZeroDigitalFilter._func(x, b, frame_period=frame_period, ignore_gain=ignore_gain,
                                         zeroth_index=zeroth_index, mode=mode)


def plp(x: Tensor, plp_order: int, n_channel: int, sample_rate: int, compression_factor: float = 0.33, lifter: int = 1,
        f_min: float = 0, f_max: float | None = None, floor: float = 1e-5, gamma: float = 0, scale: str = "htk",
        erb_factor: float | None = None, n_fft: int = 512, out_format: str = "y") -> Tensor:
    """PLP analysis of power spectra x:(..., L/2+1) -> (..., M) (+ C0 / energy) (functional.py: plp)."""
    return nn.PerceptualLinearPredictiveCoefficientsAnalysis._func(
        x, plp_order=plp_order, n_channel=n_channel, sample_rate=sample_rate, compression_factor=compression_factor,
        lifter=lifter, f_min=f_min, f_max=f_max, floor=floor, gamma=gamma, scale=scale, erb_factor=erb_factor, n_fft=n_fft,
        out_format=out_format)


def poledf(x: Tensor, a: Tensor, frame_period: int = 80, ignore_gain: bool = False) -> Tensor:
    """Time-variant all-pole filter (functional.py: poledf)."""
    return nn.AllPoleDigitalFilter._func(x, a, frame_period=frame_period, ignore_gain=ignore_gain)


def decimate(x: Tensor, period: int = 1, start: int = 0, dim: int = -1) -> Tensor:
    """Decimation (functional.py: decimate): the view x[..., start::period, ...] along dim."""
    return nn.Decimation._func(x, period=period, start=start, dim=dim)


def interpolate(x: Tensor, period: int = 1, start: int = 0, dim: int = -1) -> Tensor:
    """Interpolation (functional.py: interpolate): zeros with x[n] at start + n period along dim."""
    return nn.Interpolation._func(x, period=period, start=start, dim=dim)


def linear_intpl(x: Tensor, upsampling_factor: int = 80) -> Tensor:
    """Linear interpolation of frame-wise parameters (functional.py: linear_intpl)."""
    return nn.LinearInterpolation._func(x, upsampling_factor=upsampling_factor)


def lpc2par(a: Tensor, gamma: float = 1, c: int | None = None) -> Tensor:
    """LPC -> PARCOR coefficients a:(..., M+1) -> (..., M+1) (functional.py: lpc2par)."""
    return nn.LinearPredictiveCoefficientsToParcorCoefficients._func(a, gamma=gamma, c=c)


def par2lpc(k: Tensor, gamma: float = 1, c: int | None = None) -> Tensor:
    """PARCOR -> LPC coefficients k:(..., M+1) -> (..., M+1) (functional.py: par2lpc)."""
    return nn.ParcorCoefficientsToLinearPredictiveCoefficients._func(k, gamma=gamma, c=c)


def lpccheck(a: Tensor, margin: float = 1e-16, warn_type: str = "warn") -> Tensor:
    """Stability check of LPC coefficients a:(..., M+1) -> (..., M+1) (functional.py: lpccheck)."""
    return nn.LinearPredictiveCoefficientsStabilityCheck._func(a, margin=margin, warn_type=warn_type)


def lpc2lsp(a: Tensor, log_gain: bool = False, sample_rate: int | None = None, out_format: str = "radian") -> Tensor:
    """LPC coefficients -> line spectral pairs a:(..., M+1) -> (..., M+1) (functional.py: lpc2lsp)."""
    return nn.LinearPredictiveCoefficientsToLineSpectralPairs._func(a, log_gain=log_gain, sample_rate=sample_rate, out_format=out_format)


def lsp2lpc(w: Tensor, log_gain: bool = False, sample_rate: int | None = None, in_format: str = "radian") -> Tensor:
    """Line spectral pairs -> LPC coefficients w:(..., M+1) -> (..., M+1) (functional.py: lsp2lpc)."""
    return nn.LineSpectralPairsToLinearPredictiveCoefficients._func(w, log_gain=log_gain, sample_rate=sample_rate, in_format=in_format)


def lspcheck(w: Tensor, rate: float = 0, n_iter: int = 1, warn_type: str = "warn") -> Tensor:
    """Stability check of line spectral pairs w:(..., M+1) -> (..., M+1) (functional.py: lspcheck)."""
    return nn.LineSpectralPairsStabilityCheck._func(w, rate=rate, n_iter=n_iter, warn_type=warn_type)


def mlsacheck(c: Tensor, *, alpha: float = 0, pade_order: int = 4, strict: bool = True, threshold: float | None = None, fast: bool = True,
              n_fft: int = 256, warn_type: str = "warn", mod_type: str = "scale") -> Tensor:
    """Stability check of the MLSA digital filter c:(..., M+1) -> (..., M+1) (functional.py: mlsacheck)."""
    return MLSADigitalFilterStabilityCheck._func(c, alpha=alpha, pade_order=pade_order, strict=strict, threshold=threshold, fast=fast,
                                                 n_fft=n_fft, warn_type=warn_type, mod_type=mod_type)


def excite(p: Tensor, frame_period: int = 80, *, voiced_region: str = "pulse", unvoiced_region: str = "gauss", polarity: str = "auto",
           init_phase: str | float = "zeros") -> Tensor:
    """Excitation from pitch p:(..., N) in samples, 0 = unvoiced -> (..., N P) (functional.py: excite)."""
    return ExcitationGeneration._func(p, frame_period=frame_period, voiced_region=voiced_region, unvoiced_region=unvoiced_region,
                                      polarity=polarity, init_phase=init_phase)


def par2lar(k: Tensor) -> Tensor:
    """PARCOR coefficients -> log area ratio (functional.py: par2lar)."""
    return nn.ParcorCoefficientsToLogAreaRatio._func(k)


def lar2par(g: Tensor) -> Tensor:
    """Log area ratio -> PARCOR coefficients (functional.py: lar2par)."""
    return nn.LogAreaRatioToParcorCoefficients._func(g)


def par2is(k: Tensor) -> Tensor:
    """PARCOR coefficients -> inverse sine coefficients (functional.py: par2is)."""
    return nn.ParcorCoefficientsToInverseSine._func(k)


def is2par(s: Tensor) -> Tensor:
    """Inverse sine coefficients -> PARCOR coefficients (functional.py: is2par)."""
    return nn.InverseSineToParcorCoefficients._func(s)


def mdct(x: Tensor, frame_length: int = 400, window: str = "sine") -> Tensor:
    """Modified discrete cosine transform x:(..., T) -> (..., 2T/L, L/2) (functional.py: mdct)."""
    return ModifiedDiscreteCosineTransform._func(x, frame_length=frame_length, window=window)


def mdst(x: Tensor, frame_length: int = 400, window: str = "sine") -> Tensor:
    """Modified discrete sine transform x:(..., T) -> (..., 2T/L, L/2) (functional.py: mdst)."""
    return ModifiedDiscreteSineTransform._func(x, frame_length=frame_length, window=window)


def imdct(y: Tensor, out_length: int | None = None, frame_length: int = 400, window: str = "sine") -> Tensor:
    """Inverse modified discrete cosine transform y:(..., 2T/L, L/2) -> (..., T) (functional.py: imdct)."""
    return InverseModifiedDiscreteCosineTransform._func(y, out_length=out_length, frame_length=frame_length, window=window)


def imdst(y: Tensor, out_length: int | None = None, frame_length: int = 400, window: str = "sine") -> Tensor:
    """Inverse modified discrete sine transform y:(..., 2T/L, L/2) -> (..., T) (functional.py: imdst)."""
    return InverseModifiedDiscreteSineTransform._func(y, out_length=out_length, frame_length=frame_length, window=window)


def delta(x: Tensor, seed=[[-0.5, 0, 0.5]], static_out: bool = True) -> Tensor:
    """Delta components x:(B, T, D) or (T, D) -> (B, T, DxH) or (T, DxH) (functional.py: delta)."""
    return Delta._func(x, seed=seed, static_out=static_out)


def mlpg(u: Tensor, seed=[[-0.5, 0, 0.5], [1, -2, 1]]) -> Tensor:
    """Maximum likelihood parameter generation u:(..., T, DxH) -> (..., T, D) (functional.py: mlpg); the banded factor is cached
    per (T, seed, device, dtype)."""
    return MaximumLikelihoodParameterGeneration._func(u, seed=seed)


def mcpf(mc: Tensor, alpha: float = 0, beta: float = 0, onset: int = 2, ir_length: int = 128) -> Tensor:
    """Mel-cepstrum postfiltering mc:(..., M+1) -> (..., M+1) (functional.py: mcpf)."""
    return MelCepstrumPostfiltering._func(mc, alpha=alpha, beta=beta, onset=onset, ir_length=ir_length)


def dtw(x: Tensor, y: Tensor, lengths: Tensor | None = None, return_indices: bool = False, metric: str | int = "euclidean", p: int = 4,
        softness: float = 1e-3) -> Tensor | tuple[Tensor, list[Tensor]]:
    """Dynamic time warping distance of x:(B, T1, D) and y:(B, T2, D) -> (B,), and the Viterbi paths on request (functional.py: dtw)."""
    return DynamicTimeWarping._func(x, y, lengths=lengths, return_indices=return_indices, metric=metric, p=p, softness=softness)


def dtw_merge(x: Tensor, y: Tensor, indices: Tensor) -> Tensor:
    """The frames of x:(T1, D) and y:(T2, D) along a Viterbi path indices:(T, 2) -> (T, 2D) (functional.py: dtw_merge)."""
    return DynamicTimeWarping.merge(x=x, y=y, indices=indices)


def yingram(x: Tensor, sample_rate: int = 22050, lag_min: int = 22, lag_max: int | None = None, n_bin: int = 20) -> Tensor:
    """The Yingram of framed waveforms x:(..., L) -> (..., M) (functional.py: yingram)."""
    return Yingram._func(x, sample_rate=sample_rate, lag_min=lag_min, lag_max=lag_max, n_bin=n_bin)
