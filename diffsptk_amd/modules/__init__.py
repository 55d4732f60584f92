from .acorr import Autocorrelation
from .base import BaseFunctionalModule, Precomputed
from .dct import DiscreteCosineTransform
from .dct import DiscreteCosineTransform as DCT
from .decimate import Decimation, Interpolation
from .fbank import MelFilterBankAnalysis
from .fbank import MelFilterBankAnalysis as FBANK
from .fftcep import CepstralAnalysis
from .fftr import RealValuedFastFourierTransform
from .frame import Frame
from .griffin import GriffinLim
from .ifftr import RealValuedInverseFastFourierTransform
from .istft import InverseShortTimeFourierTransform
from .istft import InverseShortTimeFourierTransform as ISTFT
from .freqt import FrequencyTransform
from .levdur import LevinsonDurbin
from .lpc import LinearPredictiveCodingAnalysis
from .lpc import LinearPredictiveCodingAnalysis as LPC
from .fused import FusedFrameWindowLPC, FusedInterpolationIPQMF, FusedPQMFDecimation, FusedSTFTFilterBank, FusedSTFTMelCepstralAnalysis, fuse
from .gnorm import GeneralizedCepstrumGainNormalization, GeneralizedCepstrumInverseGainNormalization
from .mc2b import MelCepstrumToMLSADigitalFilterCoefficients, MLSADigitalFilterCoefficientsToMelCepstrum
from .mcep import MelCepstralAnalysis
from .mgc2mgc import MelGeneralizedCepstrumToMelGeneralizedCepstrum
from .mgc2sp import MelGeneralizedCepstrumToSpectrum
from .mgcep import MelGeneralizedCepstralAnalysis
from .mglsadf import PseudoMGLSADigitalFilter
from .mglsadf import PseudoMGLSADigitalFilter as MLSA
from .plp import PerceptualLinearPredictiveCoefficientsAnalysis
from .plp import PerceptualLinearPredictiveCoefficientsAnalysis as PLP
from .poledf import AllPoleDigitalFilter
from .lpc2par import LinearPredictiveCoefficientsToParcorCoefficients
from .par2lpc import ParcorCoefficientsToLinearPredictiveCoefficients
from .lpccheck import LinearPredictiveCoefficientsStabilityCheck
from .par2lar import ParcorCoefficientsToLogAreaRatio
from .lar2par import LogAreaRatioToParcorCoefficients
from .par2is import ParcorCoefficientsToInverseSine
from .is2par import InverseSineToParcorCoefficients
from .lpc2lsp import LinearPredictiveCoefficientsToLineSpectralPairs
from .lsp2lpc import LineSpectralPairsToLinearPredictiveCoefficients
from .lspcheck import LineSpectralPairsStabilityCheck
from .pqmf import PseudoQuadratureMirrorFilterBankAnalysis, PseudoQuadratureMirrorFilterBankSynthesis
from .pqmf import PseudoQuadratureMirrorFilterBankAnalysis as PQMF
from .pqmf import PseudoQuadratureMirrorFilterBankSynthesis as IPQMF
from .zerodf import AllZeroDigitalFilter, LinearInterpolation
from .mfcc import MelFrequencyCepstralCoefficientsAnalysis
from .mfcc import MelFrequencyCepstralCoefficientsAnalysis as MFCC
from .spec import Spectrum
from .stft import ShortTimeFourierTransform
from .stft import ShortTimeFourierTransform as STFT
from .unframe import Unframe
from .window import Window

__all__ = [
    "Autocorrelation", "BaseFunctionalModule", "CepstralAnalysis", "DCT", "DiscreteCosineTransform", "FBANK", "Frame", "GriffinLim",
    "FrequencyTransform", "ISTFT", "InverseShortTimeFourierTransform", "RealValuedInverseFastFourierTransform", "Unframe", "LPC", "LevinsonDurbin", "LinearPredictiveCodingAnalysis", "MFCC", "MelCepstralAnalysis",
    "MelFilterBankAnalysis", "MelFrequencyCepstralCoefficientsAnalysis", "Precomputed",
    "GeneralizedCepstrumGainNormalization", "GeneralizedCepstrumInverseGainNormalization",
    "MelCepstrumToMLSADigitalFilterCoefficients", "MLSADigitalFilterCoefficientsToMelCepstrum",
    "MelGeneralizedCepstrumToMelGeneralizedCepstrum", "MelGeneralizedCepstrumToSpectrum", "MelGeneralizedCepstralAnalysis",
    "PseudoMGLSADigitalFilter", "MLSA", "PerceptualLinearPredictiveCoefficientsAnalysis", "PLP", "AllPoleDigitalFilter", "AllZeroDigitalFilter", "LinearInterpolation",
    "FusedFrameWindowLPC", "FusedSTFTFilterBank", "FusedSTFTMelCepstralAnalysis", "fuse",
    "Decimation", "Interpolation", "PQMF", "IPQMF", "PseudoQuadratureMirrorFilterBankAnalysis",
    "PseudoQuadratureMirrorFilterBankSynthesis", "FusedPQMFDecimation", "FusedInterpolationIPQMF",
    "LinearPredictiveCoefficientsToParcorCoefficients", "ParcorCoefficientsToLinearPredictiveCoefficients",
    "LinearPredictiveCoefficientsStabilityCheck", "ParcorCoefficientsToLogAreaRatio", "LogAreaRatioToParcorCoefficients",
    "ParcorCoefficientsToInverseSine", "InverseSineToParcorCoefficients",
    "LinearPredictiveCoefficientsToLineSpectralPairs", "LineSpectralPairsToLinearPredictiveCoefficients", "LineSpectralPairsStabilityCheck",
    "RealValuedFastFourierTransform", "STFT", "ShortTimeFourierTransform", "Spectrum", "Window",
]
