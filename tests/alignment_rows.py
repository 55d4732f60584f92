"""The alignment sweep's table, names only: one row per public module class (diffsptk_amd/modules/__init__.py; every free function
of functional.py delegates to one of them) -> the `dsa_*_fwd` / `dsa_*_bwd` entries of include/diffsptk_amd.h that the module's forward
and backward reach with the caller's tensors.  tests/test_gpu_alignment.py runs every row with tensors that are only
element-aligned and checks that the entries a row names are really called; tests/test_alignment_cpu.py checks, without a GPU, that
no entry and no module is left out.  A family added later has to appear here (or in EXEMPT, with a reason) before the suite passes.

A row may name an entry that another row names too (the inverse transforms run on the backward entries of the analysis ops)."""

ROWS = {
    # csrc/spec.hip, stft.hip, griffin.hip
    "Frame": ("dsa_frame_fwd", "dsa_frame_bwd"),
    "Window": ("dsa_window_fwd", "dsa_window_bwd"),
    "RealValuedFastFourierTransform": ("dsa_fftr_fwd", "dsa_fftr_bwd"),
    "RealValuedInverseFastFourierTransform": ("dsa_fftr_bwd", "dsa_fftr_fwd"),
    "Spectrum": ("dsa_spec_fwd", "dsa_spec_bwd"),
    "ShortTimeFourierTransform": ("dsa_stft_fwd", "dsa_stft_bwd"),
    "InverseShortTimeFourierTransform": ("dsa_istft_fwd", "dsa_stft_fwd"),
    "Unframe": ("dsa_window_fwd", "dsa_frame_bwd", "dsa_frame_fwd"),
    "GriffinLim": ("dsa_istft_fwd", "dsa_stft_fwd"),
    # csrc/lpc.hip (tuned order 24: lpc24.hip, lpc24_bwd.hip), parcor.hip, lsp.hip
    "Autocorrelation": ("dsa_acorr_fwd", "dsa_acorr_bwd"),
    "LevinsonDurbin": ("dsa_levdur_fwd", "dsa_levdur_bwd"),
    "LinearPredictiveCodingAnalysis": ("dsa_lpc_fwd", "dsa_lpc_bwd"),
    "FusedFrameWindowLPC": ("dsa_frame_window_lpc_fwd", "dsa_frame_window_lpc_bwd"),
    "LinearPredictiveCoefficientsToParcorCoefficients": ("dsa_lpc2par_fwd", "dsa_lpc2par_bwd"),
    "ParcorCoefficientsToLinearPredictiveCoefficients": ("dsa_par2lpc_fwd", "dsa_par2lpc_bwd"),
    "LinearPredictiveCoefficientsStabilityCheck": ("dsa_lpccheck_fwd", "dsa_lpccheck_bwd"),
    "ParcorCoefficientsToLogAreaRatio": (),
    "LogAreaRatioToParcorCoefficients": (),
    "ParcorCoefficientsToInverseSine": (),
    "InverseSineToParcorCoefficients": (),
    "LinearPredictiveCoefficientsToLineSpectralPairs": ("dsa_lpc2lsp_fwd", "dsa_lpc2lsp_bwd"),
    "LineSpectralPairsToLinearPredictiveCoefficients": ("dsa_lsp2lpc_fwd", "dsa_lsp2lpc_bwd"),
    "LineSpectralPairsStabilityCheck": ("dsa_lspcheck_fwd", "dsa_lspcheck_bwd"),
    # csrc/mcep.hip, rows_gemm.hip, fbank.hip, fftcep.hip, plp.hip
    "FrequencyTransform": ("dsa_freqt_fwd", "dsa_freqt_bwd"),
    "DiscreteCosineTransform": ("dsa_freqt_fwd", "dsa_freqt_bwd"),
    "MelFilterBankAnalysis": ("dsa_fbank_fwd", "dsa_fbank_bwd"),
    "MelFrequencyCepstralCoefficientsAnalysis": ("dsa_fbank_dct_fwd", "dsa_fbank_bwd"),
    "PerceptualLinearPredictiveCoefficientsAnalysis": ("dsa_plp_fwd", "dsa_plp_bwd"),
    "FusedSTFTFilterBank": ("dsa_stft_fbank_fwd", "dsa_fbank_bins_bwd"),
    "CepstralAnalysis": ("dsa_fftcep_fwd", "dsa_fftcep_bwd"),
    "MelCepstralAnalysis": ("dsa_mcep_fwd", "dsa_mcep_bwd"),
    "FusedSTFTMelCepstralAnalysis": ("dsa_stft_mcep_opts_fwd", "dsa_mcep_bwd"),
    # csrc/mgc.hip, thsolve.hip, thsolve_quad.hip
    "MelGeneralizedCepstralAnalysis": ("dsa_thsolve_fwd", "dsa_thsolve_bwd", "dsa_thsolve_update_fwd", "dsa_mgcep_step_bwd"),
    "GeneralizedCepstrumGainNormalization": ("dsa_gnorm_fwd",),
    "GeneralizedCepstrumInverseGainNormalization": ("dsa_gnorm_fwd",),
    "MelCepstrumToMLSADigitalFilterCoefficients": (),
    "MLSADigitalFilterCoefficientsToMelCepstrum": (),
    "MelGeneralizedCepstrumToMelGeneralizedCepstrum": ("dsa_gc2gc_fwd", "dsa_gc2gc_bwd"),
    "MelGeneralizedCepstrumToSpectrum": (),
    # csrc/zerodf.hip, poledf.hip, pqmf.hip
    "AllZeroDigitalFilter": ("dsa_zerodf_fwd", "dsa_zerodf_bwd"),
    "LinearInterpolation": (),
    "AllPoleDigitalFilter": ("dsa_poledf_fwd", "dsa_poledf_bwd"),
    "PseudoMGLSADigitalFilter": ("dsa_zerodf_taylor_fwd", "dsa_zerodf_taylor_bwd"),
    "Decimation": (),
    "Interpolation": ("dsa_interpolate_fwd", "dsa_interpolate_bwd"),
    "PseudoQuadratureMirrorFilterBankAnalysis": ("dsa_pqmf_fwd", "dsa_pqmf_bwd"),
    "PseudoQuadratureMirrorFilterBankSynthesis": ("dsa_ipqmf_fwd", "dsa_ipqmf_bwd"),
    "FusedPQMFDecimation": ("dsa_pqmf_fwd", "dsa_pqmf_bwd"),
    "FusedInterpolationIPQMF": ("dsa_ipqmf_fwd", "dsa_ipqmf_bwd"),
}

# `dsa_*_fwd` / `dsa_*_bwd` entries that no row names, each with the reason the sweep does not need it
EXEMPT = {
    "dsa_stft_mcep_fwd": "forwards its arguments to dsa_stft_mcep_opts_fwd (csrc/mcep.hip), which the FusedSTFTMelCepstralAnalysis row names",
    "dsa_mcep_newton_update_bwd": "one step of the 48 kHz analysis' backward: every tensor it takes is allocated by ops.McepNewtonStepsHFn, none by the caller",
    "dsa_mcep_newton_resid_h_bwd": "as dsa_mcep_newton_update_bwd: the log spectrum, iterates and cotangents are ops.McepNewtonStepsHFn's own tensors",
}

# names of diffsptk_amd.modules.__all__ that are no module of their own
NOT_A_MODULE = {
    "BaseFunctionalModule": "abstract base class",
    "Precomputed": "container of a module's precomputed tables",
    "fuse": "returns one of the Fused* modules, each of which has a row",
}
