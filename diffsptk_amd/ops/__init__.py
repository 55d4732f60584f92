"""torch.autograd.Function wrappers over the C-ABI (include/diffsptk_amd.h), one module per family of the library's sources.

PyTorch is plumbing here: it owns device memory and the stream; every computation below is a call into libdiffsptk_amd.so.
Inputs must live on a HIP device -- there is deliberately no CPU path (the reference's autograd-derived backward, SURVEY.md
section 3.5, is replaced by the hand-written backward kernels).

`ops.<name>` resolves for every name of every module below.  That is a copy of the binding: to CHANGE a tunable that is read at
call time (MCEP_GLOGX_MIN_FRAMES, MCEP_HIST_RT_MAX_BYTES), set it on the module that reads it, `ops.mcep`.
"""
from . import _core, rows, stft, fbank, lpc, filters, mgc, mcep, mdct, paramgen, dtw, gmm, yingram, vq, world, ap, pitch_spec   # import order: _core <- the families <- mcep (uses rows, mgc)

for _m in (_core, rows, stft, fbank, lpc, filters, mgc, mcep, mdct, paramgen, dtw, gmm, yingram, vq, world, ap, pitch_spec):
    globals().update({_n: _v for _n, _v in vars(_m).items() if not _n.startswith("__")})
