"""An entry given a dtype code it does not know refuses under its own name: status DSA_ERR_UNSUPPORTED and the message
"<name>: unsupported dtype", whichever way the sources spell that refusal (csrc/common.h: with_dtype).  The refusal comes before any
HIP call, so this runs without a device; where one is visible the pointers are device memory, so that an entry that wrongly went on
would launch inside the buffer with the tiny sizes of its row."""
import ctypes as C
import glob
import os
import re

import pytest

from diffsptk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "diffsptk_amd", "csrc", "*.h*")))}
BAD_DTYPE = 99
BUFFER_BYTES = 1 << 16

# entry -> (the name its refusal speaks, the sizes of the call by parameter name).  Two rows or frames, lengths of at most 32; what a
# row does not name: `dtype` is BAD_DTYPE, every pointer is the one zeroed buffer, the stream is NULL, a double is 0.5, another
# integer (a flag, a format, a mode, DSA_ALGO_AUTO) is 0.  A pointer a row names stands that many bytes into the buffer.
SPEC = dict(lb=2, la=2, F=2, nfft=16)
STFT = dict(B=2, T=32, L=8, P=4, nfft=16, center=1)
FILT = dict(B=2, T=16, M=2, P=1)
ROWS = {
    "dsa_frame_fwd": ("frame", dict(B=2, T=32, L=8, P=4, center=1)),
    "dsa_frame_bwd": ("frame_bwd", dict(B=2, T=32, L=8, P=4, center=1)),
    "dsa_window_fwd": ("window", dict(F=2, L=8, L2=8)),
    "dsa_window_bwd": ("window_bwd", dict(F=2, L=8, L2=8)),
    "dsa_fftr_fwd": ("fftr", dict(F=2, len_in=8, nfft=16)),
    "dsa_fftr_bwd": ("fftr_bwd", dict(F=2, len_in=8, nfft=16)),
    "dsa_spec_fwd": ("spec", SPEC),
    "dsa_spec_bwd": ("spec_bwd", SPEC),
    "dsa_stft_fwd": ("stft", STFT),
    "dsa_stft_bwd": ("stft_bwd", STFT),
    "dsa_freqt_fwd": ("freqt", dict(F=2, L1=4, L2=4)),
    "dsa_freqt_bwd": ("freqt_bwd", dict(F=2, L1=4, L2=4)),
    "dsa_fbank_fwd": ("fbank", dict(F=2, K=9, C=4)),
    "dsa_fbank_bwd": ("fbank_bwd", dict(F=2, K=9, C=4)),
    "dsa_irfft_scale": ("irfft_scale", dict(F=2, nfft=16)),
    "dsa_div_rows": ("div_rows", dict(B=2, T=16)),
    "dsa_griffin_update": ("griffin_update", dict(B=2, Nt=16, N=2, K=9)),
    "dsa_fftcep_fwd": ("fftcep", dict(F=2, fft_length=16, cep_order=3, n_iter=1)),
    "dsa_fftcep_bwd": ("fftcep_bwd", dict(F=2, fft_length=16, cep_order=3, n_iter=1)),
    "dsa_mcep_fwd": ("mcep", dict(F=2, nfft=16, M=3, n_iter=1)),
    "dsa_mcep_bwd": ("mcep_bwd", dict(F=2, nfft=16, M=3, n_iter=1)),
    "dsa_gnorm_fwd": ("gnorm", dict(F=2, n=4)),
    "dsa_mgcep_gain": ("mgcep_gain", dict(F=2, M=3)),
    "dsa_mgcep_spectra": ("mgcep_spectra", dict(F=2, fft_length=16, M=3, gamma=-0.5)),
    "dsa_thsolve_fwd": ("thsolve", dict(F=2, n=4)),
    "dsa_thsolve_bwd": ("thsolve_bwd", dict(F=2, n=4)),
    "dsa_zerodf_fwd": ("zerodf", FILT),
    "dsa_zerodf_bwd": ("zerodf_bwd", FILT),
    "dsa_zerodf_taylor_fwd": ("zerodf_taylor", FILT),
    "dsa_zerodf_taylor_bwd": ("zerodf_taylor_bwd", dict(FILT, G_out=BUFFER_BYTES // 2)),   # (a buffer of its own)
    "dsa_poledf_fwd": ("poledf", FILT),
    "dsa_poledf_bwd": ("poledf_bwd", FILT),
    "dsa_plp_fwd": ("plp", dict(F=2, C=8, M=3, N=16)),
    "dsa_plp_bwd": ("plp_bwd", dict(F=2, C=8, M=3, N=16)),
    "dsa_pqmf_fwd": ("pqmf", dict(B=2, T=16, K=2, M=4, period=1)),
    "dsa_pqmf_bwd": ("pqmf_bwd", dict(B=2, T=16, K=2, M=4, period=1)),
    "dsa_ipqmf_fwd": ("ipqmf", dict(B=2, T=16, K=2, M=4, up=1)),
    "dsa_ipqmf_bwd": ("ipqmf_bwd", dict(B=2, T=16, K=2, M=4, up=1)),
    "dsa_interpolate_fwd": ("interpolate", dict(outer=2, T=8, inner=1, period=2)),
    "dsa_interpolate_bwd": ("interpolate_bwd", dict(outer=2, T=8, inner=1, period=2)),
    "dsa_acorr_fwd": ("acorr", dict(F=2, L=8, M=3)),
    "dsa_acorr_bwd": ("acorr_bwd", dict(F=2, L=8, M=3)),
    "dsa_levdur_fwd": ("levdur", dict(F=2, M=3)),
    "dsa_levdur_bwd": ("levdur_bwd", dict(F=2, M=3)),
    "dsa_lpc_fwd": ("lpc", dict(F=2, L=8, M=3)),
    "dsa_lpc_bwd": ("lpc_bwd", dict(F=2, L=8, M=3)),
    "dsa_frame_window_lpc_fwd": ("frame_window_lpc", dict(B=2, T=32, L=8, P=4, center=1, M=3)),
    # csrc/parcor.hip and csrc/lsp.hip
    **{f"dsa_{n}": (n, dict(F=2, M=4)) for n in ("lpc2par_fwd", "lpc2par_bwd", "par2lpc_fwd", "par2lpc_bwd", "lpccheck_fwd", "lpccheck_bwd",
                                                 "lpc2lsp_fwd", "lpc2lsp_bwd", "lsp2lpc_fwd", "lsp2lpc_bwd")},
    "dsa_lspcheck_fwd": ("lspcheck_fwd", dict(F=2, M=4, n_iter=1)),
    "dsa_lspcheck_bwd": ("lspcheck_bwd", dict(F=2, M=4, n_iter=1)),
}
LEFT_OUT = {}   # name -> the HIP runtime call its entry makes before it looks at dtype: none

# the names that reach the refusal through a variable: name -> (file, the launcher that forwards it)
FORWARDED = {
    **{n: ("parcor.hip", "parcor_launch") for n in ("lpc2par_fwd", "lpc2par_bwd", "par2lpc_fwd", "par2lpc_bwd", "lpccheck_fwd", "lpccheck_bwd")},
    **{n: ("lsp.hip", "lsp_lane_launch") for n in ("lsp2lpc_fwd", "lsp2lpc_bwd", "lspcheck_fwd", "lspcheck_bwd")},
}
# names given to the dispatch helper by entries that never reach its refusal: their own check comes first, with another status
# ("<name>: unknown dtype", DSA_ERR_INVALID_ARGUMENT; tests of their own hold it).  name -> the file whose check that is
UNREACHED = {"world_synth": "world_synth.hip", "ap": "ap.hip", "yingram": "yingram.hip", "gmm": "gmm.hip", "dtw": "dtw.hip", "vq": "vq.hip",
             "mdct analysis": "mdct.hip", "mdct synthesis": "mdct.hip", "excite": "excite.hip", "delta": "paramgen.hip", "mlpg": "paramgen.hip",
             "mcpf": "paramgen.hip"}


def parameters(entry):
    """[(type, name)] of the entry's prototype in the C header"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(_lib.HEADER).read(), flags=re.S)
    inside = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % entry, text).group(1)
    return [re.fullmatch(r"\s*(.+?)\s*\b(\w+)\s*", p).groups() for p in inside.split(",")]


def spelled_names(texts):
    """the names whose dtype refusal the sources spell as a literal: in the refusal itself ("name: unsupported dtype", or the name
    right behind the shared format), or as the `what` of the dispatch helper"""
    found = set()
    for text in texts.values():
        found |= set(re.findall(r'"(\w+): unsupported dtype(?:%s)?"', text))
        found |= set(re.findall(r'"%s: unsupported dtype"\s*,\s*"(\w+)"', text))
        found |= set(re.findall(r'\bwith_dtype\(\s*\w+\s*,\s*"([^"]+)"', text))
    return found


def test_the_rows_are_the_names_the_sources_refuse_by():
    assert spelled_names({"a.hip": 'fail(DSA_ERR_UNSUPPORTED, "x: unsupported dtype%s"); fail(E, "%s: unsupported dtype", "y");\n'
                                   'return with_dtype(dtype, "z", [&](auto tag) {'}) == {"x", "y", "z"}
    for name, (file, launcher) in FORWARDED.items():
        assert re.search(r'\b%s<\w+>\("%s"' % (launcher, name), CSRC[file]), f"{file}: {launcher} is not given \"{name}\""
        forwards = re.search(r"\b%s\(const char\* what\b[^{;]*\{.*?^\}" % launcher, CSRC[file], re.S | re.M).group(0)
        assert re.search(r'unsupported dtype", what\)|\bwith_dtype\(\s*dtype\s*,\s*what\b', forwards), f"{file}: {launcher} does not forward its name"
    spelled = spelled_names(CSRC)
    for name, file in UNREACHED.items():
        assert re.search(r'fail\(DSA_ERR_INVALID_ARGUMENT, "(%s|%%s): unknown dtype"' % name, CSRC[file]), f"{file} has no check of its own for \"{name}\""
    assert not set(FORWARDED) & spelled and not set(UNREACHED) & {name for name, _ in ROWS.values()}
    assert (spelled - set(UNREACHED)) | set(FORWARDED) == {name for name, _ in ROWS.values()} | set(LEFT_OUT)
    assert len(ROWS) == 59 and len(LEFT_OUT) <= 3 and len({name for name, _ in ROWS.values()}) == len(ROWS)


@pytest.fixture(scope="module")
def zeroed():
    """(address, owner) of one zeroed 64 KB buffer: device memory where a device is visible"""
    import torch

    if torch.cuda.is_available():
        t = torch.zeros(BUFFER_BYTES, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t.data_ptr(), t
    buf = C.create_string_buffer(BUFFER_BYTES)
    return C.addressof(buf), buf


@pytest.mark.parametrize("entry", sorted(ROWS))
def test_an_unknown_dtype_is_refused_by_the_entry_s_name(entry, zeroed):
    name, sizes = ROWS[entry]
    lib = _lib.load()
    params = parameters(entry)
    assert set(sizes) <= {p for _, p in params}, (entry, sizes)
    args = []
    for ctype, p in params:
        if p == "stream":
            args.append(None)
        elif ctype.endswith("*"):
            args.append(zeroed[0] + sizes.get(p, 0))
        elif p == "dtype":
            args.append(BAD_DTYPE)
        else:
            args.append(sizes.get(p, 0.5) if ctype == "double" else sizes.get(p, 0))
    assert all(sizes.get(p, 0) <= 32 for ctype, p in params if ctype.startswith("int"))
    rc = getattr(lib, entry)(*args)
    assert (rc, lib.dsa_last_error().decode()) == (_lib.ERR_UNSUPPORTED, f"{name}: unsupported dtype")
