"""CPU-only tests of the product's host side: tables vs reference-generated goldens, option
validation (same ValueErrors as the reference), the C-ABI library (loads, exports every symbol
the header declares) and the loud failure without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import diffsptk_amd as dsp
from diffsptk_amd import _lib, functional as F
from diffsptk_amd.utils import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    _lib.build()


def test_library_exports_every_header_symbol():
    header = open(os.path.join(ROOT, "include", "diffsptk_amd.h")).read()
    declared = set(re.findall(r"\b(dsa_[a-z0-9_]+)\s*\(", header))
    declared -= {"dsa_status"}
    assert len(declared) >= 26
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, f"declared in the header but not exported: {missing}"
    assert declared == set(_lib.SIGNATURES), "the header parser of _lib missed or invented a prototype"
    exported = {n for n in _dynamic_symbols(_lib.LIB_PATH) if n.startswith("dsa_")}
    assert exported == declared, f"exported without a prototype in the header (no binding): {sorted(exported - declared)}"
    assert _lib.load().dsa_version() == int(re.search(r"#define DSA_VERSION (\d+)", header).group(1)) >= 120
    assert _lib.load().dsa_num_frames(16000, 80) == 200
    assert _lib.load().dsa_num_frames(19200, 80) == 240


def _dynamic_symbols(path):
    """Names of the symbols an ELF64 (little-endian) shared object defines in its dynamic symbol table."""
    import struct

    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type == 11:   # SHT_DYNSYM; `link` is its string table
            for at in range(offset, offset + size, entsize):
                st_name, _, _, st_shndx = struct.unpack_from("<IBBH", blob, at)
                if st_shndx != 0:   # defined here, not imported
                    start = sections[link][4] + st_name
                    names.add(blob[start:blob.index(b"\0", start)].decode())
    return names


def test_header_parser_type_mapping_spot_check():
    """Three rows spelt out by hand, so that the parser's type mapping is pinned by something that is not the parser:
    int32_t / int64_t / double / pointers, an int64_t return, typed HOST pointers (const double*, float*) as addresses."""
    P, L, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    stft = _lib.SIGNATURES["dsa_stft_fwd"]
    assert stft == (ctypes.c_int, [P, L, L, I, I, I, P, P, I, I, I, D, I, D, I, I, I, P, P])
    assert len(stft[1]) == 19 and stft[1][11] is D and stft[1][12] is I and stft[1][13] is D
    assert _lib.SIGNATURES["dsa_num_frames"] == (ctypes.c_int64, [L, I])
    assert _lib.SIGNATURES["dsa_fbank_scan_plan"] == (ctypes.c_int, [P, I, I, P])
    assert _lib.SIGNATURES["dsa_last_error"] == (ctypes.c_char_p, [])
    assert L is not I and ctypes.sizeof(L) == 8 and ctypes.sizeof(I) == 4
    header = open(os.path.join(ROOT, "include", "diffsptk_amd.h")).read()
    assert re.search(r"int dsa_fbank_scan_plan\(const double\* H_host, int32_t K, int32_t C, float\* plan_host\);", header)
    # constants: an enumerator, a negative one, a hex define and the one define that is an expression
    assert (_lib.F64, _lib.ERR_UNSUPPORTED, _lib.ALGO_HIST_HAS_RT, _lib.ALGO_TUNED) == (1, -2, 0x400, 2)
    assert _lib.MCEP_BWD_WORKSPACE_BYTES == 64 + 512 * 16 * 32 * 4 and _lib.SCRATCH_BYTES == 64
    assert "DSA_ALGO_RESERVE_CUS" not in _lib.CONSTANTS and _lib.algo_reserve_cus(65) == 1 << 16   # function-like: stays Python


def test_header_parser_on_snippets(tmp_path):
    sig, const = _lib.parse_header("""
        /* int dsa_in_a_comment(float x); */
        #define DSA_A 0x10   // int dsa_also_a_comment(float x);
        #define DSA_B (DSA_A + 2 * 3)
        #define DSA_F(n) ((n) << 1)
        typedef enum { DSA_P = -1, DSA_Q, DSA_R = 7, DSA_S } dsa_status;
        const char * dsa_name(void);
        int64_t dsa_two_lines(const void* x, int64_t n,
                              double eps, float* out_host, void* stream);
    """)
    assert const == {"DSA_A": 16, "DSA_B": 22, "DSA_P": -1, "DSA_Q": 0, "DSA_R": 7, "DSA_S": 8}
    assert sig == {"dsa_name": (ctypes.c_char_p, []),
                   "dsa_two_lines": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p])}
    for bad in ("int dsa_x(const void* a, float b);",                     # a parameter type without a mapping
                "int dsa_x(const void* a, int32_t n\nint dsa_y(void);",   # unterminated
                "int dsa_x(const void* a, int32_t n",                     # unterminated at the end of the file
                "dsa_x(int32_t n);",                                      # no return type
                "unsigned dsa_x(int32_t n);",                             # a return type without a mapping
                "int dsa_x(int32_t);",                                    # a parameter without a name
                "int dsa_x(int32_t n, void (*done)(int));"):              # nested parentheses
        with pytest.raises(_lib.BackendError, match="diffsptk_amd.h"):
            _lib.parse_header("#define DSA_A 1\nint dsa_ok(void);\n" + bad)
    # a tree without the header fails at import, naming the path
    import importlib.util

    os.makedirs(tmp_path / "pkg")
    (tmp_path / "pkg" / "_lib.py").write_text(open(_lib.__file__).read())
    spec = importlib.util.spec_from_file_location("_lib_without_header", str(tmp_path / "pkg" / "_lib.py"))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "include" / "diffsptk_amd.h"))) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "BackendError"


def test_names_the_driver_uses_resolve():
    """bench.py and __graft_entry__.py reach into ops and _lib by name (ops._call, ops.McepFn, _lib.ALGO_AUTO, ...): every such
    name must resolve, wherever the code behind it lives."""
    from diffsptk_amd import ops

    used = set()
    for f in ("bench.py", "__graft_entry__.py"):
        used |= set(re.findall(r"\b(ops|_lib)\.([A-Za-z_]\w*)", open(os.path.join(ROOT, f)).read()))
    assert {("ops", "_call"), ("ops", "_stream"), ("ops", "McepFn"), ("_lib", "F32"), ("_lib", "last_kernel")} <= used
    missing = [f"{m}.{n}" for m, n in sorted(used) if not hasattr({"ops": ops, "_lib": _lib}[m], n)]
    assert not missing, missing
    assert ops._reserved_cus is ops.mcep._reserved_cus and ops._overlapped is ops.mcep._overlapped   # the lists, not copies


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsp.STFT(400, 80, 512)(torch.zeros(800))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.lpc(torch.zeros(2, 400), 24)


def test_window_tables_match_reference(golden):
    g = golden("tables")
    for w in list(range(7)) + ["povey", "sine", "vorbis", "kbd"]:
        for norm in (0, 1, 2):
            for sym in (True, False):
                if w == "kbd" and not sym:
                    continue
                for L in (8, 10, 400):
                    np.testing.assert_allclose(tables.window_table(L, w, norm, sym),
                                               g[f"win_{w}_{norm}_{int(sym)}_{L}"], rtol=1e-10, atol=1e-13)
    m = dsp.Window(400, 512)
    # the reference builds this table IN float32 (window.py:138): agree to float32 rounding of cos()
    np.testing.assert_allclose(m.window.numpy(), g["blackman400_power_f32"], rtol=1e-5, atol=1e-8)
    assert m.state_dict() == {}  # buffers are non-persistent like the reference's (base.py:67)
    assert isinstance(dsp.Window(8, learnable=True).window, torch.nn.Parameter)


def test_warp_and_composed_matrices(golden):
    g = golden("tables")
    G, D, E, av, Af, Ai, Ar = tables.mcep_matrices(512, 24, 0.42)
    for got, key in ((Af, "freqt_A"), (Ai, "ifreqt_A"), (Ar, "rfreqt_A"), (av, "alpha_vector")):
        np.testing.assert_allclose(got, g[key], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(tables.freqt_matrix(19, 29, 0.1), g["freqt_19_29_0.1"], rtol=1e-12)
    # the composed maps reproduce the reference's FFT chains (numpy evaluation of mcep.py:203-215)
    X = golden("datawav")["stft_power_f64"][::40]
    logx = np.log(X)
    c = np.fft.irfft(logx)
    c[:, 0] *= 0.5
    c[:, 256] *= 0.5
    mc0 = c[:, :257] @ Af
    np.testing.assert_allclose(logx @ G, mc0, rtol=1e-10, atol=1e-12)
    d = np.fft.rfft(mc0 @ Ai, n=512).real
    np.testing.assert_allclose(mc0 @ D, d, rtol=1e-10, atol=1e-12)
    e = np.exp(logx - 2 * d)
    np.testing.assert_allclose(e @ E, np.fft.irfft(e)[:, :257] @ Ar, rtol=1e-10, atol=1e-12)
    mod = dsp.MelCepstralAnalysis(fft_length=512, cep_order=24, alpha=0.42, n_iter=10)
    assert mod.G.shape == (257, 25) and mod.D.shape == (25, 257) and mod.E.shape == (257, 49)
    assert mod.state_dict() == {}


@pytest.mark.parametrize("call,msg", [
    (lambda: dsp.Frame(0, 1), "frame_length must be positive."),
    (lambda: dsp.Frame(1, 0), "frame_period must be positive."),
    (lambda: dsp.Window(0), "in_length must be positive."),
    (lambda: dsp.Window(4, 0), "out_length must be positive."),
    (lambda: dsp.Window(4, window="nope"), "window nope is not supported."),
    (lambda: dsp.Window(4, norm=7), "norm 7 is not supported."),
    (lambda: dsp.RealValuedFastFourierTransform(7), "fft_length must be positive even."),
    (lambda: dsp.RealValuedFastFourierTransform(8, out_format="x"), "out_format x is not supported."),
    (lambda: dsp.Spectrum(1), "fft_length must be greater than 1."),
    (lambda: dsp.Spectrum(8, eps=-1), "eps must be non-negative."),
    (lambda: dsp.Spectrum(8, relative_floor=1), "relative_floor must be negative."),
    (lambda: dsp.STFT(4, 2, 8, learnable=["x"]), "An unsupported key is found in learnable."),
    (lambda: dsp.STFT(4, 2, 8, learnable=1), "learnable must be boolean or list."),
    (lambda: dsp.FrequencyTransform(-1, 2), "in_order must be non-negative."),
    (lambda: dsp.FrequencyTransform(1, -2), "out_order must be non-negative."),
    (lambda: dsp.FrequencyTransform(1, 2, 1.0), "alpha must be in (-1, 1)."),
    (lambda: dsp.MelCepstralAnalysis(fft_length=1, cep_order=0), "fft_length must be greater than 1."),
    (lambda: dsp.MelCepstralAnalysis(fft_length=8, cep_order=-1), "cep_order must be non-negative."),
    (lambda: dsp.MelCepstralAnalysis(fft_length=8, cep_order=5), "cep_order must be less than or equal to fft_length // 2."),
    (lambda: dsp.MelCepstralAnalysis(fft_length=8, cep_order=2, alpha=-1), "alpha must be in (-1, 1)."),
    (lambda: dsp.MelCepstralAnalysis(fft_length=8, cep_order=2, n_iter=-1), "n_iter must be non-negative."),
    (lambda: dsp.Autocorrelation(0, 0), "frame_length must be positive."),
    (lambda: dsp.Autocorrelation(4, 4), "acr_order must be less than frame_length."),
    (lambda: dsp.Autocorrelation(4, 2, "x"), "out_format x is not supported."),
    (lambda: dsp.LevinsonDurbin(-1), "lpc_order must be non-negative."),
    (lambda: dsp.LevinsonDurbin(2, eps=-1.0), "eps must be non-negative."),
])
def test_validation_messages_match_reference(call, msg):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == msg


def test_forward_size_checks():
    with pytest.raises(ValueError, match=r"Unexpected input length \(input 5 vs target 4\)\."):
        dsp.Window(4)(torch.zeros(5))
    with pytest.raises(ValueError, match=r"Unexpected dimension of spectrum \(input 4 vs target 5\)\."):
        dsp.MelCepstralAnalysis(fft_length=8, cep_order=2)(torch.zeros(4))
    with pytest.raises(ValueError, match=r"Unexpected dimension of cepstrum"):
        dsp.FrequencyTransform(3, 4)(torch.zeros(3))
    with pytest.raises(ValueError, match=r"Unexpected length of waveform"):
        dsp.Autocorrelation(5, 2)(torch.zeros(4))
    with pytest.raises(ValueError, match=r"Unexpected dimension of autocorrelation"):
        dsp.LevinsonDurbin(2)(torch.zeros(4))


def test_interface_contract():
    """Same contract the reference pins by AST (tests/test_interface_consistency.py:153-207):
    every functional delegates to Module._func, and every keyword-only name of _forward is
    produced by _precompute."""
    mods = [dsp.Frame, dsp.Window, dsp.RealValuedFastFourierTransform, dsp.Spectrum, dsp.STFT,
            dsp.FrequencyTransform, dsp.MelCepstralAnalysis, dsp.Autocorrelation, dsp.LevinsonDurbin, dsp.LPC]
    samples = {
        dsp.Frame: dict(frame_length=4, frame_period=2),
        dsp.Window: dict(in_length=4, out_length=8),
        dsp.RealValuedFastFourierTransform: dict(fft_length=8),
        dsp.Spectrum: dict(fft_length=8),
        dsp.STFT: dict(frame_length=4, frame_period=2, fft_length=8),
        dsp.FrequencyTransform: dict(in_order=3, out_order=4, alpha=0.1),
        dsp.MelCepstralAnalysis: dict(fft_length=8, cep_order=2, alpha=0.1, n_iter=1),
        dsp.Autocorrelation: dict(frame_length=5, acr_order=2),
        dsp.LevinsonDurbin: dict(lpc_order=2),
        dsp.LPC: dict(frame_length=5, lpc_order=2),
    }
    for M in mods:
        for name in ("_func", "_check", "_precompute", "_forward"):
            assert isinstance(inspect.getattr_static(M, name), staticmethod), (M, name)
        m = M(**samples[M])
        sig = inspect.signature(M._forward)
        need = {k for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY and p.default is p.empty}
        assert need <= set(m._state()), (M, need - set(m._state()))
    for fn in (F.acorr, F.fftr, F.frame, F.freqt, F.levdur, F.lpc, F.mcep, F.spec, F.stft, F.window):
        assert "._func(" in inspect.getsource(fn)
    assert dsp.STFT is dsp.ShortTimeFourierTransform and dsp.LPC is dsp.LinearPredictiveCodingAnalysis


def test_get_alpha_and_read(golden, tmp_path):
    assert dsp.get_alpha(16000) == 0.42 and dsp.get_alpha(48000) == 0.55
    assert dsp.get_alpha(16000, "auto") == pytest.approx(0.41) and dsp.get_alpha(8000, "auto") == pytest.approx(0.31)
    with pytest.raises(ValueError):
        dsp.get_alpha(12345)
    import wave

    pcm = golden("datawav")["pcm"]
    p = str(tmp_path / "d.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.astype("<i2").tobytes())
    x, sr = dsp.read(p)
    assert sr == 16000 and x.shape == (19200,) and x.dtype == torch.float32
    np.testing.assert_array_equal(x.numpy(), (pcm / 32768.0).astype(np.float32))


def test_mcep_module_routes_extreme_alpha_to_generic():
    """The tuned mel-cepstral kernels scale their binary16 operand images for |alpha| <= 0.95."""
    import torch

    from diffsptk_amd import _lib
    from diffsptk_amd.modules.mcep import MelCepstralAnalysis

    for alpha, algo in ((0.42, _lib.ALGO_AUTO), (-0.95, _lib.ALGO_AUTO), (0.96, _lib.ALGO_GENERIC), (-0.99, _lib.ALGO_GENERIC)):
        pre = MelCepstralAnalysis._precompute(512, 24, alpha, 3, "cpu", torch.float32)
        assert pre.values["algo"] == algo


def test_fbank_mfcc_module_contract():
    """Constructor checks of the filter-bank / MFCC modules (fbank.py:170-196, mfcc.py:162-168)."""
    import pytest

    import diffsptk_amd as dsp

    ok = dict(fft_length=512, n_channel=40, sample_rate=16000)
    bad = [(dict(ok, fft_length=1), "fft_length must be greater than 1."), (dict(ok, n_channel=0), "n_channel must be positive."),
           (dict(ok, sample_rate=0), "sample_rate must be positive."), (dict(ok, f_min=8000), "Invalid f_min."),
           (dict(ok, f_max=9000), "Invalid f_min and f_max."), (dict(ok, floor=0), "floor must be positive."),
           (dict(ok, gamma=1.5), "gamma must be in [-1, 1]."), (dict(ok, erb_factor=0), "erb_factor must be positive."),
           (dict(ok, out_format="z"), "out_format z is not supported.")]
    for kw, msg in bad:
        import re

        with pytest.raises(ValueError, match=re.escape(msg)):
            dsp.MelFilterBankAnalysis(**kw)
    m = dsp.MelFilterBankAnalysis(**ok)
    assert m.H.shape == (257, 40) and list(m.state_dict()) == []
    with pytest.raises(ValueError, match="mfcc_order must be less than n_channel."):
        dsp.MFCC(fft_length=512, mfcc_order=40, n_channel=40, sample_rate=16000)
    with pytest.raises(ValueError, match="lifter must be non-negative."):
        dsp.MFCC(fft_length=512, mfcc_order=12, n_channel=40, sample_rate=16000, lifter=-1)
    mf = dsp.MFCC(fft_length=512, mfcc_order=12, n_channel=40, sample_rate=16000, lifter=22)
    assert mf.W.shape == (40, 13) and mf.H.shape == (257, 40)
    with pytest.raises(ValueError, match="dct_type must be in"):
        dsp.DCT(8, 5)


def test_griffin_lim_module_contract():
    """Constructor checks of GriffinLim (griffin.py:150-163, 188-193) and the no-CPU-fallback rule."""
    import re

    import pytest
    import torch

    import diffsptk_amd as dsp

    for kw, msg in ((dict(n_iter=-1), "n_iter must be non-negative."), (dict(alpha=-1), "alpha must be non-negative."),
                    (dict(beta=-0.1), "beta must be non-negative."), (dict(gamma=-2), "gamma must be non-negative."),
                    (dict(init_phase="ones"), "init_phase: ones is not supported.")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            dsp.GriffinLim(400, 80, 512, **kw)
    m = dsp.GriffinLim(400, 80, 512, n_iter=3, init_phase="zeros")
    assert list(m.state_dict()) == [] and m.n_iter == 3 and isinstance(m.istft, dsp.ISTFT) and isinstance(m.stft, dsp.STFT)
    with pytest.raises(RuntimeError, match="device"):
        m(torch.rand(5, 257))     # host tensor: there is no CPU path


def test_fftcep_module_contract():
    """Constructor checks of CepstralAnalysis (fftcep.py:95-106)."""
    import re

    import pytest

    import diffsptk_amd as dsp

    ok = dict(fft_length=512, cep_order=24)
    for kw, msg in ((dict(ok, fft_length=1), "fft_length must be greater than 1."), (dict(ok, cep_order=-1), "cep_order must be non-negative."),
                    (dict(ok, cep_order=257), "cep_order must be less than or equal to fft_length // 2."),
                    (dict(ok, accel=-1), "accel must be non-negative."), (dict(ok, n_iter=-1), "n_iter must be non-negative.")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            dsp.CepstralAnalysis(**kw)
    m = dsp.CepstralAnalysis(**ok, n_iter=2)
    assert m.A.shape == (257, 257) and list(m.state_dict()) == [] and m.in_dim == 257


def test_build_recipe_is_consistent():
    """Every per-source flag set names a source of the build, every source exists, every csrc/*.hip file is a source of the
    build (no orphaned unit), and the library on disk exports the entry points the header declares (the loader checks each
    signature on load)."""
    import os

    from diffsptk_amd import _lib

    assert set(_lib.SOURCE_FLAGS) <= set(_lib.SOURCES)
    assert len(set(_lib.SOURCES)) == len(_lib.SOURCES)
    files, deps = _lib._sources()
    assert all(os.path.exists(f) for f in files + deps)
    on_disk = {f for f in os.listdir(_lib.CSRC) if f.endswith(".hip")}
    assert on_disk == set(_lib.SOURCES), sorted(on_disk ^ set(_lib.SOURCES))
    lib = _lib.load()
    for name in _lib.SIGNATURES:
        assert hasattr(lib, name), name


def test_every_csrc_header_compiles_alone():
    """Every csrc/*.h is a header, not a fragment: it includes what it uses, so it passes the compiler's syntax check as a
    translation unit of its own (host and gfx950 device pass; nothing is written)."""
    import shutil
    import subprocess
    from concurrent.futures import ThreadPoolExecutor

    from diffsptk_amd import _lib

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    headers = sorted(h for h in os.listdir(_lib.CSRC) if h.endswith(".h"))
    assert len(headers) >= 20

    def check(h):
        return subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wno-pragma-once-outside-header",
                               "-x", "hip", os.path.join(_lib.CSRC, h)], capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        results = list(pool.map(check, headers))
    failed = {h: (r.stdout + r.stderr)[-600:] for h, r in zip(headers, results) if r.returncode != 0}
    assert not failed, failed


def test_shared_device_helpers_are_not_copied():
    """The builtins that the shared device helpers of csrc/common.h wrap -- wave_readlane, rn_mul / rn_add / rn_sub / rn_div,
    fft_brev -- appear in no other file of csrc/ (read as text): a unit that needs one calls the helper and does not bring a
    copy under a prefix of its own.  The same for the host helpers: the dynamic-LDS attribute and its per-device record belong to
    launch_lds, the dtype refusal to with_dtype.  The exceptions are listed by file and pattern, each with its reason."""
    from diffsptk_amd import _lib

    primitives = {
        "readlane": r"\b__builtin_amdgcn_readlane\b",
        "rn": r"\b__[fd](?:mul|add|sub|div)_rn\b",
        "brev": r"\b__brev\b",
        "lds_attribute": r"\bhipFuncAttributeMaxDynamicSharedMemorySize\b",
        "lds_record": r"\bensure_dynamic_lds\(",
        "dtype_refusal": r': unsupported dtype(?:%s)?"',
    }
    allowed = {
        # the one read of the wave's maximum inside the tuned lpc24 kernels, spelled as it was when they were tuned
        ("lpc24.h", "readlane"),
        # the pivot key's read in th_solve_reg: through wave_readlane the code of 25 kernels that inline it changes (two of them tuned)
        ("th_solve_reg.h", "readlane"),
        # pg_lane(double): with wave_readlane's spelling the compiler schedules mlpg_sweep_kernel<double, 0> differently
        ("paramgen.hip", "readlane"),
        # mcep_generic_fwd / _bwd: a size that grows with the call, set again on every launch above 48 KB -- launch_lds reserves one
        # size once per device, which a later, larger call would not raise
        ("mcep.hip", "lds_attribute"),
    }
    files = sorted(f for f in os.listdir(_lib.CSRC) if f.endswith((".hip", ".h")))
    assert len(files) >= 55 and "common.h" in files
    found = set()
    for f in files:
        text = open(os.path.join(_lib.CSRC, f)).read()
        found |= {(f, name) for name, pattern in primitives.items() if re.search(pattern, text)}
    assert {name for f, name in found if f == "common.h"} == set(primitives)   # the patterns see the shared definitions
    assert {(f, name) for f, name in found if f != "common.h"} == allowed


def test_no_crossed_packed_float32():
    """The mechanical form of DESIGN.md 4's invariant: NO kernel of the built library contains a packed float32 instruction
    with a set op_sel bit (a low result half reading a high source half) -- the instruction class of every transient wrong
    result recorded there.  No allow-list: a kernel that "runs alone" can meet another instruction stream on its SIMD through
    a second HIP stream.  The gfx950 code objects of the library on disk are disassembled (llvm-objdump, a private copy)."""
    import sys

    from diffsptk_amd import _lib

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import isa_mix
    finally:
        sys.path.pop(0)
    if not os.path.exists(isa_mix.OBJDUMP):
        pytest.skip("llvm-objdump not found")
    kernels = isa_mix.disassemble(_lib.build())
    assert len(kernels) > 200   # the whole library was read, not one code object
    n_packed = sum(1 for ins in kernels.values() for _, op, _t in ins if re.match(r"v_pk_\w+_f32", op))
    assert n_packed > 1000      # ... and the pattern below sees packed instructions at all
    bad = isa_mix.crossed_packed_f32(kernels)
    assert not bad, {k: (len(v), v[:2]) for k, v in bad.items()}
    # the detector itself: the two forms round 5's audit missed in mgcep_step_h_kernel, and forms that are fine
    fake = {"k": [(0, "v_pk_mul_f32", "v[4:5], v[34:35], v[36:37] op_sel:[0,1] op_sel_hi:[1,0]"),
                  (4, "v_pk_fma_f32", "v[0:1], v[2:3], v[4:5], v[0:1] op_sel_hi:[1,0,1]"),
                  (8, "v_pk_add_f32", "v[0:1], v[2:3], v[4:5] neg_lo:[0,1] neg_hi:[0,1]"),
                  (12, "v_pk_fma_f32", "v[0:1], v[2:3], v[4:5], v[0:1] op_sel:[0,1,0] op_sel_hi:[1,1,1]"),
                  (16, "v_pk_mul_f16", "v0, v1, v2 op_sel:[1,0]")]}
    assert [t.split()[0] for t in isa_mix.crossed_packed_f32(fake)["k"]] == ["v_pk_mul_f32", "v_pk_fma_f32"]


def test_learnable_fallback_operators_match_the_transforms():
    """modules/_learnable.py (the torch-operator fallbacks behind ``learnable=``) against numpy / the oracle: at
    initialisation a learnable basis must reproduce the fixed transform it replaces (fftr.py:123-129,
    ifftr.py:125-129, unframe.py:164-211, fbank.py:306-321)."""
    from diffsptk_amd.modules import _learnable as Lr
    from oracle import oracle as O

    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 20))
    W = torch.from_numpy(Lr.dft_matrix(32))
    Y = np.fft.rfft(x, n=32)
    for fmt, ref in ((0, Y), (1, Y.real), (2, Y.imag), (3, np.abs(Y)), (4, np.abs(Y) ** 2)):
        np.testing.assert_allclose(Lr.rfft_with_basis(torch.from_numpy(x), W, 32, fmt).numpy(), ref, rtol=1e-12, atol=1e-12)
    Wi = torch.from_numpy(Lr.idft_matrix(32, 20))
    np.testing.assert_allclose(Lr.irfft_with_basis(torch.from_numpy(Y), Wi).numpy(), np.fft.irfft(Y, n=32)[:, :20], atol=1e-13)
    b, a = rng.standard_normal((4, 3)), np.abs(rng.standard_normal((4, 4))) + 1.5
    s = Lr.spectrum_with_basis(torch.from_numpy(b), torch.from_numpy(a), W, 32, 1e-6, -30.0, 0).numpy()
    np.testing.assert_allclose(s, O.spec(b, a, fft_length=32, eps=1e-6, relative_floor=-30.0, out_format="db"), rtol=1e-10, atol=1e-10)
    fr = rng.standard_normal((2, 9, 12))
    w = O.window_table(12, "hanning", "none") + 0.1
    for center, out_length in ((True, None), (False, None), (True, 30)):
        got = Lr.unframe_with_window(torch.from_numpy(fr), torch.from_numpy(w), 4, center, out_length).numpy()
        np.testing.assert_allclose(got, O.unframe(fr, 4, center=center, w=w, out_length=out_length), rtol=1e-12, atol=1e-12)
    X = np.abs(rng.standard_normal((6, 17))) + 0.1
    H = O.fbank_matrix(32, 8, 8000)
    y, E = Lr.fbank_with_weights(torch.from_numpy(X), torch.from_numpy(H), 1e-5, 0.0, False)
    yo = O.fbank(X, H, 1e-5, 0.0, False)
    np.testing.assert_allclose(y.numpy(), yo[0] if isinstance(yo, tuple) else yo, rtol=1e-12)
    # the learnable options register Parameters, the fixed ones keep the state_dict empty (base.py:64-67)
    m = dsp.RealValuedFastFourierTransform(32, learnable=True)
    assert [n for n, _ in m.named_parameters()] == ["W"] and m.W.shape == (32, 34)
    assert [n for n, _ in dsp.STFT(12, 4, 16, learnable=True).named_parameters()] == ["window", "W"]
    assert [n for n, _ in dsp.ISTFT(12, 4, 16, learnable=["basis"]).named_parameters()] == ["W"]
    assert [n for n, _ in dsp.MelFilterBankAnalysis(fft_length=32, n_channel=8, sample_rate=8000, learnable=True).named_parameters()] == ["H"]
    assert len(dsp.STFT(12, 4, 16).state_dict()) == 0


def test_fbank_scan_plan_c_and_python_agree_and_the_lane_model_matches_the_matrix():
    """The per-lane plan of the fused STFT -> filter-bank kernel (dsa_fbank_scan_plan, host code of the library) equals
    its Python statement bit for bit, a lane-level numpy execution of the plan (DPP semantics of the scan network,
    tools/proto_fbank_scan.py) reproduces s @ H, and matrices without the triangular structure are refused."""
    import importlib.util

    from diffsptk_amd.utils import tables

    spec = importlib.util.spec_from_file_location(
        "proto_fbank_scan", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto_fbank_scan.py"))
    proto = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(proto)
    lib = _lib.load()
    rng = np.random.default_rng(1)
    for C, sr, fmin, fmax in ((40, 16000, 0, None), (80, 16000, 0, None), (24, 16000, 64, 7600), (126, 48000, 0, None), (1, 8000, 0, None)):
        H = np.ascontiguousarray(tables.fbank_matrix(512, C, sr, fmin, fmax, "htk", None), dtype=np.float64)
        table = np.zeros(_lib.FBANK_PLAN_FLOATS, dtype=np.float32)
        assert lib.dsa_fbank_scan_plan(H.ctypes.data, 257, C, table.ctypes.data) == 0
        plan = tables.fbank_scan_plan(H)
        assert np.array_equal(table.view(np.int32), tables.fbank_scan_table(plan).reshape(-1).view(np.int32))
        P = (rng.standard_normal(257) ** 2 * 10.0 ** rng.uniform(-6, 6, 257)).astype(np.float32)
        y, ref = proto.wave_epilogue(P, plan, C), P.astype(np.float64) @ H
        assert np.max(np.abs(y - ref) / np.maximum(np.abs(ref), 1e-300)) < 2e-6
    table = np.zeros(_lib.FBANK_PLAN_FLOATS, dtype=np.float32)
    for bad in (np.abs(rng.standard_normal((257, 40))), np.asarray(tables.fbank_matrix(512, 40, 16000, 0, None, "htk", 1.0)),
                np.asarray(tables.fbank_matrix(512, 40, 16000, 0, None, "htk", None))[:, ::-1]):
        Hb = np.ascontiguousarray(bad, dtype=np.float64)
        assert lib.dsa_fbank_scan_plan(Hb.ctypes.data, 257, 40, table.ctypes.data) == _lib.ERR_UNSUPPORTED
        assert tables.fbank_scan_plan(Hb) is None
    H127 = np.zeros((257, 127))
    assert lib.dsa_fbank_scan_plan(H127.ctypes.data, 257, 127, table.ctypes.data) == _lib.ERR_UNSUPPORTED


def test_fbank_bins_table_c_and_python_agree_and_reproduce_the_matrix():
    """The per-bin table of the fused filter bank's backward (dsa_fbank_bins_plan, host code of the library) equals its
    Python twin bit for bit, and spreading channel values through it IS the product with H^T."""
    lib = _lib.load()
    rng = np.random.default_rng(2)
    for C, sr in ((40, 16000), (80, 22050), (3, 8000), (126, 48000)):
        H = np.ascontiguousarray(np.asarray(tables.fbank_matrix(512, C, sr, 0.0, None, "htk", None), dtype=np.float64))
        t = np.zeros(4 * 257, dtype=np.float32)
        assert lib.dsa_fbank_bins_plan(H.ctypes.data, 257, C, t.ctypes.data) == 0
        tp = tables.fbank_bins_table(H)
        assert np.array_equal(t.view(np.uint32), tp.reshape(-1).view(np.uint32))
        c0 = tp[:, 0].copy().view(np.int32)
        c1 = np.minimum(c0 + 1, C - 1)
        q = rng.standard_normal((5, C))
        g = tp[:, 1] * q[:, c0] + tp[:, 2] * q[:, c1]
        np.testing.assert_allclose(g, q @ H.astype(np.float32).astype(np.float64).T, rtol=1e-12, atol=1e-12)
    Hb = rng.random((257, 5))   # dense rows: not a two-channels-per-bin matrix
    t = np.zeros(4 * 257, dtype=np.float32)
    assert lib.dsa_fbank_bins_plan(np.ascontiguousarray(Hb).ctypes.data, 257, 5, t.ctypes.data) == _lib.ERR_UNSUPPORTED
    assert tables.fbank_bins_table(Hb) is None


def test_round3_host_tables_and_dispatch_rules():
    """Host-side pieces added in round 3 (no GPU): the folded cepstrum -> spectrum matrices against the two-step numpy
    computation they replace, the backward operand images of the mgcep step against the matrices they are cut from, and the
    shape rules that route row products / Taylor stages / the composed analysis."""
    import torch

    from diffsptk_amd import ops
    from diffsptk_amd.utils import tables

    # mgc2sp: frequency transform to order L/2, then Re / Im of the L-point transform == one matrix each
    rng = np.random.default_rng(0)
    for M, L, alpha in ((24, 512, -0.42), (8, 32, -0.1), (30, 64, 0.0)):
        W_re, W_im = tables.cepstrum_to_spectrum_matrices(M, L, alpha)
        c = rng.standard_normal((5, M + 1))
        A = tables.freqt_matrix(M, L // 2, alpha) if alpha != 0 else np.eye(M + 1, L // 2 + 1)
        C = np.fft.rfft(c @ A, n=L)
        np.testing.assert_allclose(c @ W_re, C.real, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(c @ W_im, C.imag, rtol=1e-10, atol=1e-12)
    # mgcep step, backward images: tile 3, the transposed Pr block (k-step 2) and the Cr block (t = 1, r = 2)
    M, alpha = 24, 0.42
    m = tables.mgcep_matrices(512, M, alpha)
    img = tables.mgcep_step_bwd_images(512, M, alpha).astype(np.float64)
    assert img.shape == (17, 768 + 44 * 64 + 16 * 64)
    np.testing.assert_array_equal(img[:, :768], tables.mgcep_step_images(512, M, alpha)[:, :768].astype(np.float64))
    lanes = np.arange(64)
    li, lg = lanes & 15, lanes >> 4
    a2 = img[3, 768:768 + 44 * 64].reshape(44, 64)
    np.testing.assert_allclose(a2[2], m["Pr"][:, :M][16 * 3 + li, 4 * 2 + lg].astype(np.float32), rtol=0, atol=0)
    a3 = img[3, 768 + 44 * 64:].reshape(2, 2, 4, 64)
    row = 1 + 16 * 1 + li
    want = np.where(row <= M, m["Cr"][np.minimum(row, M), 16 * 3 + 4 * lg + 2], 0.0).astype(np.float32)
    np.testing.assert_allclose(a3[0, 1, 2], want, rtol=0, atol=0)
    # dispatch rules
    # (geometry only: the number of rows is not an argument -- a row's result must not depend on the batch it arrives in)
    assert ops._row_product_is_long(50, 1025, 4) and ops._row_product_is_long(1025, 99, 4)
    assert not ops._row_product_is_long(25, 200, 4)          # fits LDS
    assert not ops._row_product_is_long(200, 25, 4)          # short rows keep the library's kernel
    x, b = torch.zeros(2, 160), torch.zeros(2, 2, 40)
    assert not ops.zerodf_taylor_shapes_ok(x, b, 80)                       # host tensors never take the fused launches
    x32 = torch.zeros(2, 1025)
    assert ops._mcep_composed_applies(x32, 49) and not ops._mcep_composed_applies(x32, 64)
    assert ops._mcep_composed_applies(x32[:1], 49)                           # one frame or 12 800: the same path
    assert not ops._mcep_composed_applies(torch.zeros(2, 17), 8)             # short spectra (the reference's test grids): generic pair
    assert not ops._mcep_composed_applies(x32.double(), 49)                  # float64 keeps the generic kernel pair


def test_mlsa_learnable_constructs_on_the_host():
    """learnable=True of the multi-stage MLSA filter: a Parameter of taylor_order + 1 ones (mglsadf.py:344-349); the other
    arguments are checked as in the reference."""
    import torch

    import diffsptk_amd as dsp

    m = dsp.MLSA(24, 80, alpha=0.42, mode="multi-stage", taylor_order=7, learnable=True)
    assert isinstance(m.a, torch.nn.Parameter) and m.a.shape == (8,) and bool((m.a == 1).all())
    assert dsp.MLSA(24, 80, alpha=0.42, mode="multi-stage").a is None
    with pytest.raises(ValueError):
        dsp.MLSA(24, 80, mode="multi-stage", taylor_order=-1)


def test_round5_binary16_operand_images_reconstruct_their_matrices():
    """The hi / lo binary16 operand images of the one-launch mgcep step, of its adjoint and the Nyquist tail (utils/tables.py): every
    (lane, k-slot) entry, hi + lo, is the scaled matrix entry the kernel's lane order names -- to 2^-21 of the entry (a 3-term split
    carries 22 bits) -- and everything outside the matrices is zero.  (The 48 kHz residual's images are built on the device.)"""
    from diffsptk_amd.utils import tables

    m = tables.mgcep_matrices(512, 24, 0.42)
    img = tables.mgcep_step_h_images(512, 24, 0.42).astype(np.float64)
    assert img.shape == (9, 16384)
    sc, sw = 2.0 ** tables.MGCEP_STEP_H_LOG2_SC, 2.0 ** tables.MGCEP_STEP_H_LOG2_SW
    lanes = np.arange(64)
    li, lg = lanes & 15, lanes >> 4
    for j in (0, 3, 8):
        c1 = img[j, :4096].reshape(2, 2, 2, 64, 8)
        w2 = img[j, 4096:].reshape(12, 2, 64, 8)
        for t in range(2):
            for ci_, C in enumerate((m["Cr"], m["Ci"])):
                for i in range(8):
                    row, col = 1 + 8 * lg + i, 32 * j + 16 * t + li
                    ok = (row <= 24) & (col < 257)
                    want = np.where(ok, sc * C[np.minimum(row, 24), np.minimum(col, 256)], 0.0)
                    got = c1[t, ci_, 0, :, i] + c1[t, ci_, 1, :, i]
                    assert np.all(np.abs(got - want) <= 2.0 ** -21 * np.abs(want) + 2.0 ** -24)   # (+ the binary16 subnormal quantum)
        mats = [(m["Pr"][:, :24], 2), (m["Qr"][:, 2:], 3), (m["Qi"][:, 2:], 3), (m["Rr"], 2), (m["Ri"], 2)]
        c = 0
        for W, ntile in mats:
            for tc in range(ntile):
                for i in range(8):
                    b, col = 32 * j + 16 * (i >> 2) + 4 * lg + (i & 3), 16 * tc + li
                    ok = (b < 257) & (col < W.shape[1])
                    want = np.where(ok, sw * W[np.minimum(b, 256), np.minimum(col, W.shape[1] - 1)], 0.0)
                    got = w2[c, 0, :, i] + w2[c, 1, :, i]
                    # entries below 2^-14 / 2^11 of the scale keep fewer bits of their low piece (binary16 subnormals): absolute bound
                    assert np.all(np.abs(got - want) <= 2.0 ** -21 * np.abs(want) + 2.0 ** -24)
                c += 1
    buf = tables.mgcep_step_h_buffer(512, 24, 0.42)
    assert buf.dtype == np.uint8 and buf.size == 9 * 16384 * 2 + 240 * 4
    tail = buf[9 * 16384 * 2:].view(np.float32)
    assert np.array_equal(tail[0:24], m["Cr"][1:25, 256].astype(np.float32)) and np.array_equal(tail[24:48], m["Ci"][1:25, 256].astype(np.float32))
    assert np.array_equal(tail[48:72], m["Pr"][256, :24].astype(np.float32)) and not tail[72:80].any()
    assert np.array_equal(tail[80:127], m["Qr"][256, 2:].astype(np.float32)) and np.array_equal(tail[208:233], m["Ri"][256].astype(np.float32))
    bw = tables.mgcep_step_bwd_h_images(512, 24, 0.42).astype(np.float64)
    assert bw.shape == (9, 22528)
    assert np.array_equal(bw[:, :4096], img[:, :4096])                      # the forward's first chain, verbatim
    ct = bw[2, 4096 + 14336:].reshape(2, 2, 2, 64, 8)                       # (Cr, Ci) with coefficients as rows
    for ci_, C in enumerate((m["Cr"], m["Ci"])):
        for tc in range(2):
            for i in range(8):
                b, row = 32 * 2 + 16 * (i >> 2) + 4 * lg + (i & 3), 1 + 16 * tc + li
                ok = row <= 24
                want = np.where(ok, sc * C[np.minimum(row, 24), b], 0.0)
                got = ct[ci_, tc, 0, :, i] + ct[ci_, tc, 1, :, i]
                assert np.all(np.abs(got - want) <= 2.0 ** -21 * np.abs(want) + 2.0 ** -24)


def test_state_dict_keys_and_shapes_are_the_references():
    """Checkpoints interchange with the reference (same names): for every module of the path, learnable or not, ``state_dict()``
    has the reference's keys and shapes (tests/golden/state_keys.json, generated by importing the reference:
    tests/golden/make_golden_state_keys.py) -- the composite modules keep their learnable tensors on the module itself here (one
    fused launch) and translate (`BaseFunctionalModule._reference_state_keys`) -- a state dict with the reference's keys loads, and the
    values come back unchanged; the local names are still accepted."""
    import json

    import diffsptk_amd as dsp

    cases = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_keys.json")))
    assert len(cases) >= 39
    n_learnable = 0
    for c in cases:
        args = [tuple(v) if isinstance(v, list) else v for v in c["args"]]
        m = getattr(dsp, c["module"])(*args, **c["kwargs"])
        sd = m.state_dict()
        assert {k: list(v.shape) for k, v in sd.items()} == c["state"], (c["module"], c["kwargs"])
        if not sd:
            continue
        n_learnable += 1
        ref_like = {k: torch.randn(*shape, dtype=sd[k].dtype) for k, shape in c["state"].items()}
        m.load_state_dict(ref_like)                       # strict: no missing / unexpected keys
        back = m.state_dict()
        for k, v in ref_like.items():
            assert torch.equal(back[k], v), (c["module"], k)
        local = {k: torch.randn_like(v) for k, v in m.named_parameters()}
        m.load_state_dict(local)                          # the module's own parameter names still load
        for k, v in m.named_parameters():
            assert torch.equal(v, local[k]), (c["module"], k)
    assert n_learnable >= 15


def test_modules_deepcopy_and_pickle():
    """copy.deepcopy (EMA copies) and pickle (torch.save(model)) of the path's modules: the reference's composite modules are
    deep-copyable and, where they hold no lambda, picklable; here every module is both -- the state-dict translation hooks are
    module-level functions -- and a copy keeps the reference's state-dict keys with parameters of its own."""
    import copy
    import pickle

    import diffsptk_amd as dsp

    for name, args, kw in (("STFT", (400, 80, 512), {"learnable": True}), ("ISTFT", (400, 80, 512), {"learnable": True}),
                           ("MelCepstralAnalysis", (), {"fft_length": 512, "cep_order": 24, "alpha": 0.42}),
                           ("LPC", (400, 24), {}), ("MFCC", (), {"fft_length": 512, "mfcc_order": 12, "n_channel": 40, "sample_rate": 16000, "learnable": True}),
                           ("PseudoMGLSADigitalFilter", (24, 80), {"alpha": 0.42, "learnable": True}),
                           ("MelGeneralizedCepstralAnalysis", (), {"fft_length": 512, "cep_order": 24, "alpha": 0.42, "gamma": -0.5})):
        m = getattr(dsp, name)(*args, **kw)
        for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
            assert list(c.state_dict()) == list(m.state_dict()), name
            for (k, p), (_k2, q) in zip(m.named_parameters(), c.named_parameters()):
                assert torch.equal(p, q) and p.data_ptr() != q.data_ptr(), (name, k)
            c.load_state_dict(m.state_dict())


def test_read_write_wav_round_trip(tmp_path):
    """diffsptk.read / diffsptk.write (public.py:107-198) on the standard library's wave module: 16-bit PCM scaled by 1 / 32768 on the
    way in and by 32767 (nearest-even, as libsndfile does for normalised floats) on the way out; (T,), (C, T), (T, C); the
    sample-selecting keyword arguments of soundfile.read."""
    import numpy as np

    import diffsptk_amd as dsp

    pcm = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datawav.npz"))["pcm"]
    x = torch.from_numpy(pcm.astype(np.float64) / 32768.0)
    p = str(tmp_path / "a.wav")
    dsp.write(p, x, 16000)
    y, sr = dsp.read(p, dtype=torch.float64)
    assert sr == 16000 and y.shape == x.shape
    want = torch.from_numpy(np.clip(np.rint(x.numpy() * 32767.0), -32768, 32767) / 32768.0)
    assert torch.equal(y, want)
    assert dsp.read(p, start=100, stop=-100)[0].shape == (x.numel() - 200,)
    assert dsp.read(p, frames=50, always_2d=True)[0].shape == (1, 50)
    two = torch.stack([x, -x])
    dsp.write(p, two, 8000)
    z, sr = dsp.read(p, dtype=torch.float64)
    assert sr == 8000 and z.shape == (2, x.numel()) and torch.equal(z[0], want)
    dsp.write(p, two.T, 8000, channel_first=False, subtype="PCM_32")
    z, _ = dsp.read(p, channel_first=False, dtype=torch.float64)
    assert z.shape == (x.numel(), 2) and float((z[:, 0] - x).abs().max()) < 1e-9
    with pytest.raises(TypeError):
        dsp.write(p, x, 16000, endian="BIG")


def test_api_surface_is_the_references():
    """SURVEY 8(b) mechanically: the constructor / forward signatures of the 35 exported classes, the 26 functionals and `read` / `write` /
    `get_alpha` equal the reference's (names, kinds, defaults; this repo may add `device` / `dtype` where the reference has none), and 65
    invalid option sets raise the reference's exception type with the reference's text (tests/golden/api_surface.json, generated by
    importing the reference: tests/golden/make_golden_api_surface.py)."""
    import json

    import diffsptk_amd.functional as OF

    surf = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_surface.json")))

    def sig(f):
        return [[p.name, p.kind.name, None if p.default is inspect._empty else repr(p.default)] for p in inspect.signature(f).parameters.values()]

    def strip(s):
        return [p for p in s if p[0] not in ("device", "dtype")]

    assert len(surf["classes"]) >= 35 and len(surf["functional"]) >= 26 and len(surf["errors"]) >= 65
    for name, want in surf["classes"].items():
        cls = getattr(dsp, name)
        assert strip(sig(cls.__init__)) == strip(want["init"]), (name, "__init__")
        assert strip(sig(cls.forward)) == strip(want["forward"]), (name, "forward")
    for name, want in surf["functions"].items():
        assert sig(getattr(dsp, name)) == want, name
    for name, want in surf["functional"].items():
        assert sig(getattr(OF, name)) == want, ("functional", name)
    for c in surf["errors"]:
        try:
            getattr(dsp, c["module"])(*c["args"], **c["kwargs"])
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        assert got == c["raises"], (c["module"], c["args"], c["kwargs"], got, c["raises"])
