"""Loader / builder of the C-ABI shared library (include/diffsptk_amd.h).

The library is built IN-TREE by hipcc for gfx950 (``build()``; ``__graft_entry__.build()`` calls
it) and loaded with ctypes.  There is no CPU fallback: if the library is missing, or no HIP
device is visible, the ops raise -- they never silently compute elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
CSRC = os.path.join(_PKG, "csrc")
LIB_DIR = os.path.join(_PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libdiffsptk_amd.so")
SOURCES = ("core.hip", "stft.hip", "spec.hip", "griffin.hip", "mcep.hip", "mcep_mfma.hip", "mcep_mfma_bwd.hip", "mgcep_step.hip", "mcep_resid.hip", "mcep_big.hip", "lpc.hip", "lpc24.hip", "lpc24_bwd.hip", "fbank.hip", "fftcep.hip", "mgc.hip", "thsolve.hip",
           "zerodf.hip", "rows_gemm.hip", "thsolve_quad.hip", "poledf.hip", "plp.hip", "pqmf.hip", "parcor.hip", "lsp.hip", "mlsacheck.hip", "excite.hip", "mdct.hip",
           "paramgen.hip", "dtw.hip", "gmm.hip", "yingram.hip", "vq.hip", "world_synth.hip", "ap.hip", "pitch_spec.hip")
HIPCC_FLAGS = (
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
    "-mcode-object-version=5", "-Wno-unused-value", "-ffp-contract=on",
)
# Per-source additions.  stft.hip: the compiler's automatic v_pk_*_f32 selection costs the register-FFT kernels
# more in register-pairing moves than it saves (forward 88 -> 82 us per 204 800 frames without it; the packed
# kernels of stft_pk.h / stft_bwd_pk.h switch the feature back on for themselves and place v_pk_* by hand).
# Round 6: the same for every unit whose compiler-made packed code contained forms with a set op_sel bit (a low result half
# reading a high source half: the instruction class of DESIGN.md 4, which no shipped kernel may execute --
# tests/test_host_cpu.py::test_no_crossed_packed_float32); kernels with hand-placed packed instructions carry DSA_PK_TARGET.
_NO_PK = ("-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops")
SOURCE_FLAGS = {
    "core.hip": _NO_PK,
    "stft.hip": _NO_PK,
    "spec.hip": _NO_PK,
    "griffin.hip": _NO_PK,
    "fbank.hip": _NO_PK,
    "mgc.hip": _NO_PK,
    "thsolve.hip": _NO_PK,
    "zerodf.hip": _NO_PK,
    "thsolve_quad.hip": _NO_PK,
    "poledf.hip": _NO_PK,
    "plp.hip": _NO_PK,
    "pqmf.hip": _NO_PK,
    "parcor.hip": _NO_PK,
    "lsp.hip": _NO_PK,
    "mlsacheck.hip": _NO_PK,
    "excite.hip": _NO_PK,
    "mdct.hip": _NO_PK,
    "paramgen.hip": _NO_PK,
    "dtw.hip": _NO_PK,
    "gmm.hip": _NO_PK,
    "yingram.hip": _NO_PK,
    "vq.hip": _NO_PK,
    "world_synth.hip": _NO_PK,
    "ap.hip": _NO_PK,
    "pitch_spec.hip": _NO_PK,
    # the mel-cepstral units: their kernels carry DSA_PK_TARGET -- measured faster with the compiler's pairing -- except mgcep_step_h
    "mcep_mfma.hip": _NO_PK,
    "mcep_mfma_bwd.hip": _NO_PK,
    "mgcep_step.hip": _NO_PK,
    "mcep_resid.hip": _NO_PK,
    "mcep_big.hip": _NO_PK,
}

_lib = None


class BackendError(RuntimeError):
    """The HIP library is missing, failed to load, or a call returned an error status."""


# bindings and constants: read at import from the C header, which the compiler checks against the definitions in every .hip file
HEADER = os.path.join(_ROOT, "include", "diffsptk_amd.h")
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
_VALUES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
_PROTOTYPE = re.compile(r"\s*([\w\s*]+?)\s*\b(dsa_[a-z0-9_]+)\s*\(([^()]*)\)\s*")


def parse_header(text: str):
    """(signatures, constants) of the header's text: name -> (restype, [argtypes]) of every `dsa_*` prototype, and name -> int of
    every enumerator and object-like `#define DSA_*` (function-like macros are not evaluated).  Raises BackendError on whatever
    looks like a prototype and is not fully understood; a constant that is no integer expression raises from eval() / int()."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    signatures, constants = {}, {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DSA_\w+)[ \t]+(.+)$|\benum\s*\{([^}]*)\}", text, flags=re.M):
        last = -1   # an enumerator without a value is one more than the one before it
        for item in [f"{m.group(1)} = {m.group(2)}"] if m.group(1) else filter(str.strip, m.group(3).split(",")):
            name, _, expr = map(str.strip, item.partition("="))
            constants[name] = last = int(eval(expr or str(last + 1), {"__builtins__": {}}, constants))   # may name earlier ones
    looks_like_a_prototype = re.compile(r"\bdsa_[a-z0-9_]+\s*\(").search
    for stmt in filter(looks_like_a_prototype, re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).split(";")):
        m = _PROTOTYPE.fullmatch(stmt)
        restype = m and _RETURNS.get(re.sub(r"\s*\*", "*", " ".join(m.group(1).split())))
        if not restype:
            raise BackendError(f"{HEADER}: cannot parse the prototype `{' '.join(stmt.split())[:200]}`")
        argtypes = []
        for param in [] if m.group(3).strip() in ("", "void") else m.group(3).split(","):
            p = re.fullmatch(r"\s*(.+?)\s*\b\w+\s*", param)   # `<type> <parameter name>`
            ctype = p and (C.c_void_p if p.group(1).endswith("*") else _VALUES.get(p.group(1)))   # any pointer: an address
            if not ctype:
                raise BackendError(f"{HEADER}: {m.group(2)}: parameter `{param.strip()}` has no ctypes mapping")
            argtypes.append(ctype)
        signatures[m.group(2)] = (restype, argtypes)
    return signatures, constants


if not os.path.isfile(HEADER):
    raise BackendError(f"the C header {HEADER} is missing: the ctypes bindings are read from it")
SIGNATURES, CONSTANTS = parse_header(open(HEADER).read())   # name -> (restype, [argtypes]); "DSA_..." -> int
# every constant under its header name without the prefix: F32, SCRATCH_BYTES, ERR_UNSUPPORTED, ALGO_TUNED, ROWS_TRANS, PAD_REFLECT, ...
globals().update({name[len("DSA_"):]: value for name, value in CONSTANTS.items()})


def env_text(name: str) -> str:
    """The value of a DSA_* switch, "" when it is unset (csrc/env.h has the same pair; the table of record: INTEGRATION.md,
    "Environment switches").  Read at every call, never cached."""
    return os.environ.get(name, "")


def env_int(name: str, default: int) -> int:
    """An optional '-' and 1 to 9 decimal digits, nothing else; any other value (unset, empty, spaces, trailing text) gives
    `default`.  An on/off switch is env_int(name, d) != 0; a three-state one has default -1, 0 never, 1 always."""
    v = os.environ.get(name)
    if v is None:   # (the usual case costs what the bare read cost: these sit in front of launches of a few microseconds)
        return default
    digits = v[1:] if v[:1] == "-" else v
    return int(v) if 1 <= len(digits) <= 9 and digits.isascii() and digits.isdigit() else default


def algo_reserve_cus(n: int) -> int:
    """DSA_ALGO_RESERVE_CUS(n)"""
    return (int(n) & 63) << 16


def _sources():
    files = [os.path.join(CSRC, s) for s in SOURCES]
    deps = files + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + [os.path.join(_ROOT, "include", "diffsptk_amd.h"),
                    os.path.abspath(__file__)]   # the build flags live in this file
    return files, deps


def is_stale() -> bool:
    _, deps = _sources()
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into one shared library (cross-compiles w/o GPU)."""
    if not force and not is_stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise BackendError("hipcc not found: cannot build libdiffsptk_amd.so")
    os.makedirs(LIB_DIR, exist_ok=True)
    files, _ = _sources()
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    objs, procs = [], []
    for f in files:   # one object per source (its own flags), compiled concurrently, then one link
        obj = os.path.join(obj_dir, os.path.basename(f) + ".o")
        cmd = [hipcc, *HIPCC_FLAGS, *SOURCE_FLAGS.get(os.path.basename(f), ()), "-c", f, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for cmd, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            raise BackendError("hipcc failed: " + " ".join(cmd) + "\n" + out)
    tmp = LIB_PATH + ".tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden", "-o", tmp, *objs]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise BackendError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, LIB_PATH)
    global _lib
    _lib = None
    return LIB_PATH


def load():
    """Load the library (after torch, so both share one HIP runtime) and bind signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  diffsptk_amd has no CPU fallback."
        )
    import torch  # noqa: F401  (loads torch's libamdhip64.so first: one runtime per process)

    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise BackendError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().dsa_last_error().decode(errors="replace")
        raise BackendError(f"{what or 'diffsptk_amd call'} failed (status {rc}): {msg}")


def last_kernel() -> str:
    return load().dsa_last_kernel().decode()
