"""The cases of WorldSynthesis that tests/golden/make_golden_world_synth.py runs through the reference and the tests run through the
package: shapes, F0 tracks and the formulas of every other input.  Nothing here is random: aperiodicity, spectral envelope, noise and
cotangents are integer hashes of the element's position (splitmix64's finaliser on uint64 arrays), scaled to values that are exact in
float32, so the fixture files hold results only.  The noise is the centred sum of four 16-bit fields of one hash, a multiple of 2^-15
with unit-like variance (1.33); what matters to the comparison is that both sides see the same numbers, not their law.

Not a test module."""
import json
import os

import numpy as np

# name -> options.  f0 rows are rounded to float32 before use.  `out_length` only where the call passes one.  The F0 tracks and default_f0
# values are non-round on purpose and were chosen so that every pulse keeps the margins the generator asserts; `sparse` steps 4.6e-3 rad
# per sample, so few values of default_f0 leave 1e-3 rad on both sides of all three wraps: 11.819 is one.
CASES = {
    "mixed_odd": dict(P=75, sr=16000, L=1024, default_f0=487.3, batched=True,
                      f0=[[121.3, 125.7, 131.9, 0.0, 0.0, 12.4, 205.3, 211.7], [0.0, 0.0, 301.3, 287.9, 263.1, 0.0, 171.7, 0.0]]),
    "mixed_even": dict(P=80, sr=16000, L=1024, default_f0=487.3, batched=True,
                       f0=[[121.3, 125.7, 131.9, 0.0, 0.0, 12.4, 205.3, 211.7], [0.0, 0.0, 301.3, 287.9, 263.1, 0.0, 171.7, 0.0]]),
    "voiced_unvoiced": dict(P=75, sr=16000, L=1024, default_f0=491.3, batched=True,
                            f0=[[121.3, 126.1, 133.3, 140.3, 151.1, 163.7, 171.3, 180.9], [0.0] * 8]),
    "unbatched": dict(P=75, sr=16000, L=1024, default_f0=487.3, batched=False, out_length=500,
                      f0=[[0.0, 144.7, 151.9, 158.3, 0.0, 0.0, 231.1, 241.7]]),
    "wide": dict(P=225, sr=48000, L=2048, default_f0=487.3, batched=True, f0=[[0.0, 201.3, 215.7, 0.0, 0.0, 187.9]]),
    "sparse": dict(P=750, sr=16000, L=1024, default_f0=11.819, batched=True, f0=[[0.0] * 7]),
    "ceiling_f32": dict(P=75, sr=16000, L=8192, default_f0=487.3, batched=True, f0=[[151.3, 163.7, 0.0, 0.0]], dtypes=["float32"]),
    "ceiling_f64": dict(P=75, sr=16000, L=4096, default_f0=487.3, batched=True, f0=[[151.3, 163.7, 0.0, 0.0]]),
}
# which fixture file holds a case's results (no committed file may pass 1 MiB)
FILES = {"world_synth": ["mixed_odd", "mixed_even", "voiced_unvoiced", "unbatched", "sparse"],
         "world_synth_big": ["wide", "ceiling_f32", "ceiling_f64"]}
EPS = 1e-6   # the clip of ap and sp (world_synth.py:189-191)


def _hash(n, seed):
    """n uint64 hashes of 0 .. n-1 under `seed`"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def normal_like(shape, seed):
    """float32 multiples of 2^-15 in [-4, 4): four 16-bit fields of one hash, summed and centred"""
    z = _hash(int(np.prod(shape)), seed)
    s = sum(((z >> np.uint64(16 * i)) & np.uint64(0xFFFF)).astype(np.int64) for i in range(4))
    return ((s - 131070).astype(np.float64) / 32768.0).astype(np.float32).reshape(shape)


def uniform_like(shape, seed):
    """float32 multiples of 2^-12 in [0, 1)"""
    z = _hash(int(np.prod(shape)), seed)
    return (((z >> np.uint64(20)) & np.uint64(0xFFF)).astype(np.float64) / 4096.0).astype(np.float32).reshape(shape)


def seed_of(name):
    return 1000 * (1 + sorted(CASES).index(name))


def inputs(name):
    """(f0, ap, sp) as float32 arrays, batched (B, N) / (B, N, D).  ap holds exact 0 and 1, sp values below the clip and one exact 0."""
    c = CASES[name]
    f0 = np.asarray(c["f0"], dtype=np.float32)
    B, N = f0.shape
    D = c["L"] // 2 + 1
    s = seed_of(name)
    ap = (0.03125 + 0.9375 * uniform_like((B, N, D), s + 1)).astype(np.float32)
    k = np.arange(D, dtype=np.float64) / (D - 1)
    envelope = np.exp(-4.0 * k) * (1.0 + 0.5 * np.cos(9.0 * k))   # a falling spectrum with a few formant-like bumps
    sp = np.round((0.0625 + uniform_like((B, N, D), s + 2)) * envelope * 4096.0 + 1.0) / 4096.0
    sp = sp.astype(np.float32)
    marks = _hash(B * N * D, s + 3).reshape(B, N, D) % np.uint64(97)
    ap[marks == 0] = 0.0
    ap[marks == 1] = 1.0
    sp[marks == 2] = np.float32(2.0 ** -21)   # 4.8e-7, below the clip
    sp[marks == 3] = 0.0
    return f0, ap, sp


def noise(name, rows, L):
    return normal_like((rows, L), seed_of(name) + 4)


def cotangent(name, shape):
    return normal_like(shape, seed_of(name) + 5)


def shaped(name, f0, ap, sp):
    """the arrays as the call takes them: the leading axis dropped where the case is unbatched"""
    return (f0, ap, sp) if CASES[name]["batched"] else (f0[0], ap[0], sp[0])


def options(name):
    c = CASES[name]
    return (c["P"], c["sr"], c["L"]), dict(default_f0=c["default_f0"])


def dtypes_of(name):
    return CASES[name].get("dtypes", ["float64", "float32"])


def load(golden_dir):
    """(api, arrays): world_synth_api.json and the union of the fixture files"""
    with open(os.path.join(golden_dir, "world_synth_api.json")) as f:
        api = json.load(f)
    arrays = {}
    for stem in FILES:
        with np.load(os.path.join(golden_dir, stem + ".npz")) as z:
            arrays.update({k: z[k] for k in z.files})
    return api, arrays


def _zeros(*shape, dtype=None):
    import torch

    return torch.zeros(*shape, dtype=dtype)


# invalid calls: name -> callable(package); the fixture holds the reference's exception type and text for each
ERRORS = {
    "frame_period": lambda d: d.WorldSynthesis(0, 16000, 1024),
    "sample_rate": lambda d: d.WorldSynthesis(80, 7999, 1024),
    "fft_length": lambda d: d.WorldSynthesis(80, 16000, 1023),
    "f0_ndim": lambda d: d.WorldSynthesis(80, 16000, 1024)(_zeros(1, 2, 3), _zeros(1, 2, 3, 513), _zeros(1, 2, 3, 513)),
    "ap_ndim": lambda d: d.WorldSynthesis(80, 16000, 1024)(_zeros(2, 3), _zeros(3, 513), _zeros(2, 3, 513)),
    "batch": lambda d: d.WorldSynthesis(80, 16000, 1024)(_zeros(2, 3), _zeros(1, 3, 513), _zeros(2, 3, 513)),
    "length": lambda d: d.WorldSynthesis(80, 16000, 1024)(_zeros(2, 3), _zeros(2, 3, 513), _zeros(2, 4, 513)),
    "dimension": lambda d: d.WorldSynthesis(80, 16000, 1024)(_zeros(2, 3), _zeros(2, 3, 513), _zeros(2, 3, 512)),
}
