#!/usr/bin/env python3
"""Golden fixtures for the GRADIENTS of the MLSA filter (PseudoMGLSADigitalFilter, mglsadf.py) in every mode, phase and precision, by
importing the REFERENCE.  Build container only.

    python tests/golden/make_golden_mlsa_grad.py     # writes tests/golden/mlsa_grad.npz (float64) and mlsa_grad.json (the case list)

Inputs.  Speech cepstra as make_golden_mlsa.py builds them: data.wav -> STFT(400, 80, 512) -> MelGeneralizedCepstralAnalysis(512, M,
alpha, c, n_iter=5), twelve frames (twenty for set D), c in {0, 2}: speech keeps 1 + gamma C away from zero, so that every reference
gradient is finite (asserted).  The excitation x and the cotangent gy are seeded Gaussian; the functional is linear: (y * gy).sum().
Mixed phase: the maximum-phase part is 0.3 times other frames' shapes, as make_golden_mlsa_mixed.py.

Per case (the list with every option is in mlsa_grad.json) from a float64 run of the reference: `<tag>_y`, `<tag>_gx`, `<tag>_gmc`; and
from the reference's own float32 run of the same case E_ref = max|ref32 - ref64| / max|ref64|, one number per quantity, in the JSON.

Sets.
  A  M = 24, P = 80, N = 12, alpha = 0.42, small parameters: every mode x {minimum, maximum, zero} x ignore_gain at c = 0, the
     minimum-phase rows again at c = 2, and one freq-domain case with frame_length = 512 and a Hamming window.
  B  mixed phase, filter_order = (12, 24): every mode x ignore_gain at c = 0, one mode at c = 2.
  C  the module's defaults (no keyword arguments): single-stage minimum / zero / mixed, multi-stage minimum / zero.
  D  M = 8, P = 10, N = 20, alpha = 0, gamma = 0: fewer than 16 taps per cepstrum and P % 4 != 0.
  E  one multi-stage case with x of shape (2, 2, T) (ignore_gain=True: the reference's gain path takes at most one batch dimension).
The file is written with fixed zip timestamps: the same tree gives the same bytes."""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy, read_wav_int16  # noqa: E402

SMALL = {"multi-stage": {"taylor_order": 7, "cep_order": 100}, "single-stage": {"ir_length": 200, "n_fft": 512},
         "freq-domain": {"frame_length": 400, "fft_length": 512}}
SMALL_MIXED = {"multi-stage": {"taylor_order": 7, "cep_order": [40, 60]}, "single-stage": {"ir_length": [80, 120], "n_fft": 512},
               "freq-domain": {"frame_length": 400, "fft_length": 512}}
TINY = {"multi-stage": {"taylor_order": 7}, "single-stage": {"ir_length": 12, "n_fft": 64},
        "freq-domain": {"frame_length": 32, "fft_length": 64}}
MODES = ("multi-stage", "single-stage", "freq-domain")


def case_list():
    """Every case: options only (E_ref is added by main())."""
    out = []

    def add(cset, tag, mode, phase, ig, c, kwargs, order=24, P=80, alpha=0.42, x="x", mc=None, gy="gy"):
        if mc is None:
            mc = f"mc_mixed_c{c}" if phase == "mixed" else f"mc_c{c}"
        out.append({"tag": tag, "set": cset, "mode": mode, "phase": phase, "ignore_gain": bool(ig), "c": c, "filter_order": order, "P": P,
                    "alpha": alpha, "kwargs": kwargs, "x": x, "mc": mc, "gy": gy})

    short = {"multi-stage": "multi", "single-stage": "single", "freq-domain": "freq"}
    for mode in MODES:
        for phase in ("minimum", "maximum", "zero"):
            for ig in (0, 1):
                add("A", f"A_{short[mode]}_{phase[:3]}_g{ig}_c0", mode, phase, ig, 0, SMALL[mode])
        for ig in (0, 1):
            add("A", f"A_{short[mode]}_min_g{ig}_c2", mode, "minimum", ig, 2, SMALL[mode])
    add("A", "A_freq_min_g0_c0_hamming", "freq-domain", "minimum", 0, 0, {"frame_length": 512, "fft_length": 512, "window": "hamming"})
    for mode in MODES:
        for ig in (0, 1):
            add("B", f"B_{short[mode]}_mix_g{ig}_c0", mode, "mixed", ig, 0, SMALL_MIXED[mode], order=[12, 24])
    add("B", "B_multi_mix_g0_c2", "multi-stage", "mixed", 0, 2, SMALL_MIXED["multi-stage"], order=[12, 24])
    for phase in ("minimum", "zero", "mixed"):
        add("C", f"C_single_{phase[:3]}", "single-stage", phase, 0, 0, {}, order=[12, 24] if phase == "mixed" else 24)
    for phase in ("minimum", "zero"):
        add("C", f"C_multi_{phase[:3]}", "multi-stage", phase, 0, 0, {})
    for mode in MODES:
        for phase in ("minimum", "zero"):
            add("D", f"D_{short[mode]}_{phase[:3]}", mode, phase, 0, 0, TINY[mode], order=8, P=10, alpha=0.0, x="x_d", mc="mc_d", gy="gy_d")
    # (ignore_gain: with the gain the reference interpolates c0 of shape (2, 2, N, 1), which its LinearInterpolation refuses)
    add("E", "E_multi_min_g1_batch", "multi-stage", "minimum", 1, 0, SMALL["multi-stage"], x="x_e", mc="mc_e", gy="gy_e")
    return out


def make_module(d, case, dtype):
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in case["kwargs"].items()}
    order = case["filter_order"]
    return d.MLSA(tuple(order) if isinstance(order, list) else order, case["P"], alpha=case["alpha"], c=case["c"],
                  ignore_gain=case["ignore_gain"], phase=case["phase"], mode=case["mode"], dtype=dtype, **kw)


def run(d, case, arrays, dtype):
    x = torch.from_numpy(arrays[case["x"]]).to(dtype).requires_grad_(True)
    mc = torch.from_numpy(arrays[case["mc"]]).to(dtype).requires_grad_(True)
    gy = torch.from_numpy(arrays[case["gy"]]).to(dtype)
    y = make_module(d, case, dtype)(x, mc)
    (y * gy).sum().backward()
    return [npy(t).astype(np.float64) for t in (y, x.grad, mc.grad)]


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps (numpy stamps every member with the time of writing)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    d = import_reference()
    f64 = torch.float64
    pcm, _ = read_wav_int16(os.path.join("/root/reference", "assets", "data.wav"))
    w = torch.from_numpy(pcm.astype(np.float64) / 32768.0)
    X = d.STFT(400, 80, 512, dtype=f64)(w)

    def cepstra(frames, M, alpha, c):
        return d.MelGeneralizedCepstralAnalysis(fft_length=512, cep_order=M, alpha=alpha, c=c, n_iter=5, dtype=f64)(X[frames])

    g = {}
    gen = torch.Generator().manual_seed(20240)
    randn = lambda *shape: npy(torch.randn(*shape, generator=gen, dtype=f64))   # noqa: E731
    g["x"], g["gy"] = randn(12 * 80), randn(12 * 80)
    g["x_d"], g["gy_d"] = randn(20 * 10), randn(20 * 10)
    g["x_e"], g["gy_e"] = randn(2, 2, 12 * 80), randn(2, 2, 12 * 80)
    for c in (0, 2):
        mc = cepstra(slice(40, 52), 24, 0.42, c)
        g[f"mc_c{c}"] = npy(mc)
        c_neg = 0.3 * mc[..., 1:13].flip(-2).flip(-1)                       # c_{-12} .. c_{-1}: other frames' shapes, scaled
        g[f"mc_mixed_c{c}"] = npy(torch.cat((c_neg, mc), dim=-1))
    g["mc_d"] = npy(cepstra(slice(40, 60), 8, 0.0, 0))
    g["mc_e"] = npy(torch.stack([cepstra(slice(s, s + 12), 24, 0.42, 0) for s in (40, 64, 88, 112)]).reshape(2, 2, 12, 25))
    base = np.load(os.path.join(HERE, "mlsa.npz"))                          # the same cepstra as the forward goldens'
    assert all(np.array_equal(g[f"mc_c{c}"], base[f"mlsa_mc_c{c}"]) for c in (0, 2))

    cases = case_list()
    assert len({c["tag"] for c in cases}) == len(cases)
    for case in cases:
        ref64 = run(d, case, g, torch.float64)
        ref32 = run(d, case, g, torch.float32)
        case["E_ref"] = {}
        for name, a64, a32 in zip(("y", "gx", "gmc"), ref64, ref32):
            assert np.isfinite(a64).all() and np.isfinite(a32).all() and np.abs(a64).max() > 0, (case["tag"], name)
            e = float(np.abs(a32 - a64).max() / np.abs(a64).max())
            assert 0 < e < 1e-3, (case["tag"], name, e)
            case["E_ref"][name] = e
            g[f"{case['tag']}_{name}"] = a64
        assert ref64[0].shape == g[case["x"]].shape and ref64[1].shape == g[case["x"]].shape and ref64[2].shape == g[case["mc"]].shape
        print(case["tag"], {k: f"{v:.3g}" for k, v in case["E_ref"].items()})

    write_npz(os.path.join(HERE, "mlsa_grad.npz"), g)
    with open(os.path.join(HERE, "mlsa_grad.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    size = os.path.getsize(os.path.join(HERE, "mlsa_grad.npz"))
    assert size <= 1000000, size
    print("wrote mlsa_grad.npz:", len(g), "arrays,", size, "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
