#!/usr/bin/env python3
"""Golden fixtures of lpc2lsp / lsp2lpc / lspcheck, by importing the REFERENCE.  Build container only.

    python tests/golden/make_golden_lsp.py     # writes tests/golden/lsp.npz and lsp_api.json (data)

The frame sets, the seed and the shape of run() are those of make_golden_parcor.py: `integ`, `white` and `wav`, FRAMES Hann-windowed
frames of LENGTH samples each.  Per set and order M the input a = lpc(x, M) is stored once; per case the reference's outputs in
float64 and float32, weights w and the float64 and float32 gradients of sum(w * out): `<tag>_64` is [out, grad, w] in float64 and
`<tag>_32` is [out, grad] in float32.

lpc2lsp: every case passes the gate max|ref32 - ref64| <= GATE pi over the LSPs (asserted; 1.3e-5 pi is the worst seen).
lsp2lpc: its input is the reference's own float64 LSPs of a, so e_rt = max|ref64 - a| is the reference's OWN error: it is stored per
case in lsp_api.json.  Where the reference raises (float32 from M = 16 on, float64 at M = 63), the case is listed under "raises" with
the exception type and that dtype's output and gradient are absent.  Asserted: no float64 case raises at M <= 48 and no float32 case
at M <= 12.
lspcheck: inputs that need work -- the stored LSPs with a pair squeezed to a gap of 0, 1e-4 and -0.01, and with the end values pushed
to <= 0 and >= pi -- over rate x n_iter, ONE ROW PER CALL (the reference's early break looks at the whole batch: a row that has
converged is swept again while another has not, each time through the kink of torch.clip(min_distance - distance, min=0), and its
gradient then depends on its neighbours), at CHECK_ORDERS (the largest of them on `wav` only, for the size of lsp.npz).

The reference's deconv1d goes through torchaudio.functional.lfilter, which is not installed here: `lfilter` below, a direct-form
recursion in stock torch that autograd differentiates, is installed on the stub module that import_reference() injects."""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_golden_parcor import FRAMES, SETS, frames_of, sig  # noqa: E402

ORDERS = [0, 1, 2, 3, 9, 10, 12, 24, 25, 32, 33, 48, 63, 64]   # both parities: the trivial factors differ; 64 = DSA_LSP_MAX_ORDER
CHECK_ORDERS = [0, 1, 2, 3, 10, 25, 64]
OPTIONS = [{}, {"log_gain": True}, {"sample_rate": 16000, "out_format": "hz"}]
RATES, N_ITERS = [0, 0.01, 0.2], [0, 1, 10]
GATE = 1e-4
OPTION_FRAMES = 2   # the options other than the defaults run on the first frames of each set: lsp.npz stays below 1 MiB
COVERAGE = ("Thinner than orders x sets x options x frames, to keep lsp.npz below 1 MiB: options[0] runs on all `frames` frames of each set, "
            "options[1:] on the first `option_frames`; lspcheck is stored at `check_orders` only, the largest of them on `wav` only "
            "(tests/test_gpu_lsp.py holds lspcheck at orders 24, 25, 63 and 64 against a restatement that is bit-identical to these fixtures).")


def lfilter(x, a, b, clamp=False, batching=True):
    """y[n] = (sum_k b[k] x[n-k] - sum_{k>=1} a[k] y[n-k]) / a[0], one filter per row: x:(B, T), a, b:(B, K)."""
    assert not clamp and batching
    y = []
    for n in range(x.size(-1)):
        acc = sum(b[..., k] * x[..., n - k] for k in range(min(b.size(-1), n + 1)))
        acc = acc - sum(a[..., k] * y[n - k] for k in range(1, min(a.size(-1), n + 1)))
        y.append(acc / a[..., 0])
    return torch.stack(y, -1)


def inverse_options(o):
    return {("in_format" if k == "out_format" else k): v for k, v in o.items()}


def squeezed(w):
    """(6, M+1) float64: rows 0-2 with one pair squeezed to a gap of 0, 1e-4 and -0.01, rows 3-5 with w_1 <= 0, w_M >= pi, and both."""
    w = w.copy()
    M = w.shape[-1] - 1
    if M >= 1:
        for r, gap in enumerate((0.0, 1e-4, -0.01)):
            if M >= 2:
                j = 1 + (r * (M - 1)) // 3
                w[r, j + 1] = w[r, j] + gap
        w[3, 1] = -0.05
        w[4, M] = np.pi + 0.02
        w[5, 1], w[5, M] = 0.0, np.pi
    return w


def main():
    d = import_reference()
    sys.modules["torchaudio"].functional = types.SimpleNamespace(lfilter=lfilter)
    F = d.functional
    rng = np.random.default_rng(20241017)
    out, gate, e_rt, raises = {}, {}, {}, {}

    def run(tag, fn, x64):
        """The reference on x64 in both dtypes with the gradient of a weighted sum; a dtype in which it raises is recorded.  Returns
        {"64": [out, grad, weights] in float64, "32": [out, grad] in float32} without the dtype that raised (the weights are exact
        in every dtype; few large arrays, because an .npz spends a quarter of a KiB on each one)."""
        w = rng.standard_normal(x64.shape).astype(np.float16).astype(np.float64)
        got = {}
        for name, dt in (("64", torch.float64), ("32", torch.float32)):
            xt = torch.tensor(x64, dtype=dt, requires_grad=True)
            try:
                y = fn(xt)
                (y * torch.tensor(w, dtype=dt)).sum().backward()
            except Exception as e:   # noqa: BLE001
                raises.setdefault(tag, {})["f" + name] = [type(e).__name__, str(e)]
                continue
            got[name] = np.stack([y.detach().numpy(), xt.grad.numpy()] + ([w] if name == "64" else []))
        return got

    def keep(tag, got):
        for name, arr in got.items():
            out[f"{tag}_{name}"] = arr

    for s in SETS:
        x = torch.tensor(frames_of(s, rng))
        for M in ORDERS:
            a = F.lpc(x, max(M, 1))[..., :M + 1].numpy()   # M = 0: the gain alone
            out[f"a_{s}_{M}"] = a
            for oi, o in enumerate(OPTIONS):
                tag = f"lpc2lsp_{s}_{M}_{oi}"
                a = out[f"a_{s}_{M}"][:FRAMES if oi == 0 else OPTION_FRAMES]
                got = run(tag, lambda t: F.lpc2lsp(t, **o), a)
                assert tag not in raises, raises
                keep(tag, got)
                y64, y32 = got["64"][0], got["32"][0].astype(np.float64)
                scale = 1.0 if "out_format" not in o else 2 * np.pi / o["sample_rate"]
                gate[tag] = float(np.abs(y32 - y64)[..., 1:].max() * scale / np.pi) if M else 0.0
                lsp = y64[..., 1:] * scale
                assert gate[tag] <= GATE and (M == 0 or ((np.diff(lsp) > 0).all() and lsp.min() > 0 and lsp.max() < np.pi)), (tag, gate[tag])
                tag2 = f"lsp2lpc_{s}_{M}_{oi}"
                got = run(tag2, lambda t: F.lsp2lpc(t, **inverse_options(o)), y64)
                keep(tag2, got)
                if "64" in got:
                    e_rt[tag2] = float(np.abs(got["64"][0] - a).max())
                assert not (M <= 48 and "f64" in raises.get(tag2, {})) and not (M <= 12 and "f32" in raises.get(tag2, {})), raises[tag2]
            if M in CHECK_ORDERS and (s == "wav" or M <= 32):
                wbad = squeezed(out[f"lpc2lsp_{s}_{M}_0_64"][0])
                out[f"wbad_{s}_{M}"] = wbad
                tag = f"lspcheck_{s}_{M}"   # one array per dtype: [rate][n_iter][out, grad(, weights)]
                grid = [[run(tag, lambda t: torch.cat([F.lspcheck(r, rate, n_iter, "ignore") for r in t.split(1)]), wbad) for n_iter in N_ITERS] for rate in RATES]
                assert tag not in raises, raises
                keep(tag, {name: np.stack([np.stack([g[name] for g in row]) for row in grid]) for name in ("64", "32")})

    # the docstring examples (lpc2lsp.py:91-97, lsp2lpc.py:85-89, lspcheck.py:73-79)
    a = d.LPC(5, 2)(d.ramp(1, 5) * 0.1)
    out["doc_a"], out["doc_lpc2lsp"] = a.numpy(), F.lpc2lsp(a).numpy()
    out["doc_w"], out["doc_lsp2lpc"] = d.ramp(3).numpy(), F.lsp2lpc(d.ramp(3)).numpy()
    w1 = torch.tensor([1.0 / torch.pi, 0.0, 0.0, 0.5, 1.0]) * torch.pi
    out["doc_check_in"], out["doc_check_out"] = w1.numpy(), F.lspcheck(w1, rate=0.01, n_iter=10, warn_type="ignore").numpy()
    np.savez_compressed(os.path.join(HERE, "lsp.npz"), **out)

    classes = {"lpc2lsp": "LinearPredictiveCoefficientsToLineSpectralPairs", "lsp2lpc": "LineSpectralPairsToLinearPredictiveCoefficients",
               "lspcheck": "LineSpectralPairsStabilityCheck"}
    api = {"orders": ORDERS, "check_orders": CHECK_ORDERS, "options": OPTIONS, "rates": RATES, "n_iters": N_ITERS, "sets": SETS, "frames": FRAMES, "option_frames": OPTION_FRAMES,
           "coverage": COVERAGE, "gate": gate, "e_rt": e_rt, "raises": raises, "names": classes,
           "classes": {c: {"init": sig(getattr(d, c).__init__), "forward": sig(getattr(d, c).forward)} for c in classes.values()},
           "functional": {f: sig(getattr(F, f)) for f in classes},
           "state": {c: list(getattr(d, c)(3).state_dict()) for c in classes.values()}, "errors": []}
    cases = [("ctor", f, [-1], {}, None) for f in classes]
    cases += [("ctor", "lpc2lsp", [3], kw, None) for kw in ({"out_format": "hz"}, {"out_format": "khz"}, {"out_format": 3, "sample_rate": 0},
                                                            {"out_format": "mel"}, {"out_format": 7, "sample_rate": 8000})]
    cases += [("ctor", "lsp2lpc", [3], kw, None) for kw in ({"in_format": "hz"}, {"in_format": "khz"}, {"in_format": 2, "sample_rate": -1},
                                                            {"in_format": "mel"}, {"in_format": 7, "sample_rate": 8000})]
    cases += [("ctor", "lspcheck", [3], kw, None) for kw in ({"rate": -0.1}, {"rate": 1.5}, {"n_iter": -1}, {"rate": 2, "n_iter": -1})]
    cases += [("ctor", "lspcheck", [-1], {"rate": 2}, None)]
    cases += [("call", f, [3], {}, [2, 5]) for f in classes]
    cases += [("functional", "lpc2lsp", [], {"out_format": "hz"}, [2, 4]), ("functional", "lpc2lsp", [], {"out_format": "mel"}, [2, 4]),
              ("functional", "lsp2lpc", [], {"in_format": "khz"}, [2, 4]), ("functional", "lsp2lpc", [], {"in_format": "mel"}, [2, 4]),
              ("functional", "lspcheck", [], {"rate": 1.5}, [2, 4]), ("functional", "lspcheck", [], {"n_iter": -1}, [2, 4])]
    for kind, f, args, kw, shape in cases:
        try:
            if kind == "ctor":
                getattr(d, classes[f])(*args, **kw)
            elif kind == "call":
                getattr(d, classes[f])(*args, **kw)(torch.zeros(shape, dtype=torch.float64))
            else:
                getattr(F, f)(torch.zeros(shape, dtype=torch.float64), *args, **kw)
            got = ["ok", ""]
        except Exception as e:   # noqa: BLE001
            got = [type(e).__name__, str(e)]
        api["errors"].append({"kind": kind, "module": f, "args": args, "kwargs": kw, "shape": shape, "raises": got})
    with open(os.path.join(HERE, "lsp_api.json"), "w") as f:
        json.dump(api, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
