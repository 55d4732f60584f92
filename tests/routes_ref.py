"""float64 restatements, on the CPU, of the operations behind the kernel routes of tests/kernel_routes.py -- shared by
tests/test_gpu_routes.py (the reference of every case) and tests/test_routes_cpu.py (the inputs are checked here, without a GPU).

Every restatement is written from the operation's definition with torch tensor operations, so that float64 autograd through it
is the reference of the gradient kernels, and takes the dtype of its inputs, so that the same text evaluated in float32 measures what
float32 arithmetic costs.  Sums, matrix products and linear solves go through rsum / rmm / rsolve: with `reversed_order()` active
they accumulate (eliminate) in the opposite order, which gives the second float64 evaluation the measured tolerances are taken from:

    float64 bound = 64 x max(|ref - ref reversed| / max|ref|, 2^-53)      float32 bound = 8 x max(|ref32 - ref| / max|ref|, 2^-24)

(the floor is the rounding unit of the output format: two evaluations that happen to agree to the bit say nothing about a third that
is merely rounded correctly).  `python tests/routes_ref.py` prints the base values of every measured case of the table.

INPUTS[call](**args) -> {name: float64 tensor}; REFS[call](inputs, **args) -> tensor (or tuple of tensors)."""
import contextlib
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffsptk_amd.utils import tables   # noqa: E402  (host tables: numpy, no device)
from oracle import torch_port as TP     # noqa: E402

_REVERSED = [False]
U64, U32 = 2.0 ** -53, 2.0 ** -24


@contextlib.contextmanager
def reversed_order():
    _REVERSED[0] = True
    try:
        yield
    finally:
        _REVERSED[0] = False


def rsum(x, dim=-1):
    return x.flip(dim).sum(dim) if _REVERSED[0] else x.sum(dim)


def rmm(a, b):
    """a @ b; reversed: the inner and the outer index run backwards, so the products of the backward pass do too"""
    return (a.flip(-1) @ b.flip(-2, -1)).flip(-1) if _REVERSED[0] else a @ b


def rsolve(A, b):
    """solve(A, b) per row of b; reversed: the same system with its unknowns and equations in the opposite order"""
    if _REVERSED[0]:
        return torch.linalg.solve(A.flip(-1, -2), b.flip(-1).unsqueeze(-1)).squeeze(-1).flip(-1)
    return torch.linalg.solve(A, b.unsqueeze(-1)).squeeze(-1)


def gauss(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def const(a, like):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).to(like.dtype)


# ----------------------------------------------------------------------------------------------- csrc/lpc.hip
def lag_sums(x, M):
    """r[m] = sum_l x[l] x[l + m]; reversed: the lags are formed last to first, so autograd adds their cotangents into x in that order"""
    L = x.size(-1)
    lags = [rsum(x[..., :L - m] * x[..., m:]) for m in (range(M, -1, -1) if _REVERSED[0] else range(M + 1))]
    return torch.stack(lags[::-1] if _REVERSED[0] else lags, -1)


def acorr(inp, L, M, fmt, F=3):
    """acorr.py:94-120: r[m] = sum_l x[l] x[l + m]; naive / normalized / biased / unbiased"""
    r = lag_sums(inp["x"], M)
    if fmt == 1:
        return r / r[..., :1]
    if fmt == 2:
        return r / L
    if fmt == 3:
        return r / (L - torch.arange(M + 1)).to(r.dtype)
    return r


def acorr_inputs(L, M, fmt, F=3):
    return {"x": gauss(1000 * L + 10 * M + fmt, F, L)}


def levdur_of(r, eps):
    """levdur.py:113-127: (toeplitz(r[:M]) + eps I) a = -r[1:], K = sqrt(r[1:] . a + r[0])"""
    M = r.size(-1) - 1
    if M == 0:
        return torch.sqrt(r)
    i = torch.arange(M)
    R = r[..., (i[:, None] - i[None, :]).abs()] + eps * torch.eye(M, dtype=r.dtype)
    a = rsolve(R, -r[..., 1:])
    K = torch.sqrt(rsum(r[..., 1:] * a).unsqueeze(-1) + r[..., :1])
    return torch.cat([K, a], -1)


def levdur(inp, M, eps, F=5):
    return levdur_of(inp["r"], eps)


def levdur_inputs(M, eps, F=5):
    """the autocorrelation of Gaussian frames four times as long as the system (issue: frames at least four times the order)"""
    return {"r": lag_sums(gauss(77 + M, F, 4 * (M + 1)), M)}


def lpc(inp, L, M, eps, F=3):
    return levdur_of(lag_sums(inp["x"], M), eps)


def lpc_inputs(L, M, eps, F=3):
    return {"x": gauss(31 * L + M, F, L)}


def fwlpc(inp, T, L, P, M, eps, center=True, B=2, exact=False):
    """README.md:198-201 of the reference: LPC(Window(Frame(x)))"""
    fr = TP.frame(inp["x"], L, P, center) * inp["w"]
    return levdur_of(lag_sums(fr, M), eps)


def fwlpc_inputs(T, L, P, M, eps, center=True, B=2, exact=False):
    return {"x": gauss(L + P + M, B, T), "w": torch.from_numpy(tables.window_table(L))}


fuse_fwlpc, fuse_fwlpc_inputs = fwlpc, fwlpc_inputs   # fuse(Frame, Window, LPC): the same definition, through the three modules where the one launch refuses


# ----------------------------------------------------------------------------------------------- csrc/zerodf.hip
def zerodf(inp, M, P, z0, ig, N, B=2):
    """zerodf.py:184-243: y[t] = sum_k h_t[k] x[t - k + z0], h_t the taps of frames n and n + 1 interpolated over P samples, divided by
    the gain tap (the last tap when zeroth_index = M, else the first) with ignore_gain"""
    x, b = inp["x"], inp["b"]
    T = N * P
    t = torch.arange(T)
    n0, w = t // P, ((t % P).to(x.dtype) / P)
    n1 = torch.clamp(n0 + 1, max=N - 1)
    h = b[:, n0] * (1 - w)[None, :, None] + b[:, n1] * w[None, :, None]
    xp = TF.pad(x, (M, M))
    idx = t[:, None] - torch.arange(M + 1)[None, :] + z0 + M
    y = rsum(h * xp[:, idx])
    if ig:
        y = y / h[..., M if (z0 == M and M > 0) else 0]
    return y


def zerodf_inputs(M, P, z0, ig, N, B=2):
    """taps with 1.5 added on both end taps (tests/test_gpu_synth.py): the gain tap stays away from zero"""
    b = 0.05 * gauss(M + P + z0, B, N, M + 1)
    b[..., 0] += 1.5
    b[..., -1] += 1.5
    return {"x": gauss(M * P + N, B, N * P), "b": b}


# ----------------------------------------------------------------------------------------------- csrc/spec.hip
def half_dft(x, nfft):
    """(re, im) of rfft(x, n = nfft): the first nfft samples, zero-padded, against the cosine and sine matrices"""
    L = min(x.size(-1), nfft)
    re, im = [], []
    for k0 in range(0, nfft // 2 + 1, 1024):   # (1024 bins at a time: the rows at the LDS ceilings would need a gigabyte of angles otherwise)
        k = torch.arange(k0, min(k0 + 1024, nfft // 2 + 1), dtype=torch.float64)
        ang = 2 * math.pi * ((torch.arange(L, dtype=torch.float64)[:, None] * k[None, :]) % nfft) / nfft
        re.append(rmm(x[..., :L], torch.cos(ang).to(x.dtype)))
        im.append(-rmm(x[..., :L], torch.sin(ang).to(x.dtype)))
    return torch.cat(re, -1), torch.cat(im, -1)


def fftr(inp, len_in, nfft, fmt, F=5):
    """fftr.py:136-151: complex (as (re, im) pairs) / real / imaginary / amplitude / power"""
    re, im = half_dft(inp["x"], nfft)
    return [torch.stack([re, im], -1), re, im, torch.sqrt(re * re + im * im), re * re + im * im][fmt]


def fftr_inputs(len_in, nfft, fmt, F=5):
    return {"x": gauss(100 * nfft + len_in, F, len_in)}


def spec_format(sv, floor, fmt):
    if floor is not None:
        sv = torch.maximum(sv, sv.amax(-1, keepdim=True) * 10 ** (floor / 10))
    return [10 * torch.log10(sv), 0.5 * torch.log(sv), torch.sqrt(sv), sv][fmt]


def spec(inp, lb, la, nfft, eps, floor, fmt, F=5):
    """spec.py:152-178: |K B / A|^2 + eps on nfft / 2 + 1 bins, K = a[0] and A = [1, a[1:]]; relative floor; db / log-magnitude /
    magnitude / power"""
    sv = None
    if lb:
        re, im = half_dft(inp["b"], nfft)
        sv = re * re + im * im
    if la:
        a = inp["a"]
        re, im = half_dft(torch.cat([torch.ones_like(a[..., :1]), a[..., 1:]], -1), nfft)
        sv = (sv if sv is not None else 1.0) * a[..., :1] ** 2 / (re * re + im * im)
    return spec_format(sv + eps, floor, fmt)


def spec_inputs(lb, la, nfft, eps, floor, fmt, F=5):
    """a = [K, a_1 ..] with small a_m: A(z) has no zero near the unit circle, so the spectrum stays bounded away from zero and infinity"""
    out = {}
    if lb:
        out["b"] = gauss(nfft + lb, F, lb)
    if la:
        a = 0.4 / la * gauss(nfft + la + 1, F, la)
        a[..., 0] = 1.5 + 0.25 * gauss(la, F)
        out["a"] = a
    return out


def stft(inp, T, L, P, nfft, eps=1e-9, B=2):
    """stft.py:237-241: Frame (centred, constant padding) -> Window -> power spectrum"""
    re, im = half_dft(TP.frame(inp["x"], L, P) * inp["w"], nfft)
    return re * re + im * im + eps


def stft_inputs(T, L, P, nfft, eps=1e-9, B=2):
    return {"x": gauss(T + L, B, T), "w": torch.from_numpy(tables.window_table(L))}


def irfft_scale(inp, nfft, F=5):
    """ifftr.py:138 restated for the adjoint transform: c_k / nfft times the half spectrum, c = 1, 2, .., 2, 1"""
    c = torch.full((nfft // 2 + 1, 1), 2.0, dtype=inp["y"].dtype)
    c[0] = c[-1] = 1.0
    return inp["y"] * c / nfft


def irfft_scale_inputs(nfft, F=5):
    return {"y": gauss(nfft, F, nfft // 2 + 1, 2)}


# ----------------------------------------------------------------------------------------------- csrc/thsolve.hip, mcep.hip (row products)
def thsolve(inp, n, F=37):
    """mgcep.py:226-229: solve(symmetric_toeplitz(p) + hankel(q), r)"""
    i = torch.arange(n)
    A = inp["p"][..., (i[:, None] - i[None, :]).abs()] + inp["q"][..., i[:, None] + i[None, :]]
    return rsolve(A, inp["r"])


def thsolve_inputs(n, F=37):
    """a dominant diagonal (tests/test_gpu_synth.py::test_thsolve_kernel_vs_numpy_and_gradcheck): condition numbers of a few units"""
    p = gauss(n, F, n)
    p[:, 0] += 2.0 * n
    return {"p": p, "q": 0.3 * gauss(n + 1, F, 2 * n - 1), "r": gauss(n + 2, F, n)}


def freqt(inp, L1, L2, F=5):
    return rmm(inp["c"], inp["A"])


def freqt_inputs(L1, L2, F=5):
    return {"c": gauss(L1 * 7 + L2, F, L1), "A": gauss(L1 + L2 * 3, L1, L2)}


def rows_log(inp, n):
    return torch.log(inp["x"])


def rows_log_inputs(n):
    return {"x": gauss(n, n).square() + 0.1}


def rows_expsub(inp, n):
    return torch.exp(inp["a"] - 2 * inp["b"])


def rows_expsub_inputs(n):
    return {"a": gauss(n, n), "b": gauss(n + 1, n)}


# ----------------------------------------------------------------------------------------------- csrc/fftcep.hip, fbank.hip
def fftcep(inp, nfft, M, accel, n_iter, F=5):
    """fftcep.py:116-136 (the improved cepstral method): every transform acts on a real even sequence"""
    x = inp["x"]
    H, N = nfft // 2 + 1, M + 1
    e = torch.fft.irfft(torch.log(x))
    v = e[..., :N]
    e = TF.pad(e[..., N:H], (N, 0))
    for _ in range(n_iter):
        e = torch.fft.ihfft(torch.relu(torch.fft.hfft(e))).real
        t = e[..., :N] * (1 + accel)
        v = v + t
        e = e - TF.pad(t, (0, H - N))
    scale = torch.ones(N, dtype=x.dtype)
    scale[0] = 0.5
    if H == N:
        scale[-1] = 0.5
    return v * scale


def fftcep_inputs(nfft, M, accel, n_iter, F=5):
    """a power spectrum between 0.3 and 1.3 (tests/test_gpu_parity.py::test_fftcep_gradcheck_and_full_size): log and 1 / x stay tame"""
    return {"x": torch.rand(F, nfft // 2 + 1, generator=torch.Generator().manual_seed(nfft + M), dtype=torch.float64) + 0.3}


def fbank(inp, nfft, C, use_power, gamma, floor=1e-5, F=7):
    """fbank.py:306-321: (y, E), y = log / generalized log of max(H^T sqrt(x) or H^T x, floor), E = log of the mean power"""
    x = inp["x"]
    H = const(tables.fbank_matrix(nfft, C, 16000), x)
    s = torch.clamp(rmm(x if use_power else torch.sqrt(x), H), min=floor)
    y = torch.log(s) if gamma == 0 else (s ** gamma - 1) / gamma
    E = torch.log((x[..., :1] + x[..., -1:] + 2 * rsum(x[..., 1:-1]).unsqueeze(-1)) / (nfft))
    return y, E


def fbank_inputs(nfft, C, use_power, gamma, floor=1e-5, F=7):
    return {"x": torch.rand(F, nfft // 2 + 1, generator=torch.Generator().manual_seed(nfft + C), dtype=torch.float64) + 0.1}


def mfcc(inp, nfft, C, M, lifter=22, floor=1e-5, F=7):
    """mfcc.py:244-256 as the entry returns it: (the amplitude-domain log filter bank times DCT-II x truncation x lifter, E)"""
    x = inp["x"]
    y, E = fbank(inp, nfft, C, False, 0.0, floor)
    return rmm(y, const(tables.dct_matrix(C, 2)[:, :M + 1] * tables.mfcc_lifter(M, lifter)[None, :], x)), E


def mfcc_inputs(nfft, C, M, lifter=22, floor=1e-5, F=7):
    return fbank_inputs(nfft, C, False, 0.0, floor, F)


def stft_fbank(inp, T, C, B=2):
    """fuse(STFT(400, 80, 512), MelFilterBankAnalysis(512, C, 16000)): the log filter-bank output of the power spectrogram"""
    x = inp["x"]
    X = TP.stft_power(x, 400, 80, 512, torch.from_numpy(tables.window_table(400)).to(x.dtype))
    return fbank({"x": X}, 512, C, False, 0.0)[0]


def stft_fbank_inputs(T, C, B=2):
    return {"x": gauss(T + C, B, T)}


# ----------------------------------------------------------------------------------------------- csrc/pqmf.hip
def _pq_pads(M, analysis):
    if M % 2 == 0:
        return M // 2, M // 2
    return ((M + 1) // 2, (M - 1) // 2) if analysis else ((M - 1) // 2, (M + 1) // 2)


def pqmf(inp, K, M, T, P=1, s=0, B=2):
    """pqmf.py of the reference: zero pad left, replicate pad right, K filters of M + 1 stored (time-flipped) taps; the decimation folded in"""
    x, f = inp["x"], inp["f"]
    dl, dr = _pq_pads(M, True)
    xp = torch.cat([torch.zeros(B, dl, dtype=x.dtype), x, x[:, -1:].expand(B, dr)], 1)
    return rmm(xp.unfold(1, M + 1, 1), f.T).transpose(1, 2)[..., s::P]


def pqmf_inputs(K, M, T, P=1, s=0, B=2):
    return {"x": gauss(K * M + T, B, T), "f": 0.3 * gauss(K + M, K, M + 1)}


def ipqmf(inp, K, M, T, U=1, s=0, B=2):
    """ipqmf.py of the reference on the interpolated subband signals (zeros between the samples, `s` zeros in front)"""
    y, f = inp["y"], inp["f"]
    Tu = T * U + s
    yu = torch.zeros(B, K, Tu, dtype=y.dtype)
    yu[..., s::U] = y
    dl, dr = _pq_pads(M, False)
    yp = torch.cat([torch.zeros(B, K, dl, dtype=y.dtype), yu, yu[..., -1:].expand(B, K, dr)], 2)
    return rsum(rsum(yp.unfold(2, M + 1, 1) * f[None, :, None, :]), 1)


def ipqmf_inputs(K, M, T, U=1, s=0, B=2):
    return {"y": gauss(K * M + T + 1, B, K, T), "f": 0.3 * gauss(K + M + 1, K, M + 1)}


def interpolate(inp, T, P, s):
    """interpolate.py of the reference along the middle axis: x[t] at s + t P, zeros elsewhere"""
    x = inp["x"]
    y = torch.zeros(x.size(0), T * P + s, x.size(2), dtype=x.dtype)
    y[:, s::P] = x
    return y


def interpolate_inputs(T, P, s):
    return {"x": gauss(T + P + s, 3, T, 5)}


# ----------------------------------------------------------------------------------------------- csrc/paramgen.hip
def delta(inp, T, D, seed, B=2):
    """delta.py:105-178: y[t, h, d] = sum_j window[h, j] x[clamp(t + j - N, 0, T - 1), d] (tests/paramgen_ref.py)"""
    import paramgen_ref as R

    x = inp["x"]
    w = const(R.window_of(R.SEEDS[seed]), x)
    Hn, L = w.shape
    idx = torch.clamp(torch.arange(T)[:, None] + torch.arange(L)[None, :] - (L - 1) // 2, 0, T - 1)
    return rsum(w[None, None, :, :, None] * x[:, idx][:, :, None], 3).reshape(B, T, Hn * D)


def delta_inputs(T, D, seed, B=2):
    return {"x": gauss(T + D, B, T, D)}


def mlpg(inp, T, D, seed, B=2):
    """mlpg.py:146-156: c = (W^T W)^-1 W^T u with the edge rules of tests/paramgen_ref.py::mlpg_matrix"""
    import paramgen_ref as R

    u = inp["u"]
    W = const(R.mlpg_matrix(T, R.window_of(R.SEEDS[seed]), R.th_of(R.SEEDS[seed])), u)
    Hn = W.size(0) // T
    rhs = rmm(W.T, u.reshape(B, T * Hn, D))
    return torch.stack([rsolve(rmm(W.T, W), rhs[b].T).T for b in range(B)])


def mlpg_inputs(T, D, seed, B=2):
    import paramgen_ref as R

    return {"u": gauss(T + D, B, T, D * (1 + len(R.SEEDS[seed])))}


# ----------------------------------------------------------------------------------------------- csrc/plp.hip, poledf.hip
def plp_tail(inp, C, M, n_fft, cf=0.33, lifter=22, F=5):
    """plp.py:312-320 behind the filter bank (tests/test_gpu_plp.py::restate): equal-loudness and compression, the autocorrelation
    as a cosine product, Levinson-Durbin as a recursion, the cepstrum of the all-pole model, liftering; out_format "ycE" """
    y, E = inp["y"], inp["E"]
    table = const(tables.plp_table(C, M, n_fft, 16000, 0, None, "htk", lifter), y)
    J = n_fft // 2 + 1
    q, Q, cs, sn, w, lift = torch.split(table, [C, (C + 2) * (M + 1), (M + 1) * J, (M + 1) * J, J, M + 1])
    Q, cs, sn = Q.view(C + 2, M + 1), cs.view(M + 1, J), sn.view(M + 1, J)
    v = (torch.exp(y) * q) ** cf
    r = rmm(torch.cat((v[..., :1], v, v[..., -1:]), -1), Q)
    a, err = [], r[..., 0]
    for m in range(1, M + 1):
        acc = r[..., m]
        for j in range(1, m):
            acc = acc + a[j - 1] * r[..., m - j]
        k = -acc / err
        a = [a[j - 1] + k * a[m - j - 1] for j in range(1, m)] + [k]
        err = err * (1 - k * k)
    a = torch.stack(a, -1)
    K = torch.sqrt(r[..., 0] + rsum(r[..., 1:] * a))
    re, im = 1 + rmm(a, cs[1:]), -rmm(a, sn[1:])
    lg = w * 0.5 * torch.log(re * re + im * im)
    c = torch.cat((torch.log(K)[..., None], rmm(lg, cs[1:].T)), -1) * lift
    return torch.cat([c[..., 1:], c[..., :1], E], -1)


def plp_tail_inputs(C, M, n_fft, cf=0.33, lifter=22, F=5):
    """log filter-bank outputs of a spectrum with a few units of dynamic range, and the frame's log energy"""
    return {"y": 1.5 * gauss(C + M, F, C), "E": gauss(C + M + 1, F, 1)}


def poledf(inp, M, P, N, ig, B=2):
    """poledf.py of the reference: y[t] = K_t x[t] - sum_k a_t[k] y[t - k], a_t interpolated between frames n and n + 1 (the last held),
    K_t = 1 with ignore_gain"""
    x, a = inp["x"], inp["a"]
    T = N * P
    t = torch.arange(T)
    n0, w = t // P, ((t % P).to(x.dtype) / P)[None, :, None]
    n1 = torch.clamp(n0 + 1, max=N - 1)
    c = a[:, n0] * (1 - w) + a[:, n1] * w
    ys = []
    for i in range(T):
        v = x[:, i] if ig else c[:, i, 0] * x[:, i]
        for k in range(1, min(M, i) + 1):
            v = v - c[:, i, k] * ys[i - k]
        ys.append(v)
    return torch.stack(ys, -1)


def poledf_inputs(M, P, N, ig, B=2):
    """a stable filter (tests/test_gpu_poledf.py): |a_k| below 0.6 / M, gains in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(M + P + N)
    a = (torch.rand(B, N, M + 1, generator=g, dtype=torch.float64) * 2 - 1) * 0.6 / max(M, 1)
    a[..., 0] = torch.rand(B, N, generator=g, dtype=torch.float64) + 0.5
    return {"x": gauss(M + P, B, N * P), "a": a}


# ----------------------------------------------------------------------------------------------- mel-cepstral analysis
def mcep(inp, nfft, M, alpha, n_iter, F=70):
    """mcep.py:189-224 (oracle/torch_port.py)"""
    return TP.mcep(inp["X"], TP.McepTables(nfft, M, alpha, inp["X"].dtype), n_iter)


def mcep_inputs(nfft, M, alpha, n_iter, F=70):
    """chi-square spectra lifted off zero (tests/test_gpu_48k_grad.py)"""
    return {"X": gauss(nfft + M, F, nfft // 2 + 1).square() + 0.05}


def mcep_generic(inp, nfft, M, alpha, n_iter, F=70):
    """mcep.py:189-224 as oracle/torch_port.py::mcep states it, for the generic kernel pair asked for by name (DSA_ALGO_GENERIC) at
    its longest spectra: the warping products and the solve through rmm / rsolve, so that the second float64 evaluation reorders the
    sums over the bins"""
    X = inp["X"]
    tab, H = TP.McepTables(nfft, M, alpha, X.dtype), nfft // 2
    log_x = torch.log(X)
    scale = torch.ones(nfft, dtype=X.dtype)
    scale[0] = scale[H] = 0.5
    mc = rmm((torch.fft.irfft(log_x) * scale)[..., :H + 1], tab.A_f)
    for _ in range(n_iter):
        d = torch.fft.rfft(rmm(mc, tab.A_i), n=nfft).real
        rt = rmm(torch.fft.irfft(torch.exp(log_x - d - d))[..., :H + 1], tab.A_r)
        r = rt[..., :M + 1]
        i = torch.arange(M + 1)
        mc = mc + rsolve(r[..., (i[:, None] - i[None, :]).abs()] + rt[..., i[:, None] + i[None, :]], r - tab.av)
    return mc


mcep_generic_inputs = mcep_inputs


def newton_update(inp, n, F=65):
    """mcep.py:216-222: mc + solve(T(rt[:n]) + H(rt), rt[:n] - alpha_vector) (tests/test_gpu_configs.py::test_newton_update_with_a_gradient...)"""
    rt, av = inp["rt"], inp["av"]
    i = torch.arange(n)
    A = rt[:, (i[:, None] - i[None, :]).abs()] + rt[:, i[:, None] + i[None, :]]
    return inp["mc"] + rsolve(A, rt[:, :n] - av)


def newton_update_inputs(n, F=65):
    """rt = the cosine moments of a positive spectrum: the Hessians of the analysis, positive definite"""
    K = 4 * n
    g = torch.Generator().manual_seed(n + F)
    cw = torch.cos(torch.arange(2 * n - 1, dtype=torch.float64)[:, None] * (torch.arange(K, dtype=torch.float64) * (math.pi / K))[None, :])
    e = torch.rand(F, K, generator=g, dtype=torch.float64) + 0.05
    return {"rt": (e @ cw.t()) / K, "av": 0.1 * gauss(n, n), "mc": gauss(n + 1, F, n)}


def glogx(inp, K, n, n_iter, F):
    """sum over the steps of (grt_s E^T) * exp(logx - 2 mc_s D), D and E the module's tables (tests/test_gpu_48k_grad.py)"""
    D, E = inp["D"], inp["E"]
    return sum((inp["grts"][s] @ E.T) * torch.exp(inp["logx"] - 2 * inp["mcs"][s] @ D) for s in range(n_iter))


def glogx_inputs(K, n, n_iter, F):
    import diffsptk_amd as dsp

    m = dsp.MelCepstralAnalysis(fft_length=2 * (K - 1), cep_order=n - 1, alpha=0.55, n_iter=1, dtype=torch.float64)   # (host tables)
    mcs = 0.02 * gauss(K + n, n_iter, F, n)
    mcs[:, :, 0] += 0.3
    return {"logx": 0.7 * gauss(K, F, K), "mcs": mcs, "grts": gauss(K + 1, n_iter, F, 2 * n - 1), "D": m.D.clone(), "E": m.E.clone()}


# ----------------------------------------------------------------------------------------------- csrc/mgc.hip
def gc2gc(inp, g1, g2, n_fft, m1, m2, F=37):
    """mgc2mgc.py:333-361 with torch.fft (tests/test_gpu_synth.py::test_gc2gc_backward_kernel_against_autograd_of_the_definition)"""
    c = inp["c"]
    C1 = torch.fft.fft(torch.cat((torch.zeros_like(c[..., :1]), c[..., 1:]), -1), n=n_fft)
    if g1 == 0:
        mag, ang = torch.exp(C1.real), C1.imag
    else:
        z = 1 + g1 * C1
        mag, ang = z.abs() ** (1 / g1), z.angle() / g1
    if g2 == 0:
        C2 = torch.log(mag)
    else:
        ang = torch.remainder(ang + math.pi, 2 * math.pi) - math.pi
        C2 = (mag ** g2 * torch.cos(ang * g2) - 1) / g2
    return torch.cat((c[..., :1], 2 * torch.fft.ifft(C2).real[..., 1:m2 + 1]), -1)


def gc2gc_inputs(g1, g2, n_fft, m1, m2, F=37):
    return {"c": 0.3 * gauss(n_fft + m1, F, m1 + 1)}


gc2gc_entry, gc2gc_entry_inputs = gc2gc, gc2gc_inputs   # dsa_gc2gc_fwd / _bwd themselves, without the Python layer's own size test


def _mgcep_spectra(x, b1, M, alpha, gamma):
    mats = {k: const(v, x) for k, v in tables.mgcep_matrices(2 * (x.size(-1) - 1), M, alpha).items()}
    b = torch.cat((torch.zeros_like(b1[..., :1]), b1), -1)
    X, Y = 1 + gamma * rmm(b, mats["Cr"]), gamma * rmm(b, mats["Ci"])
    D = X * X + Y * Y
    pp = x * D ** (-1 / gamma) / D
    qq = pp / D
    return mats, (pp, qq * (X * X - Y * Y), qq * (2 * X * Y), pp * X, pp * Y)


def mgcep_spectra(inp, nfft, M, gamma, alpha=0.42, F=9):
    """mgcep.py:199-209: the five spectra of a Newton step, stacked"""
    return torch.stack(_mgcep_spectra(inp["x"], inp["b1"], M, alpha, gamma)[1])


def mgcep_step(inp, nfft, M, gamma, alpha=0.42, F=9):
    """mgcep.py:199-227: (pt, qt, r) of a Newton step -- the spectra against the module's composed matrices"""
    mats, S = _mgcep_spectra(inp["x"], inp["b1"], M, alpha, gamma)
    pt = rmm(S[0], mats["Pr"][:, :M])
    qt = (rmm(S[1], mats["Qr"][:, 2:]) + rmm(S[2], mats["Qi"][:, 2:])) * (1 + gamma)
    return pt, qt, rmm(S[3], mats["Rr"]) + rmm(S[4], mats["Ri"])


def mgcep_step_inputs(nfft, M, gamma, alpha=0.42, F=9):
    """spectra and coefficients of tests/test_gpu_configs.py::test_mgcep_step_adjoint_on_binary16_splits_against_the_float32_kernel"""
    return {"x": gauss(nfft + M, F, nfft // 2 + 1).square() + 0.05, "b1": 0.05 * gauss(M, F, M)}


mgcep_spectra_inputs = mgcep_step_inputs


def mgcep_gain(inp, M, gamma, F=9):
    """mgcep.py:213-215, 221, 231-233: (sqrt(r_0 + gamma sum_m r_{m+1} b_eps_m), b_join)"""
    r = inp["r"]
    return torch.cat((torch.sqrt(r[..., :1] + gamma * rsum(r[..., 1:] * inp["b_eps"]).unsqueeze(-1)), inp["b_join"]), -1)


def mgcep_gain_inputs(M, gamma, F=9):
    r = 0.1 * gauss(M, F, M + 1)
    r[..., 0] += 2.0
    return {"r": r, "b_eps": 0.3 * gauss(M + 1, F, M), "b_join": gauss(M + 2, F, M)}


def fbank_bins(inp, nfft, C, gamma, floor=1e-5, F=7):
    """the filter bank on linear-domain values s (the fused STFT -> filter bank feeds it power values): glog(max(s H, floor))"""
    return fbank({"x": inp["s"]}, nfft, C, True, gamma, floor)[0]


def fbank_bins_inputs(nfft, C, gamma, floor=1e-5, F=7):
    return {"s": fbank_inputs(nfft, C, True, gamma, floor, F)["x"]}


def mcep_tuned(inp, n_iter, keep_rt=True):
    return TP.mcep(inp["X"], TP.McepTables(512, 24, 0.42, inp["X"].dtype), n_iter)


def mcep_tuned_inputs(n_iter, keep_rt=True):
    """the power spectrogram of white noise (tests/test_gpu_configs.py::test_mcep_backward_two_waves_per_simd_...): 2 x 60 frames"""
    return {"X": TP.stft_power(gauss(33, 2, 4800), 400, 80, 512).reshape(-1, 257)}


# ----------------------------------------------------------------------------------------------- csrc/mlsacheck.hip
def _mlsa_parts(mc, alpha, mode, n_fft):
    """(gain, gain-free cepstrum, amplitudes (the plain sum as one column in fast mode), Cr, Ci) -- tests/test_gpu_mlsacheck.py::re_amplitudes"""
    M = mc.size(-1) - 1
    gain = rsum(mc * const((-float(alpha)) ** np.arange(M + 1), mc)).unsqueeze(-1)
    c = torch.cat((mc[..., :1] - gain, mc[..., 1:]), -1)
    if mode == "fast":
        return gain, c, rsum(c).unsqueeze(-1), None, None
    K = n_fft // 2 + 1
    ang = 2 * math.pi * ((torch.arange(K)[:, None] * torch.arange(M + 1)[None]) % n_fft).double() / n_fft
    Cr, Ci = rmm(c, torch.cos(ang).T.to(c.dtype)), -rmm(c, torch.sin(ang).T.to(c.dtype))
    A2 = Cr * Cr + Ci * Ci
    A = torch.where(A2 > 0, torch.sqrt(torch.where(A2 > 0, A2, torch.ones_like(A2))), torch.zeros_like(A2))
    return gain, c, A, Cr, Ci


def mlsacheck(inp, M, mode, n_fft, F=3, alpha=0.42, thr=4.5):
    """mlsacheck.py of the reference (tests/test_gpu_mlsacheck.py::re_mlsacheck): the gain-free cepstrum scaled ("fast", "scale") or
    its spectrum clipped bin by bin ("clip") down to the threshold, then the gain put back"""
    mc = inp["mc"]
    gain, c, A, Cr, Ci = _mlsa_parts(mc, alpha, mode, n_fft)
    a = A.amax(-1, keepdim=True).clamp(min=1e-16)
    if mode == "fast":
        out = (thr / a).clamp(max=1) * c
    else:
        K = n_fft // 2 + 1
        N2 = 2 * (K - 1)
        s = (thr / a).clamp(max=1) if mode == "scale" else torch.where(A > 0, thr / torch.where(A > 0, A, torch.ones_like(A)), torch.ones_like(A)).clamp(max=1)
        w = torch.full((K,), 2.0, dtype=mc.dtype)
        w[0] = w[K - 1] = 1.0
        ang = 2 * math.pi * ((torch.arange(K)[:, None] * torch.arange(M + 1)[None]) % N2).double() / N2
        Ci = torch.cat((torch.zeros_like(Ci[..., :1]), Ci[..., 1:K - 1], torch.zeros_like(Ci[..., :1])), -1)   # ignored by the inverse
        # (the sums over the bins through rsum, not rmm: up to 9 000 terms, and what a float32 matrix product loses on them depends on the
        # host's blocking, eightfold between two machines -- a sum's own cascade does not)
        out = rsum((w * s * Cr).unsqueeze(-2) * torch.cos(ang).T.to(mc.dtype) - (w * s * Ci).unsqueeze(-2) * torch.sin(ang).T.to(mc.dtype)) / N2
    return torch.cat((out[..., :1] + gain, out[..., 1:]), -1)


def mlsacheck_inputs(M, mode, n_fft, F=3, alpha=0.42, thr=4.5):
    """rows of tests/test_gpu_mlsacheck.py::rough_mc, exact in float32: the first row's amplitude is twice the threshold (the check
    moves it), the others' half of it (they pass through)"""
    x = 0.5 * gauss(M + n_fft, F, M + 1) * torch.linspace(1, 0.05, M + 1, dtype=torch.float64)
    A = _mlsa_parts(x, alpha, mode, n_fft)[2]
    a = A[:, 0] if mode == "fast" else A.amax(-1)
    want = torch.where(torch.arange(F) == 0, 2.0, 0.5).double() * thr
    return {"mc": (x * (want / a)[:, None]).float().double()}


# ----------------------------------------------------------------------------------------------- csrc/mdct.hip
def mdct(inp, L, T, B=2):
    """mdct.py of the reference with the sine window (tests/mdct_ref.py::analysis): y[n, k] = sum_j w[j] x[(n - 1) P + j] C[j, k]"""
    import mdct_ref as MR

    x = inp["x"]
    P = L // 2
    N = (T + P - 1) // P + 1
    xp = torch.cat([torch.zeros(B, P, dtype=x.dtype), x, torch.zeros(B, N * P - T, dtype=x.dtype)], -1)
    fr = xp[:, torch.arange(N)[:, None] * P + torch.arange(L)[None, :]] * const(MR.window_of(L, "sine"), x)
    return rmm(fr, const(MR.basis(L, "sine", "cosine"), x))


def mdct_inputs(L, T, B=2):
    return {"x": gauss(L + T, B, T)}


def imdct(inp, L, N, B=2):
    """imdct.py of the reference (tests/mdct_ref.py::synthesis): overlap-add of w (y C^T), halved where two frames overlap"""
    import mdct_ref as MR

    y = inp["y"]
    P = L // 2
    T = (N - 1) * P
    v = rmm(y, const(MR.basis(L, "sine", "cosine"), y).T) * const(MR.window_of(L, "sine"), y)
    o = torch.zeros(B, (N + 1) * P, dtype=y.dtype)
    for n in range(N):
        o = o + TF.pad(v[:, n], (n * P, (N + 1) * P - n * P - L))
    return o[:, P:P + T] * const(MR.overlap_scale(N, P, T), y)


def imdct_inputs(L, N, B=2):
    return {"y": gauss(L + N, B, N, L // 2)}


NAMES = ("acorr", "levdur", "lpc", "fwlpc", "zerodf", "fftr", "spec", "stft", "irfft_scale", "thsolve", "freqt", "rows_log", "rows_expsub",
         "fftcep", "fbank", "stft_fbank", "pqmf", "ipqmf", "interpolate", "delta", "mlpg", "plp_tail", "poledf", "mcep", "newton_update",
         "glogx", "gc2gc", "mgcep_spectra", "mgcep_step", "mgcep_gain", "mdct", "imdct", "fbank_bins", "mcep_tuned", "fuse_fwlpc", "mfcc",
         "mcep_generic", "gc2gc_entry", "mlsacheck")
REFS = {name: globals()[name] for name in NAMES}
INPUTS = {name: globals()[name + "_inputs"] for name in NAMES}


# ----------------------------------------------------------------------------------------------- what a case compares, and its base values
def cotangents(outs, dtype):
    """the stored Gaussian cotangent of every output"""
    return [gauss(4321 + i, *o.shape).to(dtype) for i, o in enumerate(outs)]


def inputs_of(c, dtype):
    """the case's inputs as the kernel gets them: rounded to its dtype"""
    return {k: v.to(dtype) for k, v in INPUTS[c["call"]](**c["args"]).items()}


def evaluate(c, inputs):
    """the tensors the case compares, from the restatement in the inputs' dtype: the outputs ("fwd"), or the gradients of
    sum(output * cotangent) with respect to the inputs named by `wrt` ("bwd")"""
    leaves = {k: v.detach().clone().requires_grad_(k in c["wrt"]) for k, v in inputs.items()}
    out = REFS[c["call"]](leaves, **c["args"])
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    if c["when"] == "fwd":
        return [o.detach() for o in outs]
    dtype = outs[0].dtype
    loss = sum((o * g).sum() for o, g in zip(outs, cotangents(outs, dtype)))
    return list(torch.autograd.grad(loss, [leaves[k] for k in c["wrt"]]))


def error(got, ref, metric):
    """the largest |got - ref| relative to the largest |ref| of the tensor ("max") or of each row ("rows")"""
    got, ref = got.double(), ref.double()
    if ref.numel() == 0:
        return 0.0
    scale = ref.abs().amax(-1, keepdim=True) if metric == "rows" else ref.abs().max()
    return float(((got - ref).abs() / scale.clamp_min(1e-300)).max())


def bases(c):
    """(base64, base32) of a case: the second float64 evaluation (reversed accumulation) and the float32 evaluation against the first"""
    out = []
    for dt in ("f64", "f32"):
        if dt not in c["dtypes"]:
            out.append(0.0)
            continue
        given = inputs_of(c, torch.float64 if dt == "f64" else torch.float32)
        ref = evaluate(c, {k: v.double() for k, v in given.items()})
        if dt == "f64":
            with reversed_order():
                other = evaluate(c, given)
        else:
            other = evaluate(c, given)
        out.append(max(error(o, r, c["metric"]) for o, r in zip(other, ref)))
    return tuple(out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import kernel_routes as KR

    for route, c in KR.all_cases():   # (ROUTES, then both sides of CEILINGS; with any argument: only the cases MEASURED does not have yet)
        if c["tol_from"] == KR.MEAS and (len(sys.argv) < 2 or KR.case_id(route, c) not in KR.MEASURED):
            b64, b32 = bases(c)
            print(f'    "{KR.case_id(route, c)}": ({b64:.2e}, {b32:.2e}),', flush=True)
