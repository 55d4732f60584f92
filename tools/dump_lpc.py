"""Outputs of the LPC units on fixed inputs, one .npy per output, for a byte-for-byte comparison of two builds of the library
(one process per library; profiles/lpc_split_bench.txt):    python tools/dump_lpc.py OUT_DIR

The cases are the smallest shapes that reach every branch of the code csrc/lpc24.h shares between the tuned forward and backward
kernels: interior and edge fetches, frame_length at compile time (400) and at run time, its extremes (25, 512), odd frame counts (a
two-frame round whose second frame is a repeat, a partial four-frame pass), both lag-sum routes; and the generic kernels."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp
from diffsptk_amd import ops, _lib

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
dev = "cuda"
gen = torch.Generator().manual_seed(20)   # tensors from the CPU generator: the same bits whatever the device library does


def rand(*shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen, dtype=dtype).to(dev)


def save(name, t):
    np.save(os.path.join(out_dir, name + ".npy"), t.detach().cpu().numpy())
    # (the dispatch record is per thread and autograd runs a backward on its own: only a forward's kernel can be named here)
    print("%-44s %-34s %s" % (name, "" if name.endswith("_bwd") else _lib.last_kernel(), tuple(t.shape)))


# fuse(frame, window, lpc), forward and backward, both lag-sum routes
for L, P, T, B, center in ((400, 80, 1234, 3, True), (400, 160, 4001, 2, True), (25, 7, 300, 2, False), (512, 512, 2048, 2, False)):
    x, g = rand(B, T), None
    for exact in (False, True):
        fl = dsp.fuse(dsp.Frame(L, P, center=center), dsp.Window(L, device=dev), dsp.LPC(L, 24, eps=1e-5, device=dev), exact_lag_sums=exact)
        tag = "fused_L%d_P%d_T%d_%s" % (L, P, T, "exact" if exact else "mfma")
        xg = x.detach().requires_grad_(True)
        y = fl(xg)
        assert fl.last_path == "fused", fl.last_path
        save(tag + "_fwd", y)
        g = rand(*y.shape) if g is None else g
        (gx,) = torch.autograd.grad(y, xg, g)
        save(tag + "_bwd", gx)
# the forward's edge fetch in every padding mode
x, w = rand(3, 1234), dsp.Window(400, device=dev).window
for mode in ("constant", "reflect", "replicate", "circular"):
    for exact in (False, True):
        with torch.no_grad():
            save("fwd_pad_%s_%s" % (mode, "exact" if exact else "mfma"), ops.frame_window_lpc(x, w, 400, 80, 24, 1e-5, True, mode, exact))
# framed rows, an odd count of them: dsa_lpc_fwd / dsa_lpc_bwd
xr = rand(67, 400).requires_grad_(True)
a = ops.LpcFn.apply(xr, 24, 1e-5)
save("rows67_fwd", a)
(gxr,) = torch.autograd.grad(a, xr, rand(67, 25))
save("rows67_bwd", gxr)
# the generic path: float64, order 10
xd = rand(5, 64, dtype=torch.float64).requires_grad_(True)
ad = dsp.LPC(64, 10, eps=1e-5, dtype=torch.float64, device=dev)(xd)
save("generic_f64_fwd", ad)
(gxd,) = torch.autograd.grad(ad, xd, rand(5, 11, dtype=torch.float64))
save("generic_f64_bwd", gxd)
torch.cuda.synchronize()
