"""Launch time of the fused Frame + Window + LPC kernel at the bench size (1024 utterances x 1 s, 204 800 frames)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffsptk_amd as dsp
from diffsptk_amd import ops, _lib
dev = "cuda"
x = torch.randn(1024, 16000, device=dev)
w = dsp.Window(400, device=dev).window
with torch.no_grad():
    for _ in range(5):
        y = ops.frame_window_lpc(x, w, 400, 80, 24, 1e-5)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            y = ops.frame_window_lpc(x, w, 400, 80, 24, 1e-5)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 20)
    k_default = _lib.last_kernel()
    te = []   # the exact route: float64 lag sums on the vector unit
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            y = ops.frame_window_lpc(x, w, 400, 80, 24, 1e-5, exact_lag_sums=True)
        b.record()
        torch.cuda.synchronize()
        te.append(a.elapsed_time(b) / 20)
    k_exact = _lib.last_kernel()
print(k_exact, "(exact_lag_sums) ms per launch:", " ".join(f"{t:.4f}" for t in te))
print(k_default, "ms per launch:", " ".join(f"{t:.4f}" for t in ts))
