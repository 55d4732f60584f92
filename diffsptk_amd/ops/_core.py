"""Shared by every family: argument checks, raw pointers, the current stream, the status-checked call, the kernels' scratch."""
from __future__ import annotations

import torch

from .. import _lib

_PAD = {"constant": _lib.PAD_CONSTANT, "reflect": _lib.PAD_REFLECT, "replicate": _lib.PAD_REPLICATE, "circular": _lib.PAD_CIRCULAR}


def pad_mode_code(mode: str) -> int:
    try:
        return _PAD[mode]
    except KeyError:
        raise ValueError(f"mode {mode} is not supported.") from None


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.float64:
        return _lib.F64
    raise TypeError(f"diffsptk_amd supports float32/float64 tensors, got {t.dtype}")


def _require_device(*tensors) -> None:
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError(
                "diffsptk_amd is a HIP (MI355X) device backend: expected tensors on a 'cuda' "
                f"(ROCm) device, got {t.device}.  There is no CPU fallback."
            )


def _same_dtype(ref: torch.Tensor, *others) -> None:
    for t in others:
        if t is not None and t.dtype != ref.dtype:
            raise RuntimeError(f"expected scalar type {ref.dtype} but found {t.dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _call(name, *args):
    lib = _lib.load()
    _lib.check(getattr(lib, name)(*args), name)


def num_frames(T: int, P: int) -> int:
    return 0 if T <= 0 else (T - 1) // P + 1


def _scratch(device) -> torch.Tensor:
    """DSA_SCRATCH_BYTES of per-call workspace for the persistent tuned kernels (include/diffsptk_amd.h,
    Conventions): a fresh block from PyTorch's stream-ordered caching allocator, so calls that can overlap in
    time (other streams) never share one -- the library itself owns no device memory."""
    return torch.empty(_lib.SCRATCH_BYTES, dtype=torch.uint8, device=device)


_CLEAN_SCRATCH: dict = {}   # (device index, stream handle) -> a zeroed scratch the mel-cepstral forward keeps clean


def _clean_scratch(device) -> torch.Tensor:
    """A scratch that is zero on entry and left zero by the kernel (DSA_ALGO_SCRATCH_IS_CLEAN): one per (device, stream), so
    calls on one stream -- which cannot overlap -- share it and calls on different streams never do."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    t = _CLEAN_SCRATCH.get(key)
    if t is None:
        t = torch.zeros(_lib.SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        _CLEAN_SCRATCH[key] = t
    return t


def _mcep_scratch(device):
    """(scratch, clean) of a tuned persistent launch: the per-(device, stream) kept-zero counters (clean = True: no fill launch per
    call) -- except while a HIP graph is being captured: a graph replays on whatever stream is current, possibly next to an eager
    call that uses the capture stream's counters, so a captured launch gets its own block and the library's reset (a captured
    memset node) instead."""
    with torch.cuda.device(device):
        if torch.cuda.is_current_stream_capturing():
            return _scratch(device), False
        return _clean_scratch(device), True
