"""Modified discrete cosine / sine transform (reference: mdct.py): framing at half overlap, windowing and the transform in one launch
(csrc/mdct.hip) -- window, time-domain aliasing, a DCT-IV through a quarter-length complex FFT for float32 power-of-two frame lengths,
the plain sums against the basis table otherwise.

learnable=True or a list builds the reference's cascade of sub-modules instead -- Frame, a learnable Window and the row product with the
basis Parameter -- on stock device operators (the policy of modules/_learnable.py): the kernels treat their tables as constants.  Its
state_dict keys are the reference's ("window.window", "mdt.W").

The classes are exported from the package root and through functional.mdct / mdst, not from diffsptk_amd.modules, for the reason given
in modules/mlsacheck.py."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from ..utils import tables
from ..utils.private import check_size, filter_values, get_layer, to
from .base import BaseFunctionalModule, Precomputed
from .frame import Frame
from .window import Window

LEARNABLES = ("basis", "window")


def _learnable_keys(learnable) -> tuple:
    return LEARNABLES if learnable is True else () if learnable is False else tuple(learnable)


def _kernel_tables(frame_length: int, window: str, transform: str, device, dtype, inverse: bool = False) -> dict:
    """What MdctFn / ImdctFn read: the window, and per direction the twiddles (fast kernels) or the basis and its transpose.  The checks
    are those of the reference's sub-modules in the order it builds them: Frame, Window, the transform; the transform first when inverse."""
    if inverse:
        ModifiedDiscreteTransform._check(frame_length)
    else:
        Frame._check(frame_length, frame_length // 2)
    w = tables.window_table(frame_length, window, "none", True)
    ModifiedDiscreteTransform._check(frame_length)
    if transform not in ("cosine", "sine"):
        raise ValueError(f"transform must be either 'cosine' or 'sine'. Got '{transform}'.")
    dtype = torch.get_default_dtype() if dtype is None else dtype
    w = to(w, device=device, dtype=dtype)
    if ops.mdct_fast_supported(frame_length, dtype):
        table_a = table_s = to(tables.mdct_twiddle(frame_length), device=device, dtype=dtype)
    else:
        C = tables.mdct_basis(frame_length, window, transform)
        table_a, table_s = to(C, device=device, dtype=dtype), to(C.T, device=device, dtype=dtype)
    return {"w": w, "table_a": table_a, "table_s": table_s, "scale": tables.mdct_scale(frame_length, window)}


class ModifiedDiscreteCosineTransform(BaseFunctionalModule):
    """x:(..., T) -> (..., N, L/2), N = (T + L/2 - 1) // (L/2) + 1 (mdct.py:166-176).  window: "sine", "vorbis", "kbd" or "rectangular"
    (any window of Window is accepted, as in the reference); learnable: bool, or a list of "basis" and "window"."""

    def __init__(self, frame_length: int, window: str = "sine", learnable: bool | list[str] = False,
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = ModifiedDiscreteCosineTransform._precompute(*args, **kwargs, device=x.device, dtype=x.dtype, module=False)
        return ModifiedDiscreteCosineTransform._apply_precomputed(pre, x=x)

    @staticmethod
    def _check(learnable: bool | list[str]) -> None:
        if isinstance(learnable, (tuple, list)):
            if any(x not in LEARNABLES for x in learnable):
                raise ValueError("An unsupported key is found in learnable.")
        elif not isinstance(learnable, bool):
            raise ValueError("learnable must be boolean or list.")

    @staticmethod
    def _precompute(frame_length: int, window: str, learnable: bool | list[str] = False, device: torch.device | None = None,
                    dtype: torch.dtype | None = None, transform: str = "cosine", module: bool = True) -> Precomputed:
        ModifiedDiscreteCosineTransform._check(learnable)
        keys = _learnable_keys(learnable)
        values = {"frame_period": frame_length // 2, "transform": transform}
        if not keys:
            kernel = _kernel_tables(frame_length, window, transform, device, dtype)
            return Precomputed(values={**values, "scale": kernel.pop("scale")}, tensors=kernel)
        frame = get_layer(module, Frame, dict(frame_length=frame_length, frame_period=frame_length // 2))
        window_ = get_layer(module, Window, dict(in_length=frame_length, out_length=None, window=window, norm="none", symmetric=True,
                                                 learnable="window" in keys, device=device, dtype=dtype))
        mdt = get_layer(module, ModifiedDiscreteTransform, dict(length=frame_length, window=window, transform=transform,
                                                                learnable="basis" in keys, device=device, dtype=dtype))
        return Precomputed(values=values, layers={"frame": frame, "window": window_, "mdt": mdt})

    @staticmethod
    def _forward(x: torch.Tensor, *, frame_period: int, transform: str, scale: float | None = None, w: torch.Tensor | None = None,
                 table_a: torch.Tensor | None = None, table_s: torch.Tensor | None = None, frame=None, window=None, mdt=None) -> torch.Tensor:
        if mdt is not None:   # the learnable cascade (mdct.py:174-176; the padding is for perfect reconstruction)
            return mdt(window(frame(F.pad(x, (0, frame_period)))))
        return ops.MdctFn.apply(x, w, table_a, table_s, scale, transform)


class ModifiedDiscreteSineTransform(BaseFunctionalModule):
    """The sine twin of ModifiedDiscreteCosineTransform (mdst.py:93-107): the same launch with the sine basis."""

    def __init__(self, frame_length: int, window: str = "sine", learnable: bool | list[str] = False,
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._call_forward(x)

    @staticmethod
    def _func(*args, **kwargs) -> torch.Tensor:
        return ModifiedDiscreteCosineTransform._func(*args, **kwargs, transform="sine")

    @staticmethod
    def _check(*args, **kwargs) -> None:
        raise NotImplementedError

    @staticmethod
    def _precompute(*args, **kwargs) -> Precomputed:
        return ModifiedDiscreteCosineTransform._precompute(*args, **kwargs, transform="sine")

    @staticmethod
    def _forward(*args, **kwargs) -> torch.Tensor:
        return ModifiedDiscreteCosineTransform._forward(*args, **kwargs)


class ModifiedDiscreteTransform(BaseFunctionalModule):
    """x:(..., L) -> (..., L/2) = x @ W, W the oddly stacked cosine / sine basis of mdct.py:253-285; learnable: W is a Parameter."""

    _takes_input_size = True

    def __init__(self, length: int, window: str, transform: str = "cosine", learnable: bool = False,
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self.in_dim = length
        self._register_precomputed(self._precompute(**filter_values(locals(), drop_keys=["learnable"])), learnable=learnable)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        check_size(x.size(-1), self.in_dim, "dimension of input")
        return self._call_forward(x)

    @staticmethod
    def _func(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = ModifiedDiscreteTransform._precompute(x.size(-1), *args, **kwargs, device=x.device, dtype=x.dtype)
        return ModifiedDiscreteTransform._apply_precomputed(pre, x=x)

    @staticmethod
    def _check(length: int) -> None:
        if length < 2 or length % 2 == 1:
            raise ValueError("length must be at least 2 and even.")

    @staticmethod
    def _precompute(length: int, window: str, transform: str, device: torch.device | None, dtype: torch.dtype | None) -> Precomputed:
        ModifiedDiscreteTransform._check(length)
        return Precomputed(tensors={"W": to(tables.mdct_basis(length, window, transform), device=device, dtype=dtype)})

    @staticmethod
    def _forward(x: torch.Tensor, *, W: torch.Tensor) -> torch.Tensor:
        if W.requires_grad:   # a learnable basis: autograd's product gives its gradient (modules/_learnable.py)
            return torch.matmul(x, W)
        return ops.MatmulRowsFn.apply(x, W)
