"""Inverse modified discrete cosine / sine transform (reference: imdct.py): the transform back, windowing and the overlap-add divided by
the number of frames over each sample, in one launch (csrc/mdct.hip) that writes every output sample once.

learnable=True or a list builds the reference's cascade instead -- the row product with the basis Parameter, a learnable Window and
Unframe -- on stock device operators (modules/mdct.py); its state_dict keys are the reference's ("imdt.W", "window.window").

The classes are exported from the package root and through functional.imdct / imdst, not from diffsptk_amd.modules, for the reason
given in modules/mlsacheck.py."""
from __future__ import annotations

import torch

from .. import ops
from ..utils import tables
from ..utils.private import check_size, filter_values, get_layer, to
from .base import BaseFunctionalModule, Precomputed
from .mdct import ModifiedDiscreteCosineTransform, ModifiedDiscreteTransform, _kernel_tables, _learnable_keys
from .unframe import Unframe
from .window import Window


class InverseModifiedDiscreteCosineTransform(BaseFunctionalModule):
    """y:(..., N, L/2) -> (..., (N - 1) L/2), or min(out_length, N L/2) samples (imdct.py:169-181).  The options of
    ModifiedDiscreteCosineTransform."""

    def __init__(self, frame_length: int, window: str = "sine", learnable: bool | list[str] = False,
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, y: torch.Tensor, out_length: int | None = None) -> torch.Tensor:
        return self._call_forward(y, out_length)

    @staticmethod
    def _func(y: torch.Tensor, out_length: int | None, *args, **kwargs) -> torch.Tensor:
        pre = InverseModifiedDiscreteCosineTransform._precompute(*args, **kwargs, device=y.device, dtype=y.dtype, module=False)
        return InverseModifiedDiscreteCosineTransform._apply_precomputed(pre, y=y, out_length=out_length)

    @staticmethod
    def _check(*args, **kwargs) -> None:
        ModifiedDiscreteCosineTransform._check(*args, **kwargs)

    @staticmethod
    def _precompute(frame_length: int, window: str, learnable: bool | list[str] = False, device: torch.device | None = None,
                    dtype: torch.dtype | None = None, transform: str = "cosine", module: bool = True) -> Precomputed:
        InverseModifiedDiscreteCosineTransform._check(learnable)
        keys = _learnable_keys(learnable)
        values = {"frame_period": frame_length // 2, "transform": transform}
        if not keys:
            kernel = _kernel_tables(frame_length, window, transform, device, dtype, inverse=True)
            return Precomputed(values={**values, "scale": kernel.pop("scale")}, tensors=kernel)
        imdt = get_layer(module, InverseModifiedDiscreteTransform, dict(length=frame_length, window=window, transform=transform,
                                                                        learnable="basis" in keys, device=device, dtype=dtype))
        window_ = get_layer(module, Window, dict(in_length=frame_length, out_length=None, window=window, norm="none", symmetric=True,
                                                 learnable="window" in keys, device=device, dtype=dtype))
        unframe = get_layer(module, Unframe, dict(frame_length=frame_length, frame_period=frame_length // 2, device=device, dtype=dtype))
        return Precomputed(values=values, layers={"imdt": imdt, "window": window_, "unframe": unframe})

    @staticmethod
    def _forward(y: torch.Tensor, out_length: int | None, *, frame_period: int, transform: str, scale: float | None = None, w: torch.Tensor | None = None,
                 table_a: torch.Tensor | None = None, table_s: torch.Tensor | None = None, imdt=None, window=None,
                 unframe=None) -> torch.Tensor:
        if imdt is not None:   # the learnable cascade (imdct.py:178-181)
            x = unframe(window(imdt(y)), out_length=out_length)
            return x[..., :-frame_period] if out_length is None else x
        check_size(y.size(-1), frame_period, "dimension of input")   # the reference's checks in its order: imdct.py:243, unframe.py:174
        if y.dim() <= 1:
            raise ValueError("Input must be at least 2D tensor.")
        return ops.ImdctFn.apply(y, out_length, w, table_a, table_s, scale, transform)


class InverseModifiedDiscreteSineTransform(BaseFunctionalModule):
    """The sine twin of InverseModifiedDiscreteCosineTransform (imdst.py:96-110)."""

    def __init__(self, frame_length: int, window: str = "sine", learnable: bool | list[str] = False,
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self._register_precomputed(self._precompute(**filter_values(locals())))

    def forward(self, y: torch.Tensor, out_length: int | None = None) -> torch.Tensor:
        return self._call_forward(y, out_length)

    @staticmethod
    def _func(*args, **kwargs) -> torch.Tensor:
        return InverseModifiedDiscreteCosineTransform._func(*args, **kwargs, transform="sine")

    @staticmethod
    def _check(*args, **kwargs) -> None:
        raise NotImplementedError

    @staticmethod
    def _precompute(*args, **kwargs) -> Precomputed:
        return InverseModifiedDiscreteCosineTransform._precompute(*args, **kwargs, transform="sine")

    @staticmethod
    def _forward(*args, **kwargs) -> torch.Tensor:
        return InverseModifiedDiscreteCosineTransform._forward(*args, **kwargs)


class InverseModifiedDiscreteTransform(BaseFunctionalModule):
    """y:(..., L/2) -> (..., L) = y @ W^T, W the basis of ModifiedDiscreteTransform (imdct.py:262-268); learnable: W^T is a Parameter."""

    _takes_input_size = True

    def __init__(self, length: int, window: str, transform: str = "cosine", learnable: bool = False,
                 device: torch.device | None = None, dtype: torch.dtype | None = None) -> None:
        super().__init__()
        self.in_dim = length // 2
        self._register_precomputed(self._precompute(**filter_values(locals(), drop_keys=["learnable"])), learnable=learnable)

    def forward(self, y: torch.Tensor) -> torch.Tensor:
        check_size(y.size(-1), self.in_dim, "dimension of input")
        return self._call_forward(y)

    @staticmethod
    def _func(y: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        pre = InverseModifiedDiscreteTransform._precompute(2 * y.size(-1), *args, **kwargs, device=y.device, dtype=y.dtype)
        return InverseModifiedDiscreteTransform._apply_precomputed(pre, y=y)

    @staticmethod
    def _check(*args, **kwargs) -> None:
        raise NotImplementedError

    @staticmethod
    def _precompute(length: int, window: str, transform: str, device: torch.device | None, dtype: torch.dtype | None) -> Precomputed:
        ModifiedDiscreteTransform._check(length)
        return Precomputed(tensors={"W": to(tables.mdct_basis(length, window, transform).T, device=device, dtype=dtype)})

    @staticmethod
    def _forward(y: torch.Tensor, *, W: torch.Tensor) -> torch.Tensor:
        if W.requires_grad:
            return torch.matmul(y, W)
        return ops.MatmulRowsFn.apply(y, W)
