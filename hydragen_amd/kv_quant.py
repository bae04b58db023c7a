"""
fp8 (OCP e4m3fn) unique K/V caches: the quantizer every kernel matches.

A unique (per-sequence) cache may hold `torch.float8_e4m3fn` values with one fp32 scale per kv head, separately for K and V
(`k_scale`, `v_scale`: [Hkv], None = 1).  The stored value is x / scale[h], clamped to the format's largest finite value
(+-448) and rounded to nearest, ties to even.  The clamp is part of the definition: a plain `.to(torch.float8_e4m3fn)`
turns values of 464 and more into NaN.  NaN stays NaN.

q, outputs, partials and the shared-prefix caches stay 16-bit.  Every e4m3fn value is exactly a bf16 and an f16 value, so the
kernels widen the bytes without rounding: quantizing is the only new rounding of the operator.
"""

from __future__ import annotations

import torch
from torch import Tensor

FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0


def _per_head(scale: Tensor, x: Tensor) -> Tensor:
    """[Hkv] scale -> broadcastable against [..., Hkv, D]."""
    h = x.shape[-2]
    if scale.numel() != h:
        raise ValueError(f"scale has {scale.numel()} entries for {h} kv heads")
    return scale.to(device=x.device, dtype=torch.float32).reshape(h, 1)


def quantize_kv(x: Tensor, scale: Tensor | None = None) -> Tensor:
    """x [..., Hkv, D] (any float dtype) -> float8_e4m3fn: (x.float() / scale[h]).clamp(-448, 448), round-half-even."""
    xf = x.float()
    if scale is not None:
        xf = xf / _per_head(scale, x)
    return xf.clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)


def dequantize_kv(x8: Tensor, scale: Tensor | None, dtype: torch.dtype) -> Tensor:
    """The inverse of quantize_kv: x8.float() * scale[h], rounded to `dtype` (exact for scale None / 1 and a 16-bit dtype)."""
    if x8.dtype != FP8_DTYPE:
        raise TypeError(f"dequantize_kv takes {FP8_DTYPE}, got {x8.dtype}")
    xf = x8.float()
    if scale is not None:
        xf = xf * _per_head(scale, x8)
    return xf.to(dtype)


def is_fp8(t: Tensor) -> bool:
    return t.dtype == FP8_DTYPE
