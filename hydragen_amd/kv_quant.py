"""
fp8 (OCP e4m3fn) unique K/V caches: the quantizer every kernel matches.

A unique (per-sequence) cache may hold `torch.float8_e4m3fn` values with one fp32 scale per kv head, separately for K and V
(`k_scale`, `v_scale`: [Hkv], None = 1).  The stored value is x / scale[h], clamped to the format's largest finite value
(+-448) and rounded to nearest, ties to even.  The clamp is part of the definition: a plain `.to(torch.float8_e4m3fn)`
turns values of 464 and more into NaN.  NaN stays NaN.

q, outputs, partials and the shared-prefix caches stay 16-bit.  Every e4m3fn value is exactly a bf16 and an f16 value, so the
kernels widen the bytes without rounding: quantizing is the only new rounding of the operator.

Calibration: the scales come from the K / V the prefill computes in 16 bits before any fp8 byte is written.  `observe_absmax`
folds max |x| per kv head into a running buffer amax f32 [2, Hkv] (K row, V row; hyd_kv_absmax), `scales_from_absmax` turns it
into scale[h] = the smallest power of two >= amax[h] * margin / 448 (hyd_kv_scales_from_absmax), so that the largest observed
magnitude lands at 448 / margin or, by the rounding up, as low as half of that: the margin is the headroom of values that were
not observed (generated tokens).  Power-of-two scales keep every dequantized value exactly a bf16 / f16 value, and rescaling K or
V by a power of two changes the scale by exactly that power and no stored byte.  `absmax_reference` and
`scales_from_absmax_reference` are the definitions in torch; the kernels match them bit for bit.

What calibration fixes is RANGE: e4m3 with scale 1 saturates at 448, is subnormal below 2^-6 and flushes to zero below 2^-10, so a
head whose V has std 2e-3 or 3000 loses most of its values (relative L2 of float64 attention, B 4 x S 64 x H 4 x D 128: 2.8e-1 and
8.8e-1 with scale 1, 3.8e-2 and 3.7e-2 calibrated; unit-normal inputs 3.5e-2 either way).  What it does not fix is MANTISSA: the
three mantissa bits give every stored value a relative error of up to 2^-4 whatever the scale, and a large K turns that into a
large absolute error of the scores (K std 40: 9e-2 ... 2.7e-1 depending on the sample, with scale 1 and calibrated alike).  Values beyond the margin are clamped
by the quantizer, as they are with scale 1.
"""

from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _lib

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


# ---- calibration: per-kv-head scales from observed 16-bit K / V ---------------------------------------------------------------
SCALE_MIN_EXP, SCALE_MAX_EXP = -100, 100  # scales are clamped to [2^-100, 2^100]


def scale_constant(margin: float = 2.0) -> float:
    """c = float32(margin / 448): the constant both routes multiply amax by (computed once, in double, rounded to fp32)."""
    margin = float(margin)
    c = torch.tensor(margin / FP8_MAX, dtype=torch.float64).to(torch.float32).item()
    if not (margin > 0 and 0 < c < float("inf")):
        raise ValueError(f"margin {margin} must be finite and positive (and margin / 448 a positive fp32 number)")
    return c


def _check_observed(k, v, amax, row_lens):
    """Shapes and dtypes both routes refuse.  -> (reference tensor, Hkv)."""
    x = k if k is not None else v
    if x is None:
        raise ValueError("observe K, V or both: k and v are both None")
    for name, t in (("k", k), ("v", v)):
        if t is None:
            continue
        if t.ndim not in (3, 4) or t.shape != x.shape or t.dtype != x.dtype:
            raise ValueError(f"k / v must be [rows, Hkv, d] or [outer, rows, Hkv, d] views of one shape and dtype, got {name} "
                             f"{tuple(t.shape)} {t.dtype} against {tuple(x.shape)} {x.dtype}")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"observed dtype {x.dtype}: float16 / bfloat16 (fp8 sources are not taken)")
    Hkv, d = x.shape[-2], x.shape[-1]
    if d % 8 or not 8 <= d <= 256:
        raise ValueError(f"head dim {d} must be a multiple of 8 in 8..256")
    if amax.dtype != torch.float32 or tuple(amax.shape) != (2, Hkv) or not amax.is_contiguous():
        raise ValueError(f"amax must be a contiguous float32 [2, {Hkv}] buffer, got {tuple(amax.shape)} {amax.dtype}")
    if row_lens is not None:
        n_outer = x.shape[0] if x.ndim == 4 else 1
        if row_lens.ndim != 1 or row_lens.numel() != n_outer or row_lens.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"row_lens must be an int32 / int64 [{n_outer}] vector, got {tuple(row_lens.shape)} {row_lens.dtype}")
    return x, Hkv


def _absmax_one(x: Tensor, row_lens) -> Tensor:
    """[Hkv] f32: max |x| over the finite elements of the rows inside their lengths (0 where there is none)."""
    x4 = x if x.ndim == 4 else x.unsqueeze(0)
    a = x4.float().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    if row_lens is not None:
        lens = row_lens.to(device=x.device, dtype=torch.int64).clamp(0, x4.shape[1])
        inside = torch.arange(x4.shape[1], device=x.device)[None, :] < lens[:, None]
        a = torch.where(inside[:, :, None, None], a, torch.zeros_like(a))
    if a.numel() == 0:
        return torch.zeros((x4.shape[2],), dtype=torch.float32, device=x.device)
    return a.amax(dim=(0, 1, 3))


def absmax_reference(k, v, row_lens=None) -> Tensor:
    """The definition of hyd_kv_absmax in torch (any device): f32 [2, Hkv], row 0 the largest finite |k| of every kv head over
    k [outer, rows, Hkv, d] (or [rows, Hkv, d]), row 1 the same for v; a None tensor gives a row of zeros.  row_lens [outer]: outer
    index o contributes its first row_lens[o] rows.  NaN and +-inf elements are ignored, -0 and subnormals count by magnitude."""
    x = k if k is not None else v
    if x is None:
        raise ValueError("observe K, V or both: k and v are both None")
    rows = [_absmax_one(t, row_lens) if t is not None else torch.zeros((x.shape[-2],), dtype=torch.float32, device=x.device)
            for t in (k, v)]
    return torch.stack(rows)


def scales_from_absmax_reference(amax: Tensor, margin: float = 2.0, pow2: bool = True) -> Tensor:
    """The definition of hyd_kv_scales_from_absmax in torch: scales of amax's shape.  t = amax * c as an fp32 product,
    c = float32(margin / 448), clamped to [2^-100, 2^100]; pow2: the smallest power of two >= t (frexp / ldexp: t = m * 2^e with
    m in [0.5, 1) -> 2^e, or 2^(e - 1) when m == 0.5: a power of two is kept); amax == 0 gives 1.0.  The definition is the
    evaluation on CPU tensors: torch's GPU kernels may treat subnormal fp32 values as zero."""
    a = amax.to(torch.float32)
    c = torch.tensor(scale_constant(margin), dtype=torch.float32, device=a.device)
    lo = torch.tensor(2.0 ** SCALE_MIN_EXP, dtype=torch.float32, device=a.device)
    hi = torch.tensor(2.0 ** SCALE_MAX_EXP, dtype=torch.float32, device=a.device)
    t = torch.minimum(torch.maximum(a * c, lo), hi)
    if pow2:
        m, e = torch.frexp(t)
        e = torch.where(m == 0.5, e - 1, e)
        t = torch.ldexp(torch.ones_like(t), e)
    return torch.where(a == 0, torch.ones_like(t), t)


def observe_absmax(k, v, amax: Tensor, row_lens=None) -> None:
    """amax [2, Hkv] f32 <- max(amax, absmax_reference(k, v, row_lens)), in place: one hyd_kv_absmax launch on the current stream
    for GPU tensors (no allocation, no synchronisation, capture-safe), the definition for CPU tensors.  k / v: float16 / bfloat16
    views [outer, rows, Hkv, d] or [rows, Hkv, d] with any outer / row / head strides that are multiples of 8 elements, d
    contiguous (the k / v splits of a fused q|k|v GEMM output, a slice of a shared cache, a packed level, the halves of a
    placement.kv_arena: taken as they are, nothing is copied); either may be None: that row of amax is left alone.  row_lens
    [outer] int32 (int64 is converted: one small launch): rows at or past a length are never read, nor are columns past d."""
    x, Hkv = _check_observed(k, v, amax, row_lens)
    if not amax.is_cuda:
        ref = absmax_reference(k, v, row_lens).to(amax.device)
        for i, t in enumerate((k, v)):
            if t is not None:
                amax[i] = torch.maximum(amax[i], ref[i])
        return
    from .flash import _require_gpu, _stream

    _require_gpu(k, v, amax, row_lens)
    if x.numel() == 0:
        return  # nothing to read (an empty tensor has no address to hand over)
    p = _lib.KvAbsmaxParams()
    p.dtype = _lib.HYD_F16 if x.dtype == torch.float16 else _lib.HYD_BF16
    p.Hkv, p.d = Hkv, x.shape[-1]
    p.n_outer, p.n_rows = (x.shape[0], x.shape[1]) if x.ndim == 4 else (1, x.shape[0])
    for name, t in (("k", k), ("v", v)):
        if t is None:
            continue
        if t.stride(-1) != 1:
            raise ValueError(f"the head dim of {name} must be contiguous")
        st = t.stride() if t.ndim == 4 else (0,) + tuple(t.stride())
        setattr(p, name, t.data_ptr())
        setattr(p, name + "_outer_stride", st[0])
        setattr(p, name + "_row_stride", st[1])
        setattr(p, name + "_head_stride", st[2])
    if row_lens is not None:
        row_lens = row_lens.to(torch.int32).contiguous()
        p.row_lens = row_lens.data_ptr()
    p.amax = amax.data_ptr()
    _lib.check(_lib.load().hyd_kv_absmax(C.byref(p), _stream()))


def scales_from_absmax(amax: Tensor, k_scale: Tensor, v_scale: Tensor, margin: float = 2.0, pow2: bool = True) -> None:
    """k_scale / v_scale [Hkv] f32 <- scales_from_absmax_reference(amax [2, Hkv]) rows 0 / 1, in place: one
    hyd_kv_scales_from_absmax launch for GPU tensors (capture-safe), the definition for CPU tensors."""
    Hkv = amax.shape[-1] if amax.ndim == 2 else 0
    for name, t, shape in (("amax", amax, (2, Hkv)), ("k_scale", k_scale, (Hkv,)), ("v_scale", v_scale, (Hkv,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 {list(shape)} tensor, got {tuple(t.shape)} {t.dtype}")
    c = scale_constant(margin)
    if not amax.is_cuda:
        s = scales_from_absmax_reference(amax, margin, pow2)
        k_scale.copy_(s[0])
        v_scale.copy_(s[1])
        return
    from .flash import _require_gpu, _stream

    _require_gpu(amax, k_scale, v_scale)
    p = _lib.KvScalesParams()
    p.amax, p.k_scale, p.v_scale = amax.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr()
    p.Hkv, p.c, p.pow2 = Hkv, c, 1 if pow2 else 0
    _lib.check(_lib.load().hyd_kv_scales_from_absmax(C.byref(p), _stream()))
