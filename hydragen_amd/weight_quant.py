"""
fp8 (OCP e4m3fn) linear-layer weights: the quantizer, the definition of the product, and the module the model shell holds.

Weight-only quantization.  A weight w [N, K] is stored as codes w8 [N, K] in `torch.float8_e4m3fn` with one fp32 scale per output
channel; activations, accumulators and outputs stay as they are.  The scale of a row is the smallest power of two >= absmax(row)
/ 448 -- the rule of the fp8 K/V caches (kv_quant.scales_from_absmax_reference with margin 1) -- and 1.0 for an all-zero row; the
codes are (w.float() / scale).clamp(-448, 448) rounded to nearest even.  Every e4m3fn value is exactly a bf16 and an f16 value
and the scales are powers of two, so the dequantized weight is exact in 16 bits: `hyd_linear_w8` differs from a 16-bit GEMM on
`dequantize_weight` in accumulation order only.  Per-channel scales make concatenation along N exact: q|k|v and gate|up are
quantized per projection and concatenated, so fusing them changes no value.

    y[m, n] = round16(scale[n] * sum_k x[m, k] * w8[n, k])        (fp32 accumulation, the scale in fp32, one rounding)

`linear_reference` is that in float64.  What quantizing costs is the three mantissa bits: |deq - w| <= 2^-4 |w| + scale 2^-10
elementwise (half an ulp of a normal e4m3 value, the subnormal step below 2^-6 scale).
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor, nn

from . import _lib
from .kv_quant import FP8_DTYPE, FP8_MAX, scales_from_absmax_reference

# Rows (tokens of a step: batch x (drafts + 1)) up to which Fp8Linear runs hyd_linear_w8; above it the weight is widened into the
# model's scratch buffer (hyd_weight_widen) and a 16-bit F.linear runs on it.  Measured (profiles/weight_fp8.md, bf16, M in {1, 8,
# 16, 32, 64, 128, 256, 512}): the kernel beats widen + F.linear on all four Llama-2-7B shapes up to M = 128 (0.33-0.93 x its
# time) and loses on q|k|v, o and down at 256 (1.04-1.15 x): the crossover is 128.  Against the 16-bit F.linear of a model that is
# not quantized it wins up to M = 16 on every shape (0.48-0.75 x), is level at 32 (0.79-1.14 x) and at 64 / 128 wins on down only.
W8_MAX_ROWS = 128


def quantize_weight(w: Tensor) -> tuple[Tensor, Tensor]:
    """w [N, K] (any float dtype) -> (w8 float8_e4m3fn [N, K], scale float32 [N]).  +-inf and values beyond 448 * scale clamp to
    the largest finite code (the row's scale comes from its finite values); the NaN codes are never produced: NaN weights are
    refused."""
    if w.ndim != 2 or not w.is_floating_point():
        raise ValueError(f"quantize_weight takes a floating-point [N, K] weight, got {tuple(w.shape)} {w.dtype}")
    wf = w.detach().float()
    if bool(torch.isnan(wf).any()):
        raise ValueError("quantize_weight: the weight holds NaN")
    a = wf.abs()
    amax = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).amax(dim=1) if w.shape[1] else a.new_zeros((w.shape[0],))
    # the rule is evaluated on the CPU, where it is defined (torch's GPU kernels may treat subnormal fp32 values as zero)
    scale = scales_from_absmax_reference(amax.cpu(), margin=1.0, pow2=True).to(w.device)
    w8 = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
    return w8, scale


def _check_pair(w8: Tensor, scale: Tensor):
    if w8.dtype != FP8_DTYPE or w8.ndim != 2:
        raise TypeError(f"w8 must be a {FP8_DTYPE} [N, K] tensor, got {tuple(w8.shape)} {w8.dtype}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (w8.shape[0],):
        raise ValueError(f"scale must be float32 [{w8.shape[0]}], got {tuple(scale.shape)} {scale.dtype}")


def dequantize_weight(w8: Tensor, scale: Tensor, dtype: torch.dtype) -> Tensor:
    """float(w8) * scale[n] as an fp32 product, rounded once to `dtype` (exact for power-of-two scales and a 16-bit dtype as long
    as the product stays in the dtype's normal range)."""
    _check_pair(w8, scale)
    return (w8.float() * scale[:, None]).to(dtype)


def linear_reference(x: Tensor, w8: Tensor, scale: Tensor) -> Tensor:
    """The definition in float64: x [..., K] -> [..., N]."""
    _check_pair(w8, scale)
    return x.double() @ (w8.double() * scale.double()[:, None]).T


def _dtype_code(dtype: torch.dtype) -> int:
    if dtype == torch.float16:
        return _lib.HYD_F16
    if dtype == torch.bfloat16:
        return _lib.HYD_BF16
    raise NotImplementedError(f"dtype {dtype}: the fp8-weight kernels take float16 / bfloat16 activations")


def workspace_bytes(M: int, N: int, K: int) -> int:
    """Scratch bytes hyd_linear_w8 needs for x [M, K], w8 [N, K] (shapes only; 0 where the plan does not split K)."""
    return int(_lib.load().hyd_linear_w8_workspace_bytes(M, N, K))


def max_workspace_bytes(max_rows: int, N: int, K: int) -> int:
    """The largest workspace_bytes over 1 <= M <= max_rows: the plan changes at the row-tile boundaries 16, 32 and every 64, and
    between two boundaries the bytes grow with M."""
    ms = {min(max_rows, m) for m in (16, 32)} | {min(max_rows, m) for m in range(64, max_rows + 64, 64)}
    return max(workspace_bytes(m, N, K) for m in ms)


def linear_w8(x: Tensor, w8: Tensor, scale: Tensor, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """hyd_linear_w8 on the current stream: x [M, K] float16 / bfloat16 (unit last stride, rows 16-byte aligned), w8 [N, K]
    contiguous e4m3fn, scale [N] -> y [M, N] in x's dtype (out: a [M, N] view with a unit last stride to write into).  workspace:
    a uint8 buffer of at least workspace_bytes(M, N, K); None allocates one when the plan splits (not capture-safe by itself)."""
    from .flash import _require_gpu, _stream

    _require_gpu(x, w8, scale, out, workspace)
    _check_pair(w8, scale)
    if x.ndim != 2 or x.shape[1] != w8.shape[1]:
        raise ValueError(f"x must be [M, {w8.shape[1]}], got {tuple(x.shape)}")
    M, K = x.shape
    N = w8.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (M, N) or out.dtype != x.dtype:
        raise ValueError(f"out must be [{M}, {N}] {x.dtype}, got {tuple(out.shape)} {out.dtype}")
    if M == 0:
        return out
    if x.stride(1) != 1 or out.stride(1) != 1 or not w8.is_contiguous() or not scale.is_contiguous():
        raise ValueError("x and out need a unit last stride, w8 and scale must be contiguous")
    lib = _lib.load()
    need = int(lib.hyd_linear_w8_workspace_bytes(M, N, K))
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        if workspace is not None:
            raise ValueError(f"workspace holds {workspace.numel() * workspace.element_size()} bytes, the call needs {need}")
        workspace = torch.empty((need,), dtype=torch.uint8, device=x.device)
    p = _lib.LinearW8Params()
    p.x, p.w8, p.scale, p.y = x.data_ptr(), w8.data_ptr(), scale.data_ptr(), out.data_ptr()
    if need:
        p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    p.x_row_stride, p.y_row_stride = (x.stride(0), out.stride(0)) if M > 1 else (K, (N + 7) // 8 * 8)  # (one row: the stride is never used)
    p.M, p.N, p.K, p.dtype = M, N, K, _dtype_code(x.dtype)
    _lib.check(lib.hyd_linear_w8(C.byref(p), _stream()))
    return out


def weight_widen(w8: Tensor, scale: Tensor, out: Tensor) -> Tensor:
    """hyd_weight_widen on the current stream: out [N, K] float16 / bfloat16 (unit last stride) <- dequantize_weight(w8, scale,
    out.dtype), bit for bit.  One launch, nothing allocated."""
    from .flash import _require_gpu, _stream

    _require_gpu(w8, scale, out)
    _check_pair(w8, scale)
    if tuple(out.shape) != tuple(w8.shape) or out.stride(1) != 1 or not w8.is_contiguous() or not scale.is_contiguous():
        raise ValueError(f"out must be a [{w8.shape[0]}, {w8.shape[1]}] view with a unit last stride of contiguous w8 / scale")
    p = _lib.WeightWidenParams()
    p.w8, p.scale, p.out = w8.data_ptr(), scale.data_ptr(), out.data_ptr()
    p.out_row_stride = out.stride(0) if w8.shape[0] > 1 else w8.shape[1]
    p.N, p.K, p.dtype = w8.shape[0], w8.shape[1], _dtype_code(out.dtype)
    _lib.check(_lib.load().hyd_weight_widen(C.byref(p), _stream()))
    return out


class W8Scratch:
    """What the Fp8Linear modules of one model share, allocated once when the model is quantized so that no forward allocates
    (capture-safe; the calls of a model are ordered on one stream): `widen`, 16-bit room for the largest quantized weight (the
    route of calls with more than W8_MAX_ROWS rows), and `workspace`, the largest split-K scratch of any of them."""

    def __init__(self):
        self.widen: Optional[Tensor] = None
        self.workspace: Optional[Tensor] = None

    def reserve(self, N: int, K: int, dtype: torch.dtype, device, workspace: int) -> None:
        """Make room for a [N, K] weight of `dtype` and `workspace` split-K bytes on `device` (a no-op once it is there)."""
        device = torch.device(device)
        if device.type != "cuda":
            return
        w, ws = self.widen, self.workspace
        if w is None or w.numel() < N * K or w.dtype != dtype or w.device != device:
            self._no_capture()
            keep = w.numel() if w is not None and w.dtype == dtype and w.device == device else 0
            self.widen = torch.empty((max(N * K, keep),), dtype=dtype, device=device)
        if workspace and (ws is None or ws.numel() < workspace or ws.device != device):
            self._no_capture()
            self.workspace = torch.empty((workspace,), dtype=torch.uint8, device=device)

    @staticmethod
    def _no_capture():
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the fp8 weights' scratch buffers must exist before graph capture: run one forward (or "
                               "quantize_weights()) on this device and dtype first")


class Fp8Linear(nn.Module):
    """A linear layer on fp8 weights: `weight` float8_e4m3fn [N, K] and `weight_scale` float32 [N] (buffers: they travel in the
    state dict and are never trained), an optional 16-bit `bias` added by torch after the product.  `dtype` is the activation
    dtype the layer was quantized from (what `weight.dtype` was).  CPU tensors and dtypes the kernels do not take run the torch
    definition F.linear(x, dequantize_weight(...)); GPU calls with up to W8_MAX_ROWS rows run hyd_linear_w8, larger ones widen the
    weight into the shared scratch buffer (hyd_weight_widen) and run a 16-bit F.linear on it."""

    def __init__(self, weight: Tensor, weight_scale: Tensor, bias: Optional[Tensor] = None, dtype: torch.dtype = torch.bfloat16,
                 scratch: Optional[W8Scratch] = None):
        super().__init__()
        _check_pair(weight, weight_scale)
        self.out_features, self.in_features = weight.shape
        self.dtype = dtype
        self.register_buffer("weight", weight.contiguous())
        self.register_buffer("weight_scale", weight_scale.contiguous())
        self.bias = None if bias is None else nn.Parameter(bias.detach().clone(), requires_grad=False)
        self.scratch = scratch if scratch is not None else W8Scratch()
        self._ws_bytes = max_workspace_bytes(W8_MAX_ROWS, *weight.shape) if weight.is_cuda else None
        self._reserve(dtype, weight.device)

    def _reserve(self, dtype, device):
        if self._ws_bytes is None and torch.device(device).type == "cuda":
            self._ws_bytes = max_workspace_bytes(W8_MAX_ROWS, self.out_features, self.in_features)
        self.scratch.reserve(self.out_features, self.in_features, dtype, device, self._ws_bytes or 0)

    @classmethod
    def from_linears(cls, linears, scratch: Optional[W8Scratch] = None) -> "Fp8Linear":
        """One module for several nn.Linear that read the same input (q|k|v, gate|up; or a single one): every projection is
        quantized on its own and the codes, scales and biases are concatenated along N."""
        pairs = [quantize_weight(l.weight) for l in linears]
        bias = None
        if any(l.bias is not None for l in linears):
            bias = torch.cat([l.bias if l.bias is not None else l.weight.new_zeros((l.weight.shape[0],)) for l in linears])
        return cls(torch.cat([p[0].view(torch.uint8) for p in pairs]).view(FP8_DTYPE), torch.cat([p[1] for p in pairs]), bias,
                   linears[0].weight.dtype, scratch)

    def _apply(self, fn, recurse=True):
        """`.to(device)` moves the buffers as they are.  A floating-point cast (`.to(torch.float16)`, `.half()`) would turn the codes
        and the scales into 16-bit values: they keep their formats, and the cast sets the activation dtype instead."""
        w8, scale = self.weight, self.weight_scale
        super()._apply(fn, recurse)
        if self.weight.dtype != FP8_DTYPE:
            self.dtype = self.weight.dtype
            self.weight, self.weight_scale = w8.to(self.weight.device), scale.to(self.weight.device)
        elif self.weight_scale.dtype != torch.float32:
            self.weight_scale = scale.to(self.weight.device)
        return self

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, fp8 weights for {self.dtype}"

    def dequantized(self, dtype: Optional[torch.dtype] = None) -> Tensor:
        return dequantize_weight(self.weight, self.weight_scale, self.dtype if dtype is None else dtype)

    def forward(self, x: Tensor) -> Tensor:
        N, K = self.out_features, self.in_features
        if not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16) or x.numel() == 0:
            return nn.functional.linear(x, self.dequantized(x.dtype), self.bias)
        x2 = x.reshape(-1, K)
        rows = x2.shape[0]
        if rows <= W8_MAX_ROWS:
            if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
                x2 = x2.clone(memory_format=torch.contiguous_format)
            self._reserve(x.dtype, x.device)
            y = linear_w8(x2, self.weight, self.weight_scale, workspace=self.scratch.workspace)
        else:
            self._reserve(x.dtype, x.device)
            w16 = weight_widen(self.weight, self.weight_scale, self.scratch.widen[: N * K].view(N, K))
            y = nn.functional.linear(x2, w16)
        if self.bias is not None:
            y = y + self.bias
        return y.view(*x.shape[:-1], N)


# ---- 4-bit (OCP e2m1) weights ----------------------------------------------------------------------------------------------------
# A weight w [N, K], K % 32 == 0, as three tensors: `w4` uint8 [N, K / 2] (byte i of a row holds the e2m1 code of k = 2 i in its low
# nibble and of k = 2 i + 1 in its high nibble; codes are sign + magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}), `shift` uint8 [N, K / 32]
# (0..12, one per group of 32 consecutive k) and `scale` float32 [N] (a power of two per output channel).  The dequantized weight is

#     e2m1(code) * 2^-shift[n, k // 32] * scale[n]

# MX-style block scaling in two levels: e2m1 * 2^-shift lies in [2^-13, 6] for every non-zero code -- an exact normal value in bf16
# AND f16 whatever the row's magnitude -- and scale[n] is applied once to the fp32 sum, as hyd_linear_w8 applies its scale.  So
# `hyd_linear_w4` differs from a 16-bit GEMM on the dequantized weight in accumulation order only, and concatenation along N is exact.
FP4_DTYPE = torch.float4_e2m1fn_x2  # what quantize_weights(dtype=...) names the format by; the codes travel as uint8
FP4_MAX_SHIFT = 12
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)

# Rows up to which Fp4Linear runs hyd_linear_w4; above it the weight is widened into the model's scratch buffer
# (hyd_weight_widen_w4) and a 16-bit F.linear runs on it.  Measured (profiles/weight_fp4.md, bf16, M in {1, 8, 16, 32, 64, 128, 256}):
# the kernel beats widen + F.linear on all four Llama-2-7B shapes at every M up to 128 (0.45-0.76 x its time there); 128 is also the
# extent of the rows form.  Against the 16-bit F.linear of a model that is not quantized it wins up to M = 32 on every shape and
# loses from 64 on q|k|v and o.
W4_MAX_ROWS = 128


def _pow2_exponent_over_6(amax: Tensor) -> Tensor:
    """q with 2^q the smallest power of two >= amax / 6 (int32; exact: amax = m 2^e with m in [0.5, 1) needs 6 * 2^q >= m 2^e, which
    is q = e - 3 up to m = 0.75 and e - 2 above), at least -126 so that 2^q is a normal fp32 value; 0 where amax == 0."""
    m, e = torch.frexp(amax)
    q = torch.where(m <= 0.75, e - 3, e - 2).clamp(min=-126)
    return torch.where(amax > 0, q, torch.zeros_like(q)).to(torch.int32)


def quantize_weight_fp4(w: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """w [N, K] (any float dtype, K % 32 == 0) -> (w4 uint8 [N, K / 2], shift uint8 [N, K / 32], scale float32 [N]).
    scale[n] is the smallest power of two >= absmax(row) / 6 (1.0 for a zero row); a group's own smallest power of two >=
    absmax(group) / 6 is expressed as scale[n] * 2^-shift with shift clamped to [0, 12] (a zero group gets 0); the codes are
    w / (scale * 2^-shift) clamped to +-6 and rounded to the nearest e2m1 value, ties to the even mantissa.  +-inf clamps (scales come
    from the finite values), NaN is refused.  The rule is evaluated in float64 (exact: no subnormal fp32 value takes part), so the
    device it runs on does not matter.
    What it costs, elementwise: |deq - w| <= max(|w|, group scale) / 4 wherever the shift was not clamped -- half a step of the
    one mantissa bit (1 of 4 at |t| in [4, 6], 0.5 of 2 at [2, 4), 0.25 of 1 at [1, 2)) and the quarter step below one group scale."""
    if w.ndim != 2 or not w.is_floating_point() or w.shape[1] % 32:
        raise ValueError(f"quantize_weight_fp4 takes a floating-point [N, K] weight with K % 32 == 0, got {tuple(w.shape)} {w.dtype}")
    wf = w.detach().double()
    if bool(torch.isnan(wf).any()):
        raise ValueError("quantize_weight_fp4: the weight holds NaN")
    N, K = wf.shape
    a = wf.abs()
    ga = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).view(N, K // 32, 32).amax(dim=2)
    q = _pow2_exponent_over_6(ga.amax(dim=1)) if K else torch.zeros((N,), dtype=torch.int32, device=w.device)
    gq = _pow2_exponent_over_6(ga)
    shift = torch.where(ga > 0, q[:, None] - gq, torch.zeros_like(gq)).clamp(0, FP4_MAX_SHIFT)
    scale = torch.ldexp(torch.ones((N,), device=w.device), q)
    step = torch.ldexp(torch.ones((N, K // 32), dtype=torch.float64, device=w.device), q[:, None] - shift)
    t = (wf.view(N, K // 32, 32) / step[:, :, None]).clamp(-6, 6).view(N, K)
    v = t.abs()
    v = torch.where(v < 2, torch.round(v * 2) / 2, torch.where(v < 4, torch.round(v), torch.round(v / 2) * 2))  # half to even = even mantissa
    idx = torch.where(v < 2, v * 2, torch.where(v < 4, v + 2, v / 2 + 4)).to(torch.uint8) | ((t < 0).to(torch.uint8) << 3)
    w4 = idx[:, 0::2] | (idx[:, 1::2] << 4)
    return w4.contiguous(), shift.to(torch.uint8), scale


def _check_triple(w4: Tensor, shift: Tensor, scale: Tensor):
    if w4.dtype != torch.uint8 or w4.ndim != 2 or w4.shape[1] % 16:
        raise TypeError(f"w4 must be a uint8 [N, K / 2] tensor with K % 32 == 0, got {tuple(w4.shape)} {w4.dtype}")
    if shift.dtype != torch.uint8 or tuple(shift.shape) != (w4.shape[0], w4.shape[1] // 16):
        raise ValueError(f"shift must be uint8 [{w4.shape[0]}, {w4.shape[1] // 16}], got {tuple(shift.shape)} {shift.dtype}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (w4.shape[0],):
        raise ValueError(f"scale must be float32 [{w4.shape[0]}], got {tuple(scale.shape)} {scale.dtype}")


def _group_values(w4: Tensor, shift: Tensor, dtype: torch.dtype) -> Tensor:
    """e2m1(code) * 2^-shift as [N, K] of `dtype` (exact in float32 and float64)."""
    lut = torch.tensor(_E2M1 + tuple(-x for x in _E2M1), dtype=dtype, device=w4.device)
    codes = torch.stack((w4 & 15, w4 >> 4), dim=2).view(w4.shape[0], -1).long()
    return lut[codes] * torch.ldexp(torch.ones((), dtype=dtype, device=w4.device), -shift.to(torch.int32)).repeat_interleave(32, dim=1)


def dequantize_weight_fp4(w4: Tensor, shift: Tensor, scale: Tensor, dtype: torch.dtype) -> Tensor:
    """(e2m1(code) * 2^-shift) * scale[n] as an fp32 product, rounded once to `dtype`."""
    _check_triple(w4, shift, scale)
    return (_group_values(w4, shift, torch.float32) * scale[:, None]).to(dtype)


def linear_reference_fp4(x: Tensor, w4: Tensor, shift: Tensor, scale: Tensor) -> Tensor:
    """The definition in float64: x [..., K] -> [..., N]."""
    _check_triple(w4, shift, scale)
    return x.double() @ (_group_values(w4, shift, torch.float64) * scale.double()[:, None]).T


class LinearW4Params(C.Structure):  # hyd_linear_w4_params
    _fields_ = [
        ("x", C.c_void_p), ("w4", C.c_void_p), ("shift", C.c_void_p), ("scale", C.c_void_p), ("y", C.c_void_p), ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t), ("x_row_stride", C.c_int64), ("y_row_stride", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("dtype", C.c_int32),
    ]


class WeightWidenW4Params(C.Structure):  # hyd_weight_widen_w4_params
    _fields_ = [
        ("w4", C.c_void_p), ("shift", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p), ("out_row_stride", C.c_int64),
        ("N", C.c_int32), ("K", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


def max_workspace_bytes_w4(max_rows: int, N: int, K: int) -> int:
    """The largest hyd_linear_w4_workspace_bytes over 1 <= M <= max_rows (the plan changes where hyd_linear_w8's does)."""
    q = _lib.load().hyd_linear_w4_workspace_bytes
    ms = {min(max_rows, m) for m in (16, 32)} | {min(max_rows, m) for m in range(64, max_rows + 64, 64)}
    return max(int(q(m, N, K)) for m in ms)


def linear_w4(x: Tensor, w4: Tensor, shift: Tensor, scale: Tensor, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """hyd_linear_w4 on the current stream: x [M, K] float16 / bfloat16 (unit last stride, rows 16-byte aligned), contiguous w4
    [N, K / 2], shift [N, K / 32] and scale [N] -> y [M, N] in x's dtype.  out and workspace as in linear_w8 (the bytes:
    hyd_linear_w4_workspace_bytes(M, N, K))."""
    from .flash import _require_gpu, _stream

    _require_gpu(x, w4, shift, scale, out, workspace)
    _check_triple(w4, shift, scale)
    N, K = w4.shape[0], w4.shape[1] * 2
    if x.ndim != 2 or x.shape[1] != K:
        raise ValueError(f"x must be [M, {K}], got {tuple(x.shape)}")
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (M, N) or out.dtype != x.dtype:
        raise ValueError(f"out must be [{M}, {N}] {x.dtype}, got {tuple(out.shape)} {out.dtype}")
    if M == 0:
        return out
    if x.stride(1) != 1 or out.stride(1) != 1 or not (w4.is_contiguous() and shift.is_contiguous() and scale.is_contiguous()):
        raise ValueError("x and out need a unit last stride, w4, shift and scale must be contiguous")
    lib = _lib.load()
    need = int(lib.hyd_linear_w4_workspace_bytes(M, N, K))
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        if workspace is not None:
            raise ValueError(f"workspace holds {workspace.numel() * workspace.element_size()} bytes, the call needs {need}")
        workspace = torch.empty((need,), dtype=torch.uint8, device=x.device)
    p = LinearW4Params()
    p.x, p.w4, p.shift, p.scale, p.y = x.data_ptr(), w4.data_ptr(), shift.data_ptr(), scale.data_ptr(), out.data_ptr()
    if need:
        p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    p.x_row_stride, p.y_row_stride = (x.stride(0), out.stride(0)) if M > 1 else (K, (N + 7) // 8 * 8)  # (one row: the stride is never used)
    p.M, p.N, p.K, p.dtype = M, N, K, _dtype_code(x.dtype)
    _lib.check(lib.hyd_linear_w4(C.byref(p), _stream()))
    return out


def weight_widen_fp4(w4: Tensor, shift: Tensor, scale: Tensor, out: Tensor) -> Tensor:
    """hyd_weight_widen_w4 on the current stream: out [N, K] float16 / bfloat16 (unit last stride) <- dequantize_weight_fp4(w4,
    shift, scale, out.dtype), bit for bit.  One launch, nothing allocated."""
    from .flash import _require_gpu, _stream

    _require_gpu(w4, shift, scale, out)
    _check_triple(w4, shift, scale)
    N, K = w4.shape[0], w4.shape[1] * 2
    if tuple(out.shape) != (N, K) or out.stride(1) != 1 or not (w4.is_contiguous() and shift.is_contiguous() and scale.is_contiguous()):
        raise ValueError(f"out must be a [{N}, {K}] view with a unit last stride of contiguous w4 / shift / scale")
    p = WeightWidenW4Params()
    p.w4, p.shift, p.scale, p.out = w4.data_ptr(), shift.data_ptr(), scale.data_ptr(), out.data_ptr()
    p.out_row_stride = out.stride(0) if N > 1 else K
    p.N, p.K, p.dtype = N, K, _dtype_code(out.dtype)
    _lib.check(_lib.load().hyd_weight_widen_w4(C.byref(p), _stream()))
    return out


class Fp4Linear(Fp8Linear):
    """A linear layer on 4-bit weights: buffers `weight` uint8 [N, K / 2], `weight_shift` uint8 [N, K / 32] and `weight_scale`
    float32 [N], an optional 16-bit `bias`.  Everything else is Fp8Linear's: CPU tensors run the torch definition, GPU calls with
    up to W4_MAX_ROWS rows run hyd_linear_w4, larger ones widen into the model's shared W8Scratch and run a 16-bit F.linear."""

    def __init__(self, weight: Tensor, weight_shift: Tensor, weight_scale: Tensor, bias: Optional[Tensor] = None,
                 dtype: torch.dtype = torch.bfloat16, scratch: Optional[W8Scratch] = None):
        nn.Module.__init__(self)
        _check_triple(weight, weight_shift, weight_scale)
        self.out_features, self.in_features = weight.shape[0], weight.shape[1] * 2
        self.dtype = dtype
        self.register_buffer("weight", weight.contiguous())
        self.register_buffer("weight_shift", weight_shift.contiguous())
        self.register_buffer("weight_scale", weight_scale.contiguous())
        self.bias = None if bias is None else nn.Parameter(bias.detach().clone(), requires_grad=False)
        self.scratch = scratch if scratch is not None else W8Scratch()
        self._ws_bytes = None
        self._reserve(dtype, weight.device)

    def _reserve(self, dtype, device):
        if self._ws_bytes is None and torch.device(device).type == "cuda":
            self._ws_bytes = max_workspace_bytes_w4(W4_MAX_ROWS, self.out_features, self.in_features)
        self.scratch.reserve(self.out_features, self.in_features, dtype, device, self._ws_bytes or 0)

    @classmethod
    def from_linears(cls, linears, scratch: Optional[W8Scratch] = None) -> "Fp4Linear":
        """One module for several nn.Linear that read the same input: every projection is quantized on its own and the codes,
        shifts, scales and biases are concatenated along N."""
        parts = [quantize_weight_fp4(l.weight) for l in linears]
        bias = None
        if any(l.bias is not None for l in linears):
            bias = torch.cat([l.bias if l.bias is not None else l.weight.new_zeros((l.weight.shape[0],)) for l in linears])
        return cls(*(torch.cat([p[i] for p in parts]) for i in range(3)), bias, linears[0].weight.dtype, scratch)

    def _apply(self, fn, recurse=True):
        """`.to(device)` moves the buffers as they are.  A floating-point cast leaves the integer buffers alone and would turn the
        scales into 16-bit values: they stay float32, and the cast sets the activation dtype instead."""
        scale = self.weight_scale
        nn.Module._apply(self, fn, recurse)
        if self.weight_scale.dtype != torch.float32:
            self.dtype = self.weight_scale.dtype
            self.weight_scale = scale.to(self.weight.device)
        return self

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, e2m1 weights for {self.dtype}"

    def dequantized(self, dtype: Optional[torch.dtype] = None) -> Tensor:
        return dequantize_weight_fp4(self.weight, self.weight_shift, self.weight_scale, self.dtype if dtype is None else dtype)

    def forward(self, x: Tensor) -> Tensor:
        N, K = self.out_features, self.in_features
        if not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16) or x.numel() == 0:
            return nn.functional.linear(x, self.dequantized(x.dtype), self.bias)
        x2 = x.reshape(-1, K)
        self._reserve(x.dtype, x.device)
        if x2.shape[0] <= W4_MAX_ROWS:
            if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.data_ptr() % 16:
                x2 = x2.clone(memory_format=torch.contiguous_format)
            y = linear_w4(x2, self.weight, self.weight_shift, self.weight_scale, workspace=self.scratch.workspace)
        else:
            w16 = weight_widen_fp4(self.weight, self.weight_shift, self.weight_scale, self.scratch.widen[: N * K].view(N, K))
            y = nn.functional.linear(x2, w16)
        if self.bias is not None:
            y = y + self.bias
        return y.view(*x.shape[:-1], N)
