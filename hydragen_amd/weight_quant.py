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
