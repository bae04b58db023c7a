"""
Mixture-of-experts MLP: the DEFINITION of routing and of the expert products with the elementwise error bound that goes with it,
and the device path that is held to them -- `moe_mlp` (hyd_moe_mlp, csrc/moe.hip: routing, grouping and the expert products on the
device, capture-safe) and `MoeMLP`, the module a decoder layer of a model with experts carries (llama.py).

    logits = round16(x @ router_w^T)
    ids, weights = the k largest logits of a row, descending, ties to the lower index; softmax(logits)[ids], renormalized or not
    act[t, j] = round16(silu(x[t] @ Wg[e_j]^T) * (x[t] @ Wu[e_j]^T))          (gate_up[e] = Wg[e] rows, then Wu[e] rows)
    y[t] = sum_j weights[t, j] * (act[t, j] @ Wd[e_j]^T)                      (in j order; rounded once by whoever compares)

Large inputs with 16-bit experts (`moe_rows_grouped`, hyd_moe_mlp_grouped, csrc/moe_grouped.hip): up to 2048 rows per call, the slots
sorted by expert and both products tiled through LDS, so that an expert is read once per call; the same definition and bound.

The weight layouts are transformers 5's (`experts.gate_up_proj` [E, 2 I, H], `experts.down_proj` [E, H, I], `gate.weight` [E, H]).

fp8 experts (`quantize_experts`, hyd_moe_mlp_w8, csrc/moe_w8.hip, `Fp8Experts`): the two expert tensors as e4m3fn codes with one
power-of-two fp32 scale per expert and output channel -- weight_quant.quantize_weight's rule on the [E N, K] view.  The fp8 MLP is
DEFINED as `moe_reference` on the float64 dequantized weights (code * scale, exact), and `moe_error_bound` on the same weights is
its bound: the codes are exact 16-bit values and the scales powers of two applied to the fp32 sums, so a kernel differs from the
16-bit kernels on the dequantized weights in accumulation order only.  The router stays a 16-bit F.linear.

Large inputs with fp8 experts (`moe_rows_grouped_w8`, hyd_moe_mlp_grouped_w8, csrc/moe_grouped_w8.hip): the grouped call on the same
four tensors -- its sort, its workspace and its range of rows, the weights carried as codes through LDS and widened in registers; the
fp8 definition and bound.  `moe_mlp(..., grouped=True)` reaches it, and `MoeMLP` with Fp8Experts from MOE_GROUPED_W8_MIN_ROWS rows
on (profiles/moe.md has the measurement that sets it).  4-bit experts have no grouped kernel.

4-bit experts (`quantize_experts_fp4`, hyd_moe_mlp_w4, csrc/moe_w4.hip, `Fp4Experts`): weight_quant.quantize_weight_fp4's format on
the same view -- packed e2m1 codes [E, N, K / 2], a shift 0..12 per group of 32 k [E, N, K / 32], a power-of-two scale per expert
and output channel [E, N].  The 4-bit MLP is DEFINED the same way, as `moe_reference` on e2m1(code) * 2^-shift * scale in float64
with `moe_error_bound` on the same weights: e2m1 * 2^-shift lies in [2^-13, 6], an exact normal value in both 16-bit types, and the
channel scale multiplies the fp32 sum, so here too a kernel differs in accumulation order only (what the quantizer costs is the
quantizer's, not the kernel's: the bound has no term for it).
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor, nn

from . import _lib
from .kv_quant import FP8_DTYPE
from .weight_quant import _group_values, quantize_weight, quantize_weight_fp4


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def route_reference(logits: Tensor, k: int, renormalize: bool) -> tuple[Tensor, Tensor]:
    """logits [T, E] -> (ids [T, k] int64, weights [T, k] float64): the k largest LOGITS of a row in descending order, equal logits
    to the lower expert index (a stable descending sort; torch.topk leaves the order of ties open), weights = softmax(logits in
    float64)[ids], divided by their sum when `renormalize`.
    This is transformers' router (softmax in float, top-k of the probabilities, optional renormalisation) with the tie rule made
    definite.  The two can differ only where distinct logits round to equal fp32 probabilities: there transformers' top-k sees a tie
    that the logits do not have, and may pick either."""
    if logits.ndim != 2 or not 1 <= k <= logits.shape[1]:
        raise ValueError(f"route_reference takes [T, E] logits and 1 <= k <= E, got {tuple(logits.shape)}, k = {k}")
    l = logits.double()
    ids = torch.sort(l, dim=1, descending=True, stable=True).indices[:, :k]
    w = torch.softmax(l, dim=1).gather(1, ids)
    return ids, w / w.sum(dim=1, keepdim=True) if renormalize else w


def _slot_terms(x: Tensor, gate_up: Tensor, down: Tensor, ids: Tensor):
    """Per route position j: (rows of the float64 down product of the rounded act, and the abs-sum terms the bound is made of)."""
    xd, I = x.double(), gate_up.shape[1] // 2
    for j in range(ids.shape[1]):
        y = xd.new_zeros(x.shape)
        s_act, s_gu = xd.new_zeros(x.shape), xd.new_zeros(x.shape)  # sum_i |act_i wd_i|, sum_i dact_i |wd_i| / (H 2^-23)
        s_wd = xd.new_zeros(x.shape)                                 # sum_i |wd_i|
        for e in ids[:, j].unique().tolist():
            rows = (ids[:, j] == e).nonzero()[:, 0]
            w, wd = gate_up[e].double(), down[e].double()
            g, u = (xd[rows] @ w.T).split(I, dim=1)
            ag, au = (xd[rows].abs() @ w.abs().T).split(I, dim=1)
            silu = torch.nn.functional.silu(g)
            act = (silu * u).to(x.dtype).double()
            y[rows] = act @ wd.T
            s_act[rows] = act.abs() @ wd.abs().T
            s_gu[rows] = (ag * u.abs() * 1.1 + au * silu.abs()) @ wd.abs().T
            s_wd[rows] = wd.abs().sum(dim=1)[None].expand(len(rows), -1)
        yield j, y, s_act, s_gu, s_wd


def _routed(x: Tensor, router_w: Tensor, k: int, renormalize: bool, logits: Optional[Tensor] = None):
    # the product stays a 16-bit F.linear; `logits`: the ones a device call routed by (a GEMM's last bit may depend on the device)
    return route_reference(torch.nn.functional.linear(x, router_w) if logits is None else logits, k, renormalize)


def moe_reference(x: Tensor, router_w: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool, logits: Optional[Tensor] = None) -> Tensor:
    """The definition in float64: x [T, H], router_w [E, H], gate_up [E, 2 I, H], down [E, H, I] (all of one 16-bit dtype) ->
    [T, H] float64.  Two 16-bit roundings per token and expert on the way -- the router logits and act -- exactly where the
    kernels round; the output's own rounding is left to the caller of the comparison.  `logits` [T, E], when given, are routed by
    in place of round16(x @ router_w^T)."""
    ids, w = _routed(x, router_w, k, renormalize, logits)
    out = x.new_zeros(x.shape, dtype=torch.float64)
    for j, y, *_ in _slot_terms(x, gate_up, down, ids):
        out += w[:, j, None] * y
    return out


def moe_error_bound(x: Tensor, router_w: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool, logits: Optional[Tensor] = None) -> Tensor:
    """Elementwise bound [T, H] (float64) on |kernel output - moe_reference| that goes with the definition, from sums of absolute
    products; u16 = 2^-8 (bfloat16) or 2^-11 (float16) is half a 16-bit ulp, relative.  With y_j = act_j . wd (float64) and w_j the
    route weight, a kernel's out = round16(sum_j fl(w_j' * fl(act_j' . wd))) differs from sum_j w_j y_j by at most the sum of
      - the final rounding: u16 |y|;
      - the down product's fp32 accumulation over I terms: I 2^-23 sum_i |act_i wd_i| (the form of the fp8 linear bound, K 2^-23
        sum |x w|);
      - act values that differ from the definition's: the kernel rounds the fp32 value of silu(g) u, the definition the exact one.
        The fp32 value is off by at most d_i = H 2^-23 (sum |x wg| |u| 1.1 + sum |x wu| |silu g|) -- the gate and up accumulations over
        H terms, carried through the product rule with |silu'| <= 1.1 -- which reaches the output as sum_i d_i |wd_i|; and where d_i
        pushes the value across a rounding boundary the rounded act moves to the neighbouring 16-bit value: u16 sum_i |act_i wd_i|;
      - the route weight (fp32 exponentials: within 4 2^-23 relative of the float64 softmax), its fp32 product with the row and the
        k - 1 fp32 additions of the combine: (k + 5) 2^-23 |w_j y_j| in all;
    all weighted by w_j and summed over j.  float16 adds the absolute half-steps below its normal range: 2^-25 sum_i |wd_i| per act
    row and 2^-25 for the output.  `logits` as in moe_reference."""
    ids, w = _routed(x, router_w, k, renormalize, logits)
    H, I = x.shape[1], down.shape[2]
    u16, tiny = (2.0 ** -8, 0.0) if x.dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    out = x.new_zeros(x.shape, dtype=torch.float64)
    bound = x.new_zeros(x.shape, dtype=torch.float64)
    for j, y, s_act, s_gu, s_wd in _slot_terms(x, gate_up, down, ids):
        wj = w[:, j, None]
        out += wj * y
        bound += wj * ((I * 2.0 ** -23 + u16) * s_act + H * 2.0 ** -23 * s_gu + (k + 5) * 2.0 ** -23 * y.abs() + tiny * s_wd)
    return bound + u16 * out.abs() + tiny


def quantize_experts(gate_up: Tensor, down: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """gate_up [E, 2 I, H], down [E, H, I] (any float dtype) -> (gate_up8 e4m3fn [E, 2 I, H], gate_up_scale float32 [E, 2 I], down8
    [E, H, I], down_scale [E, H]): quantize_weight on the [E N, K] view -- a gate row, an up row and a down row each own a scale."""
    out = []
    for w in (gate_up, down):
        if w.ndim != 3:
            raise ValueError(f"quantize_experts takes [E, N, K] expert weights, got {tuple(w.shape)}")
        w8, scale = quantize_weight(w.reshape(-1, w.shape[2]))
        out += [w8.view(w.shape), scale.view(w.shape[:2])]
    return tuple(out)


def _check_experts8(gate_up8: Tensor, gate_up_scale: Tensor, down8: Tensor, down_scale: Tensor):
    for name, w8, scale in (("gate_up", gate_up8, gate_up_scale), ("down", down8, down_scale)):
        if w8.dtype != FP8_DTYPE or w8.ndim != 3:
            raise TypeError(f"{name} must be a {FP8_DTYPE} [E, N, K] tensor, got {tuple(w8.shape)} {w8.dtype}")
        if scale is None or scale.dtype != torch.float32 or tuple(scale.shape) != tuple(w8.shape[:2]):
            raise ValueError(f"{name}_scale must be float32 {tuple(w8.shape[:2])}, got {None if scale is None else (tuple(scale.shape), scale.dtype)}")


def dequantize_experts(gate_up8: Tensor, gate_up_scale: Tensor, down8: Tensor, down_scale: Tensor, dtype: torch.dtype = torch.float64) -> tuple[Tensor, Tensor]:
    """(gate_up, down) = code * scale in `dtype`: exact in float64 and float32, and in a 16-bit dtype as long as the product stays in
    its normal range."""
    _check_experts8(gate_up8, gate_up_scale, down8, down_scale)
    return tuple((w8.double() * scale.double()[:, :, None]).to(dtype) for w8, scale in ((gate_up8, gate_up_scale), (down8, down_scale)))


def quantize_experts_fp4(gate_up: Tensor, down: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """gate_up [E, 2 I, H], down [E, H, I] (any float dtype) -> (gate_up4 uint8 [E, 2 I, H / 2], gate_up_shift uint8 [E, 2 I, H / 32],
    gate_up_scale float32 [E, 2 I], down4 [E, H, I / 2], down_shift [E, H, I / 32], down_scale [E, H]): quantize_weight_fp4 on the
    [E N, K] view.  Byte b of a row holds k = 2 b in its low nibble and k = 2 b + 1 in its high nibble, as in Fp4Linear."""
    out = []
    for w in (gate_up, down):
        if w.ndim != 3:
            raise ValueError(f"quantize_experts_fp4 takes [E, N, K] expert weights, got {tuple(w.shape)}")
        w4, shift, scale = quantize_weight_fp4(w.reshape(-1, w.shape[2]))
        out += [w4.view(*w.shape[:2], -1), shift.view(*w.shape[:2], -1), scale.view(w.shape[:2])]
    return tuple(out)


def _check_experts4(gate_up4: Tensor, gate_up_shift: Tensor, gate_up_scale: Tensor, down4: Tensor, down_shift: Tensor, down_scale: Tensor):
    for name, w4, shift, scale in (("gate_up", gate_up4, gate_up_shift, gate_up_scale), ("down", down4, down_shift, down_scale)):
        if w4.dtype != torch.uint8 or w4.ndim != 3 or w4.shape[2] % 16:
            raise TypeError(f"{name} must be a uint8 [E, N, K / 2] tensor of packed e2m1 codes with K % 32 == 0, got {tuple(w4.shape)} {w4.dtype}")
        E, N, K2 = w4.shape
        if shift is None or shift.dtype != torch.uint8 or tuple(shift.shape) != (E, N, K2 // 16):
            raise ValueError(f"{name}_shift must be uint8 {(E, N, K2 // 16)}, got {None if shift is None else (tuple(shift.shape), shift.dtype)}")
        if scale is None or scale.dtype != torch.float32 or tuple(scale.shape) != (E, N):
            raise ValueError(f"{name}_scale must be float32 {(E, N)}, got {None if scale is None else (tuple(scale.shape), scale.dtype)}")


def dequantize_experts_fp4(gate_up4: Tensor, gate_up_shift: Tensor, gate_up_scale: Tensor, down4: Tensor, down_shift: Tensor, down_scale: Tensor,
                           dtype: torch.dtype = torch.float64) -> tuple[Tensor, Tensor]:
    """(gate_up, down) = e2m1(code) * 2^-shift * scale in `dtype`: exact in float64 and float32, and in a 16-bit dtype as long as the
    product stays in its normal range."""
    _check_experts4(gate_up4, gate_up_shift, gate_up_scale, down4, down_shift, down_scale)
    out = []
    for w4, shift, scale in ((gate_up4, gate_up_shift, gate_up_scale), (down4, down_shift, down_scale)):
        E, N, K2 = w4.shape
        out.append((_group_values(w4.reshape(E * N, K2), shift.reshape(E * N, -1), torch.float64).view(E, N, 2 * K2) * scale.double()[:, :, None]).to(dtype))
    return tuple(out)


# ---- the device path ---------------------------------------------------------------------------------------------------------------
MOE_MAX_ROWS = 128  # HYD_MOE_MAX_ROWS: rows per hyd_moe_mlp call; moe_mlp chunks longer inputs (the MLP is row-independent: exact)
MOE_GROUPED_MAX_ROWS = 2048  # HYD_MOE_GROUPED_MAX_ROWS: rows per hyd_moe_mlp_grouped call (csrc/moe_grouped.hip)
MOE_GROUPED_MIN_ROWS = 512  # moe_mlp: 16-bit experts take the grouped call from this many rows on (profiles/moe.md has the measurement)
# MoeMLP: Fp8Experts take hyd_moe_mlp_grouped_w8 from this many rows on (None: never).  256 is the smallest size measured: 2.1 - 2.5 x the
# chunked fp8 route there on both layers of profiles/moe.md, spreads under 1 %; smaller calls were not measured
MOE_GROUPED_W8_MIN_ROWS: Optional[int] = 256

_MOE_FIELDS = [
    ("x", C.c_void_p), ("logits", C.c_void_p), ("gate_up", C.c_void_p), ("down", C.c_void_p), ("y", C.c_void_p), ("workspace", C.c_void_p),
    ("workspace_bytes", C.c_size_t), ("ids_out", C.c_void_p), ("weights_out", C.c_void_p), ("x_row_stride", C.c_int64), ("y_row_stride", C.c_int64),
    ("T", C.c_int32), ("E", C.c_int32), ("k", C.c_int32), ("H", C.c_int32), ("I", C.c_int32), ("renormalize", C.c_int32), ("dtype", C.c_int32),
    ("reserved", C.c_int32),
]


class MoeParams(C.Structure):  # hyd_moe_params
    _fields_ = _MOE_FIELDS


class MoeW8Params(C.Structure):  # hyd_moe_w8_params
    _fields_ = _MOE_FIELDS + [("gate_up_scale", C.c_void_p), ("down_scale", C.c_void_p)]


class MoeW4Params(C.Structure):  # hyd_moe_w4_params
    _fields_ = MoeW8Params._fields_ + [("gate_up_shift", C.c_void_p), ("down_shift", C.c_void_p)]


_workspaces: dict = {}  # (device, rows, E, k, H, I, dtype, grouped) -> uint8 tensor: allocated on first use, so that a graph's replay allocates nothing


def _workspace(device, T, E, k, H, I, dtype, grouped=False) -> Tensor:
    key = (device, T, E, k, H, I, dtype, grouped)
    ws = _workspaces.get(key)
    if ws is None:
        query = _lib.load().hyd_moe_grouped_workspace_bytes if grouped else _lib.load().hyd_moe_workspace_bytes
        need = int(query(T, E, k, H, I, _lib.HYD_F16 if dtype == torch.float16 else _lib.HYD_BF16))
        ws = _workspaces[key] = torch.empty((max(need, 16),), dtype=torch.uint8, device=device)
    return ws


def _moe_call(x, logits, gate_up, down, scales, k, renormalize, out, ids_out, weights_out, workspace, grouped=False) -> Tensor:
    """moe_rows (scales None: 16-bit weights of x's dtype), moe_rows_grouped (the same with `grouped`: hyd_moe_mlp_grouped), moe_rows_w8 (scales = (gate_up_scale, down_scale): e4m3fn codes),
    moe_rows_grouped_w8 (the same with `grouped`: hyd_moe_mlp_grouped_w8) and
    moe_rows_w4 (scales = (gate_up_scale, down_scale, gate_up_shift, down_shift): packed e2m1 codes, two k per byte)."""
    from .flash import _require_gpu, _stream

    _require_gpu(x, logits, gate_up, down, out, ids_out, weights_out, workspace, *(scales or ()))
    fp4 = scales is not None and len(scales) == 4
    if fp4 and grouped:
        raise ValueError("4-bit experts have no grouped call")
    (T, H), E, I, per = x.shape, gate_up.shape[0], down.shape[2] * (2 if fp4 else 1), 2 if fp4 else 1  # per: k per element of the weights
    if scales is None:
        if not (x.dtype == logits.dtype == gate_up.dtype == down.dtype == out.dtype) or x.dtype not in (torch.float16, torch.bfloat16):
            raise TypeError("x, logits, gate_up, down and out must share one of float16 / bfloat16")
    else:
        if fp4:
            _check_experts4(gate_up, scales[2], scales[0], down, scales[3], scales[1])
        else:
            _check_experts8(gate_up, scales[0], down, scales[1])
        if not (x.dtype == logits.dtype == out.dtype) or x.dtype not in (torch.float16, torch.bfloat16):
            raise TypeError("x, logits and out must share one of float16 / bfloat16")
        if not all(s.is_contiguous() for s in scales):
            raise ValueError("gate_up_scale and down_scale" + (", gate_up_shift and down_shift" if fp4 else "") + " must be contiguous")
    if tuple(logits.shape) != (T, E) or tuple(gate_up.shape) != (E, 2 * I, H // per) or tuple(down.shape) != (E, H, I // per) or tuple(out.shape) != (T, H):
        raise ValueError(f"shapes: x {tuple(x.shape)}, logits {tuple(logits.shape)}, gate_up {tuple(gate_up.shape)}, down {tuple(down.shape)}, out {tuple(out.shape)}")
    if x.stride(1) != 1 or out.stride(1) != 1 or not (logits.is_contiguous() and gate_up.is_contiguous() and down.is_contiguous()):
        raise ValueError("x and out need a unit last stride; logits, gate_up and down must be contiguous")
    for name, t, dt in (("ids_out", ids_out, torch.int32), ("weights_out", weights_out, torch.float32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (T, k) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous [{T}, {k}] {dt} tensor")
    if workspace is None:
        workspace = _workspace(x.device, T, E, k, H, I, x.dtype, grouped)
    p = MoeParams() if scales is None else MoeW4Params() if fp4 else MoeW8Params()
    p.x, p.logits, p.gate_up, p.down, p.y = x.data_ptr(), logits.data_ptr(), gate_up.data_ptr(), down.data_ptr(), out.data_ptr()
    p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    p.ids_out = None if ids_out is None else ids_out.data_ptr()
    p.weights_out = None if weights_out is None else weights_out.data_ptr()
    p.x_row_stride, p.y_row_stride = (x.stride(0), out.stride(0)) if T > 1 else (H, H)  # (one row: the stride is never used)
    p.T, p.E, p.k, p.H, p.I, p.renormalize = T, E, k, H, I, int(bool(renormalize))
    p.dtype = _lib.HYD_F16 if x.dtype == torch.float16 else _lib.HYD_BF16
    if scales is None:
        _lib.check((_lib.load().hyd_moe_mlp_grouped if grouped else _lib.load().hyd_moe_mlp)(C.byref(p), _stream()))
        return out
    p.gate_up_scale, p.down_scale = scales[0].data_ptr(), scales[1].data_ptr()
    if fp4:
        p.gate_up_shift, p.down_shift = scales[2].data_ptr(), scales[3].data_ptr()
        _lib.check(_lib.load().hyd_moe_mlp_w4(C.byref(p), _stream()))
    else:
        _lib.check((_lib.load().hyd_moe_mlp_grouped_w8 if grouped else _lib.load().hyd_moe_mlp_w8)(C.byref(p), _stream()))
    return out


def moe_rows(x: Tensor, logits: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool, out: Tensor, ids_out: Optional[Tensor] = None,
             weights_out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """One hyd_moe_mlp call on the current stream: x [T, H] (T <= MOE_MAX_ROWS, unit last stride), logits [T, E] contiguous, into
    out [T, H] (unit last stride); ids_out int32 / weights_out float32 [T, k] receive the routing.  The C layer refuses what is
    out of range."""
    return _moe_call(x, logits, gate_up, down, None, k, renormalize, out, ids_out, weights_out, workspace)


def moe_rows_grouped(x: Tensor, logits: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool, out: Tensor, ids_out: Optional[Tensor] = None,
                     weights_out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """One hyd_moe_mlp_grouped call on the current stream: moe_rows for T <= MOE_GROUPED_MAX_ROWS rows, the slots sorted by expert
    and both products tiled through LDS, so that every chosen expert is read once.  The same routing and the same roundings as
    moe_rows; the fp32 sums inside the two products are added in another order.  Its workspace (hyd_moe_grouped_workspace_bytes) is
    cached per (device, shapes) like moe_rows'."""
    return _moe_call(x, logits, gate_up, down, None, k, renormalize, out, ids_out, weights_out, workspace, grouped=True)


def moe_rows_w8(x: Tensor, logits: Tensor, gate_up8: Tensor, gate_up_scale: Tensor, down8: Tensor, down_scale: Tensor, k: int, renormalize: bool,
                out: Tensor, ids_out: Optional[Tensor] = None, weights_out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """One hyd_moe_mlp_w8 call on the current stream: moe_rows on quantize_experts' four tensors (contiguous); x, logits and out
    stay 16-bit, the workspace is moe_rows'."""
    return _moe_call(x, logits, gate_up8, down8, (gate_up_scale, down_scale), k, renormalize, out, ids_out, weights_out, workspace)


def moe_rows_grouped_w8(x: Tensor, logits: Tensor, gate_up8: Tensor, gate_up_scale: Tensor, down8: Tensor, down_scale: Tensor, k: int, renormalize: bool,
                        out: Tensor, ids_out: Optional[Tensor] = None, weights_out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """One hyd_moe_mlp_grouped_w8 call on the current stream: moe_rows_grouped (T <= MOE_GROUPED_MAX_ROWS rows, every chosen expert
    read once) on quantize_experts' four tensors (contiguous).  The same routing and roundings as moe_rows_w8; the fp32 sums inside
    the two products are added in another order.  The workspace is moe_rows_grouped's, cached under the same key."""
    return _moe_call(x, logits, gate_up8, down8, (gate_up_scale, down_scale), k, renormalize, out, ids_out, weights_out, workspace, grouped=True)


def moe_rows_w4(x: Tensor, logits: Tensor, gate_up4: Tensor, gate_up_shift: Tensor, gate_up_scale: Tensor, down4: Tensor, down_shift: Tensor,
                down_scale: Tensor, k: int, renormalize: bool, out: Tensor, ids_out: Optional[Tensor] = None, weights_out: Optional[Tensor] = None,
                workspace: Optional[Tensor] = None) -> Tensor:
    """One hyd_moe_mlp_w4 call on the current stream: moe_rows on quantize_experts_fp4's six tensors (contiguous); x, logits and out
    stay 16-bit, the workspace is moe_rows'."""
    return _moe_call(x, logits, gate_up4, down4, (gate_up_scale, down_scale, gate_up_shift, down_shift), k, renormalize, out, ids_out, weights_out, workspace)


def moe_mlp(x: Tensor, router_w: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool, *, return_routing: bool = False,
            gate_up_scale: Optional[Tensor] = None, down_scale: Optional[Tensor] = None, gate_up_shift: Optional[Tensor] = None,
            down_shift: Optional[Tensor] = None, grouped: Optional[bool] = None):
    """The routed MLP of x [..., H]: logits = F.linear(x, router_w) in the 16-bit dtype, then one hyd_moe_mlp call per chunk of
    MOE_MAX_ROWS rows (rows are independent, so chunking is exact); 16-bit experts on MOE_GROUPED_MIN_ROWS rows and more take
    hyd_moe_mlp_grouped per chunk of MOE_GROUPED_MAX_ROWS rows instead (each expert read once per chunk).  The workspace is cached per (device, shapes): a captured graph
    replays without allocating it.  CPU tensors run the definition, rounded once to the dtype.  `return_routing`: (y, ids [T, k]
    int32, weights [T, k] float32).  With `gate_up_scale` and `down_scale` (both or neither), gate_up and down are quantize_experts'
    e4m3fn codes: hyd_moe_mlp_w8 per chunk, and on the CPU the definition on the dequantized weights.  With `gate_up_shift` and
    `down_shift` as well (both, and only with the scales), they are quantize_experts_fp4's packed e2m1 codes: hyd_moe_mlp_w4.
    `grouped`: None is the rule above (fp8 and 4-bit experts take the 128-row calls at every size); True takes the grouped call per
    chunk of MOE_GROUPED_MAX_ROWS rows at any T -- hyd_moe_mlp_grouped, or hyd_moe_mlp_grouped_w8 for fp8 experts; 4-bit experts
    have none: ValueError -- and False the 128-row calls at any T.  On the CPU the keyword changes nothing."""
    if (gate_up_scale is None) != (down_scale is None):
        raise ValueError("gate_up_scale and down_scale come together")
    if (gate_up_shift is None) != (down_shift is None) or (gate_up_shift is not None and gate_up_scale is None):
        raise ValueError("gate_up_shift and down_shift come together, and with gate_up_scale and down_scale")
    scales = None if gate_up_scale is None else (gate_up_scale, down_scale) if gate_up_shift is None else (gate_up_scale, down_scale, gate_up_shift, down_shift)
    x2 = x.reshape(-1, x.shape[-1])
    T = x2.shape[0]
    logits = nn.functional.linear(x2, router_w)
    if not x.is_cuda:
        if gate_up_shift is not None:
            gate_up, down = dequantize_experts_fp4(gate_up, gate_up_shift, gate_up_scale, down, down_shift, down_scale)
        elif scales is not None:
            gate_up, down = dequantize_experts(gate_up, gate_up_scale, down, down_scale)
        y = moe_reference(x2, router_w, gate_up, down, k, renormalize, logits=logits).to(x.dtype).view(x.shape)
        if not return_routing:
            return y
        ids, w = route_reference(logits, k, renormalize)
        return y, ids.int(), w.float()
    y = torch.empty_like(x2)
    ids = torch.empty((T, k), dtype=torch.int32, device=x.device) if return_routing else None
    w = torch.empty((T, k), dtype=torch.float32, device=x.device) if return_routing else None
    if grouped and gate_up_shift is not None:
        raise ValueError("grouped=True: 4-bit experts have no grouped call")
    if grouped is None:
        grouped = scales is None and T >= MOE_GROUPED_MIN_ROWS
    step = MOE_GROUPED_MAX_ROWS if grouped else MOE_MAX_ROWS
    for r in range(0, T, step):
        rows = slice(r, min(T, r + step))
        _moe_call(x2[rows], logits[rows], gate_up, down, scales, k, renormalize, y[rows], None if ids is None else ids[rows], None if w is None else w[rows], None,
                  grouped)
    y = y.view(x.shape)
    return (y, ids, w) if return_routing else y


class _Experts(nn.Module):
    def __init__(self, E: int, H: int, I: int):
        super().__init__()
        self.gate_up_proj = nn.Parameter(torch.empty(E, 2 * I, H))
        self.down_proj = nn.Parameter(torch.empty(E, H, I))


class Fp8Experts(nn.Module):
    """A layer's experts in fp8: buffers `gate_up_proj` e4m3fn [E, 2 I, H], `gate_up_proj_scale` float32 [E, 2 I], `down_proj`
    e4m3fn [E, H, I] and `down_proj_scale` float32 [E, H] (they travel in the state dict and are never trained).  `dtype` is the
    activation dtype the experts were quantized from."""

    def __init__(self, gate_up_proj: Tensor, gate_up_proj_scale: Tensor, down_proj: Tensor, down_proj_scale: Tensor, dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        _check_experts8(gate_up_proj, gate_up_proj_scale, down_proj, down_proj_scale)
        self.dtype = dtype
        for name, t in (("gate_up_proj", gate_up_proj), ("gate_up_proj_scale", gate_up_proj_scale), ("down_proj", down_proj), ("down_proj_scale", down_proj_scale)):
            self.register_buffer(name, t.contiguous())

    @classmethod
    def from_experts(cls, experts: nn.Module) -> "Fp8Experts":
        return cls(*quantize_experts(experts.gate_up_proj, experts.down_proj), dtype=experts.gate_up_proj.dtype)

    def _apply(self, fn, recurse=True):
        """`.to(device)` moves the buffers as they are.  A floating-point cast (`.half()`, `.to(dtype)`) would turn the codes and
        the scales into 16-bit values: they keep their formats, and the cast sets the activation dtype instead (Fp8Linear's rule)."""
        kept = {n: b for n, b in self.named_buffers(recurse=False)}
        super()._apply(fn, recurse)
        if self.gate_up_proj.dtype != FP8_DTYPE:
            self.dtype = self.gate_up_proj.dtype
        for n, b in kept.items():
            if getattr(self, n).dtype != b.dtype:
                setattr(self, n, b.to(getattr(self, n).device))
        return self

    def extra_repr(self) -> str:
        return f"experts={self.gate_up_proj.shape[0]}, hidden={self.down_proj.shape[1]}, intermediate={self.down_proj.shape[2]}, fp8 weights for {self.dtype}"


class Fp4Experts(nn.Module):
    """A layer's experts in 4 bits: buffers `gate_up_proj` uint8 [E, 2 I, H / 2], `gate_up_proj_shift` uint8 [E, 2 I, H / 32],
    `gate_up_proj_scale` float32 [E, 2 I], `down_proj` uint8 [E, H, I / 2], `down_proj_shift` uint8 [E, H, I / 32] and
    `down_proj_scale` float32 [E, H] (they travel in the state dict and are never trained).  `dtype` is the activation dtype the
    experts were quantized from."""

    NAMES = ("gate_up_proj", "gate_up_proj_shift", "gate_up_proj_scale", "down_proj", "down_proj_shift", "down_proj_scale")

    def __init__(self, gate_up_proj: Tensor, gate_up_proj_shift: Tensor, gate_up_proj_scale: Tensor, down_proj: Tensor, down_proj_shift: Tensor,
                 down_proj_scale: Tensor, dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        bufs = (gate_up_proj, gate_up_proj_shift, gate_up_proj_scale, down_proj, down_proj_shift, down_proj_scale)
        _check_experts4(*bufs)
        self.dtype = dtype
        for name, t in zip(self.NAMES, bufs):
            self.register_buffer(name, t.contiguous())

    @classmethod
    def from_experts(cls, experts: nn.Module) -> "Fp4Experts":
        return cls(*quantize_experts_fp4(experts.gate_up_proj, experts.down_proj), dtype=experts.gate_up_proj.dtype)

    def _apply(self, fn, recurse=True):
        """Fp8Experts' rule: `.to(device)` moves the buffers as they are; a floating-point cast reaches the scales only (codes and
        shifts are integers), is taken as the new activation dtype and undone on the buffers."""
        kept = {n: b for n, b in self.named_buffers(recurse=False)}
        super()._apply(fn, recurse)
        if self.gate_up_proj_scale.dtype != torch.float32:
            self.dtype = self.gate_up_proj_scale.dtype
        for n, b in kept.items():
            if getattr(self, n).dtype != b.dtype:
                setattr(self, n, b.to(getattr(self, n).device))
        return self

    def extra_repr(self) -> str:
        return f"experts={self.gate_up_proj.shape[0]}, hidden={self.down_proj.shape[1]}, intermediate={2 * self.down_proj.shape[2]}, e2m1 weights for {self.dtype}"


class MoeMLP(nn.Module):
    """A decoder layer's routed MLP under transformers 5's parameter names and layouts (`gate.weight` [E, H],
    `experts.gate_up_proj` [E, 2 I, H], `experts.down_proj` [E, H, I]: Mixtral's and Qwen3-MoE's alike under `model.layers.N.mlp.`).
    `experts` holds the 16-bit parameters, or an Fp8Experts / Fp4Experts after HydragenLlamaForCausalLM.quantize_experts()."""

    def __init__(self, hidden_size: int, intermediate_size: int, num_experts: int, top_k: int, renormalize: bool):
        super().__init__()
        self.gate = nn.Linear(hidden_size, num_experts, bias=False)
        self.experts = _Experts(num_experts, hidden_size, intermediate_size)
        self.top_k, self.renormalize = top_k, renormalize

    def forward(self, x: Tensor) -> Tensor:
        e = self.experts
        scales = dict(gate_up_scale=e.gate_up_proj_scale, down_scale=e.down_proj_scale) if isinstance(e, (Fp8Experts, Fp4Experts)) else {}
        if isinstance(e, Fp4Experts):
            scales.update(gate_up_shift=e.gate_up_proj_shift, down_shift=e.down_proj_shift)
        rows = x.numel() // x.shape[-1]
        grouped = True if isinstance(e, Fp8Experts) and MOE_GROUPED_W8_MIN_ROWS is not None and rows >= MOE_GROUPED_W8_MIN_ROWS else None
        return moe_mlp(x, self.gate.weight, e.gate_up_proj, e.down_proj, self.top_k, self.renormalize, grouped=grouped, **scales)
