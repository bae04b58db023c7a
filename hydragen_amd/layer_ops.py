"""Python face of `hyd_add_rmsnorm` / `hyd_swiglu` / `hyd_sample_tokens[_filtered]` / `hyd_token_logprobs` (include/hydragen_hip.h): the elementwise glue of the decoder layer
around the attention block -- residual add + RMSNorm (/root/reference/hydragen/llama.py:615-631 with transformers'
LlamaRMSNorm, llama.py:605-608,656) and the SwiGLU gate (transformers' LlamaMLP, llama.py:2,604) -- each as one
HIP kernel instead of two torch launches."""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import AddRmsnormParams, SwigluParams
from .flash import _dtype_code, _require_gpu, _stream
from .sampling import check_filters, filters_active
from .scoring import check_top_n, token_logprobs_reference


def supported(x: Tensor, n_max: int = 16384) -> bool:
    """Shapes the kernels take: 16-bit CUDA rows, contiguous in the last dimension, a multiple of 8 wide, every row
    16-byte aligned (what the C entry points check); anything else takes the torch form in the model shell."""
    return (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.shape[-1] % 8 == 0 and x.shape[-1] <= n_max
            and x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and all(st % 8 == 0 for st in x.stride()[:-1]))


def _rows(t: Tensor) -> Tensor:
    """[..., n] -> [rows, n] view with one row stride (no copy for the views the model shell produces)."""
    return t.reshape(-1, t.shape[-1])


def add_rms_norm(x: Tensor, residual: Optional[Tensor], weight: Tensor, eps: float):
    """(residual + x, RMSNorm(residual + x) * weight); residual None: (x, RMSNorm(x) * weight).  The sum is rounded to
    x.dtype before the statistic is taken (it is the stored residual stream); the norm is fp32 inside, one rounding."""
    _require_gpu(x, weight)
    lib = _lib.load()
    x2 = _rows(x)
    n = x2.shape[1]
    assert x2.stride(1) == 1 and n % 8 == 0 and weight.shape == (n,) and weight.dtype == x.dtype and weight.is_contiguous()
    normed = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if x2.shape[0] == 0:
        return (x if residual is None else torch.empty_like(normed)), normed
    p = AddRmsnormParams()
    p.x, p.weight, p.norm_out = x2.data_ptr(), weight.data_ptr(), normed.data_ptr()
    p.x_row_stride, p.norm_row_stride = x2.stride(0) if x2.shape[0] > 1 else n, n
    summed = x
    if residual is not None:
        _require_gpu(residual)
        r2 = _rows(residual)
        assert r2.shape == x2.shape and r2.dtype == x.dtype and r2.stride(1) == 1
        summed = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        p.residual, p.sum_out = r2.data_ptr(), summed.data_ptr()
        p.residual_row_stride, p.sum_row_stride = r2.stride(0) if r2.shape[0] > 1 else n, n
    p.rows, p.n, p.dtype, p.eps = x2.shape[0], n, _dtype_code(x), float(eps)
    _lib.check(lib.hyd_add_rmsnorm(C.byref(p), _stream()))
    return summed, normed


def swiglu(gate: Tensor, up: Tensor) -> Tensor:
    """silu(gate) * up; gate / up [..., n] may be the column halves of one fused GEMM output (row-strided views)."""
    _require_gpu(gate, up)
    lib = _lib.load()
    g2, u2 = _rows(gate), _rows(up)
    n = g2.shape[1]
    assert g2.shape == u2.shape and gate.dtype == up.dtype and g2.stride(1) == 1 and u2.stride(1) == 1 and n % 8 == 0
    out = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
    if g2.shape[0] == 0:
        return out
    p = SwigluParams()
    p.gate, p.up, p.out = g2.data_ptr(), u2.data_ptr(), out.data_ptr()
    one = g2.shape[0] <= 1
    p.gate_row_stride, p.up_row_stride, p.out_row_stride = (n if one else g2.stride(0)), (n if one else u2.stride(0)), n
    p.rows, p.n, p.dtype = g2.shape[0], n, _dtype_code(gate)
    _lib.check(lib.hyd_swiglu(C.byref(p), _stream()))
    return out


_HYD_F32 = 2


def _next_sample_key(device: torch.device):
    """(seed, offset) of the next sampling call, taken from -- and advancing -- torch's CUDA generator of the device: the
    draw is a function of torch.manual_seed and of the random ops issued since, like torch.multinomial's (the reference
    seeds every tensor-parallel rank alike so that all ranks draw the same tokens, tp.py:178)."""
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    seed, offset = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, gen.get_offset()
    gen.set_offset(offset + 4)
    return seed, offset


def sample_tokens(logits: Tensor, temperature: float, key: Optional[tuple] = None, *, top_k: Optional[int] = None,
                  top_p: Optional[float] = None, min_p: Optional[float] = None, return_logprobs: bool = False):
    """[B, V] logits (fp16 / bf16 / fp32, rows contiguous) -> [B, 1] int64 tokens drawn from softmax(logits / temperature)
    (temperature 0: argmax) in one kernel.  top_k / top_p / min_p cut the UNSCALED softmax(logits) first (hydragen_amd/
    sampling.py states the rules); return_logprobs also returns the [B, 1] fp32 log softmax(logits) of each drawn token.
    With no cut and no log-prob this is hyd_sample_tokens; otherwise hyd_sample_tokens_filtered, whose draw uses the same
    noise (one key per call either way)."""
    if not filters_active(top_k, top_p, min_p) and not return_logprobs:
        _require_gpu(logits)
        lib = _lib.load()
        assert logits.ndim == 2 and logits.stride(1) == 1 and logits.shape[1] > 0
        out = torch.empty((logits.shape[0], 1), dtype=torch.int64, device=logits.device)
        if logits.shape[0] == 0:
            return out
        seed, offset = key if key is not None else _next_sample_key(logits.device)
        p = _lib.SampleParams()
        p.logits, p.out, p.row_stride = logits.data_ptr(), out.data_ptr(), logits.stride(0) if logits.shape[0] > 1 else logits.shape[1]
        p.seed, p.offset, p.rows, p.n = seed, offset, logits.shape[0], logits.shape[1]
        p.dtype = _HYD_F32 if logits.dtype == torch.float32 else _dtype_code(logits)
        p.temperature = float(temperature)
        _lib.check(lib.hyd_sample_tokens(C.byref(p), _stream()))
        return out
    tok, lp, _ = sample_tokens_filtered(logits, temperature, key, top_k=top_k, top_p=top_p, min_p=min_p)
    return (tok, lp[:, None]) if return_logprobs else tok


def sample_tokens_filtered(logits: Tensor, temperature: float, key: Optional[tuple] = None, *, top_k: Optional[int] = None,
                           top_p: Optional[float] = None, min_p: Optional[float] = None):
    """hyd_sample_tokens_filtered: ([B, 1] int64 tokens, [B] fp32 log-probs, [B] int32 number of kept tokens)."""
    _require_gpu(logits)
    lib = _lib.load()
    assert logits.ndim == 2 and logits.stride(1) == 1 and logits.shape[1] > 0
    rows = logits.shape[0]
    out = torch.empty((rows, 1), dtype=torch.int64, device=logits.device)
    logprobs = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    kept = torch.empty((rows,), dtype=torch.int32, device=logits.device)
    if rows == 0:
        return out, logprobs, kept
    check_filters(top_k, top_p, min_p)  # (before the key is taken: a rejected call leaves the generator as it was)
    p = _lib.SampleFilterParams()
    p.top_k, p.top_p, p.min_p = int(top_k or 0), 1.0 if top_p is None else float(top_p), float(min_p or 0.0)
    seed, offset = key if key is not None else _next_sample_key(logits.device)
    p.logits, p.out, p.logprobs, p.kept = logits.data_ptr(), out.data_ptr(), logprobs.data_ptr(), kept.data_ptr()
    p.row_stride = logits.stride(0) if rows > 1 else logits.shape[1]
    p.seed, p.offset, p.rows, p.n = seed, offset, rows, logits.shape[1]
    p.dtype = _HYD_F32 if logits.dtype == torch.float32 else _dtype_code(logits)
    p.temperature = float(temperature)
    _lib.check(lib.hyd_sample_tokens_filtered(C.byref(p), _stream()))
    return out, logprobs, kept


def token_logprobs(logits: Tensor, targets: Tensor, top_n: int = 0):
    """hyd_token_logprobs, one launch: [R, V] logits (fp16 / bf16 / fp32, unit last stride) and [R] int64 targets ->
    (logprobs [R] f32, greedy [R] bool, top_ids [R, top_n] int64, top_logprobs [R, top_n] f32); hydragen_amd/scoring.py states
    the definition.  Targets outside [0, V) mark padding rows (NaN, not greedy).  Shapes and dtypes are checked on the host;
    nothing synchronises.  CPU tensors take scoring.token_logprobs_reference."""
    top_n = check_top_n(top_n)
    if logits.ndim != 2 or logits.shape[1] <= 0 or logits.stride(1) != 1:
        raise ValueError(f"logits must be [R, V] with V > 0 and a unit last stride, got {tuple(logits.shape)} / {logits.stride()}")
    if logits.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"logits dtype {logits.dtype}: float16, bfloat16 or float32")
    if targets.shape != (logits.shape[0],) or targets.dtype != torch.int64 or targets.device != logits.device:
        raise ValueError(f"targets must be [{logits.shape[0]}] int64 on {logits.device}, got {tuple(targets.shape)} {targets.dtype} "
                         f"on {targets.device}")
    if logits.shape[1] > _lib.SAMPLE_FILTER_MAX_N:
        raise ValueError(f"rows of {logits.shape[1]} logits: at most {_lib.SAMPLE_FILTER_MAX_N}")
    if not logits.is_cuda:
        return token_logprobs_reference(logits, targets, top_n)
    _require_gpu(logits)
    lib = _lib.load()
    rows, n = logits.shape
    dev = logits.device
    lp = torch.empty((rows,), dtype=torch.float32, device=dev)
    greedy = torch.empty((rows,), dtype=torch.uint8, device=dev)
    top_ids = torch.empty((rows, top_n), dtype=torch.int64, device=dev)
    top_lp = torch.empty((rows, top_n), dtype=torch.float32, device=dev)
    if rows > 0:
        t = targets.contiguous()
        p = _lib.TokenLogprobParams()
        p.logits, p.dtype, p.n, p.rows = logits.data_ptr(), _HYD_F32 if logits.dtype == torch.float32 else _dtype_code(logits), n, rows
        p.row_stride = logits.stride(0) if rows > 1 else n
        p.targets, p.logprobs, p.greedy, p.top_n = t.data_ptr(), lp.data_ptr(), greedy.data_ptr(), top_n
        if top_n:
            p.top_ids, p.top_logprobs = top_ids.data_ptr(), top_lp.data_ptr()
        _lib.check(lib.hyd_token_logprobs(C.byref(p), _stream()))
    return lp, greedy.view(torch.bool), top_ids, top_lp
