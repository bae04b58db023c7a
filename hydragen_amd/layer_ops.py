"""Python face of `hyd_add_rmsnorm` / `hyd_swiglu` / `hyd_sample_tokens[_filtered | _rows]` / `hyd_token_logprobs` / `hyd_stop_update[_rows]` (include/hydragen_hip.h): the elementwise glue of the decoder layer
around the attention block -- residual add + RMSNorm (/root/reference/hydragen/llama.py:615-631 with transformers'
LlamaRMSNorm, llama.py:605-608,656) and the SwiGLU gate (transformers' LlamaMLP, llama.py:2,604) -- each as one
HIP kernel instead of two torch launches."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import AddRmsnormParams, SwigluParams
from .flash import _dtype_code, _require_gpu, _stream
from . import sampling, stopping
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


def _draw_outputs(logits: Tensor, stats: bool) -> tuple:
    """What every sampling entry point starts with: the rows it takes, and its outputs -- ([B, 1] int64 tokens,) and, with
    `stats`, ([B] fp32 log-probs, [B] int32 kept counts) behind them."""
    _require_gpu(logits)
    _lib.load()
    assert logits.ndim == 2 and logits.stride(1) == 1 and logits.shape[1] > 0
    rows, dev = logits.shape[0], logits.device
    out = torch.empty((rows, 1), dtype=torch.int64, device=dev)
    if not stats:
        return (out,)
    return out, torch.empty((rows,), dtype=torch.float32, device=dev), torch.empty((rows,), dtype=torch.int32, device=dev)


def _fill_rows(p, logits: Tensor, outs: tuple, temperature: float, key: Optional[tuple], top_k=None, top_p=None, min_p=None):
    """The logits-row header the three sampling structs share, and the cut fields of the two whose outputs have stats.  It takes
    the call's key, so it comes after every check: a rejected call leaves the generator as it was."""
    rows, n = logits.shape
    p.logits, p.out, p.row_stride = logits.data_ptr(), outs[0].data_ptr(), logits.stride(0) if rows > 1 else n
    p.seed, p.offset = key if key is not None else _next_sample_key(logits.device)
    p.rows, p.n, p.temperature = rows, n, float(temperature)
    p.dtype = _HYD_F32 if logits.dtype == torch.float32 else _dtype_code(logits)
    if len(outs) > 1:
        p.logprobs, p.kept = outs[1].data_ptr(), outs[2].data_ptr()
        p.top_k, p.top_p, p.min_p = int(top_k or 0), 1.0 if top_p is None else float(top_p), float(min_p or 0.0)


def row_array(v, rows: int, device, dtype, off, what: str = "value") -> Optional[Tensor]:
    """A per-row sampling argument as the [rows] device array hyd_sample_tokens_rows reads, or None for a scalar (which stays
    in the parameter block).  Lists / tuples (None inside = `off`) and tensors of 1 or `rows` entries are taken; a tensor that
    already is a contiguous [rows] array of `dtype` on the device is passed as it is (generate() uploads its arrays once per
    call).  Nothing synchronises."""
    if not sampling.is_per_row(v):
        return None
    if isinstance(v, Tensor):
        t = v.reshape(-1)
        if dtype == torch.int64 and t.dtype == torch.uint64:
            t = t.view(torch.int64)
        t = t.to(device=device, dtype=dtype)
    else:
        vals = [off if x is None else x for x in v]
        if dtype == torch.int64:  # seeds: 64 bits, carried as their two's-complement pattern
            vals = [((int(x) & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)) - (1 << 63) for x in vals]
        t = torch.tensor(vals, dtype=dtype).to(device)
    if t.numel() == 1 and rows != 1:
        t = t.expand(rows)
    if t.shape != (rows,):
        raise ValueError(f"{what}: {t.numel()} per-row values for {rows} rows")
    return t.contiguous()


ROW_FIELDS = (("temperature", torch.float32, 0.0), ("top_k", torch.int32, 0), ("top_p", torch.float32, 1.0), ("min_p", torch.float32, 0.0),
              ("repetition_penalty", torch.float32, 1.0), ("frequency_penalty", torch.float32, 0.0), ("presence_penalty", torch.float32, 0.0))


def _scalar_or(v, off):
    """What goes into the parameter block's scalar: the value, or `off` where an array overrides it (the entry point checks the
    scalars whatever the arrays are)."""
    return off if v is None or sampling.is_per_row(v) else v


@dataclass
class Penalties:
    """What sampling.py's penalty definition needs for a batch of rows: the scalars, the bias list as (ids int64 [K], values fp32
    [K]) tensors on the logits' device, the context bitmaps [(bits int32 [groups, ceil(V / 32)], rows_per_group)], and the rows'
    generated tokens gen int32 [B, stride] with their device-side lengths gen_len int32 [B].  append: the kernel stores each
    drawn token behind the row's list (hyd_sample_penalty_params.append_out); the torch route does the same with two small
    launches, so either way the list follows the draws without a host sync."""
    repetition_penalty: Optional[float] = None
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    logit_bias: Optional[tuple] = None
    context: list = field(default_factory=list)
    gen: Optional[Tensor] = None
    gen_len: Optional[Tensor] = None
    append: bool = False

    def active(self) -> bool:
        return sampling.penalties_active(self.repetition_penalty, self.presence_penalty, self.frequency_penalty, self.logit_bias)

    def per_row(self) -> bool:
        """One of the three scalars is a list or a tensor of per-row values."""
        return any(sampling.is_per_row(v) for v in (self.repetition_penalty, self.presence_penalty, self.frequency_penalty))

    def apply(self, logits: Tensor, rows_per_sample: int = 1) -> Tensor:
        """sampling.penalize_logits of these penalties (float64).  rows_per_sample = s > 1: `logits` holds one row for every s
        consecutive rows of the batch (the fan-out first token: the samples of a leaf share its context and have generated
        nothing yet)."""
        ctx = self.context
        gen, gen_len = self.gen, self.gen_len
        if rows_per_sample > 1:
            if any(k % rows_per_sample for _, k in ctx):
                raise ValueError(f"context groups do not nest in {rows_per_sample} samples per row")
            ctx = [(b, k // rows_per_sample) for b, k in ctx]
            gen = gen_len = None
        return sampling.penalize_logits(logits, self.repetition_penalty, self.presence_penalty, self.frequency_penalty,
                                        self.logit_bias, ctx, gen, gen_len)

    def push(self, tokens: Tensor) -> None:
        """Append one token per row ([B, 1] or [B]) to gen / gen_len: two small launches, no sync."""
        t = tokens.reshape(-1, 1).to(torch.int32)
        pos = self.gen_len.long().clamp_(max=self.gen.shape[1] - 1)[:, None]
        self.gen.scatter_(1, pos, torch.where(self.gen_len[:, None] < self.gen.shape[1], t, self.gen.gather(1, pos)))
        self.gen_len += 1


def token_bitmap(ids: Tensor, lens: Optional[Tensor], n: int, out: Optional[Tensor] = None) -> Tensor:
    """hyd_token_bitmap_build: [groups, L] int64 token ids (+ [groups] lengths, None = all L) -> presence bitmap int32
    [groups, ceil(n / 32)] (bit v % 32 of word v // 32 = token v occurs), one launch and no [groups, n] table.  out: OR into an
    existing bitmap instead of a zeroed one.  CPU tensors take sampling.token_bitmap_reference."""
    if ids.ndim != 2 or ids.dtype != torch.int64:
        raise ValueError(f"ids must be [groups, L] int64, got {tuple(ids.shape)} {ids.dtype}")
    groups, L = ids.shape
    if lens is not None and (lens.numel() != groups or lens.device != ids.device):
        raise ValueError(f"lens must hold {groups} lengths on {ids.device}")
    words = (n + 31) // 32
    if not ids.is_cuda:
        ref = sampling.token_bitmap_reference(ids, lens, n)
        return ref if out is None else out.bitwise_or_(ref)
    _require_gpu(ids)
    lib = _lib.load()
    bits = torch.zeros((groups, words), dtype=torch.int32, device=ids.device) if out is None else out
    assert bits.shape == (groups, words) and bits.dtype == torch.int32 and bits.is_contiguous()
    if ids.stride(1) != 1:
        ids = ids.contiguous()
    p = _lib.TokenBitmapParams()
    p.ids, p.bits, p.id_stride = ids.data_ptr(), bits.data_ptr(), ids.stride(0) if groups > 1 else L
    if lens is not None:
        lens = lens.reshape(-1).to(torch.int64).contiguous()
        p.lens = lens.data_ptr()
    p.groups, p.L, p.n = groups, L, n
    _lib.check(lib.hyd_token_bitmap_build(C.byref(p), _stream()))
    return bits


def sample_tokens_penalized(logits: Tensor, temperature, key: Optional[tuple] = None, *, penalties: Penalties,
                            top_k=None, top_p=None, min_p=None, constraint: Optional[tuple] = None, seed=None,
                            drafts: Optional[Tensor] = None):
    """hyd_sample_tokens_penalized, one launch whatever the penalties are (neutral ones included): ([B, 1] int64 tokens, [B] fp32
    log-probs under softmax(penalised logits), [B] int32 number of kept tokens).  hydragen_amd/sampling.py states the
    definition.  Nothing of size [B, V] is allocated and nothing synchronises; the bias list must already be checked
    (sampling.check_penalties) and on the device.  constraint = (dfa, state int32 [B], advance): hyd_sample_tokens_constrained
    instead -- the same launch behind the automaton's mask (sample_tokens_constrained).
    temperature, top_k, top_p, min_p and the penalties' three scalars may each be PER ROW (a list with None = off, or a tensor of
    [B] entries; sampling.py), and seed= one integer per row: hyd_sample_tokens_rows, one launch, each row bit for bit what a
    scalar call with its values returns for it.  Per-row values reach the kernel as fp32 (top_k int32); they are checked on
    the host only where they are host values (lists), the kernel sanitises what it reads (include/hydragen_hip.h).  With seed=
    row r's noise is that of row 0 of a call with key = (seed[r], offset): its draw does not depend on its place in the batch,
    and the device's generator is not advanced (key = (anything, offset); None: offset 0).
    drafts = fed int64 [B, T] (contiguous, on the device): hyd_sample_tokens_penalized_drafts -- the logits are the B * T rows of a
    speculative step, penalties.gen / gen_len hold ONE list per sequence ([B, stride] / [B]), the context bitmaps cover B rows, and
    the row behind fed[b, i] also counts the drafts fed[b, 1 .. i] (sampling.draft_row_lists_reference).  The sampler never
    appends on this route, and neither per-row values nor a constraint are carried."""
    outs = _draw_outputs(logits, stats=True)
    rows, n = logits.shape
    dev, pen = logits.device, penalties
    if rows == 0:
        return outs
    T = 1
    if drafts is not None:
        if (drafts.dtype != torch.int64 or drafts.ndim != 2 or not drafts.is_contiguous() or drafts.device != dev
                or not 1 <= drafts.shape[1] <= 8 or drafts.numel() != rows):
            raise ValueError(f"drafts must be the step's fed tokens, a contiguous int64 [B, T <= 8] with B * T = {rows} on {dev}, got "
                             f"{tuple(drafts.shape)} {drafts.dtype}")
        if constraint is not None or seed is not None or pen.append:
            raise NotImplementedError("drafts= with a constraint, per-row seeds or an appending Penalties: "
                                      "hyd_sample_tokens_penalized_drafts carries none of them")
        T = drafts.shape[1]
    seqs = rows // T
    check_filters(top_k, top_p, min_p)
    p = _lib.SamplePenaltyParams()
    words = (n + 31) // 32
    if len(pen.context) > _lib.SAMPLE_MAX_CONTEXT:
        raise ValueError(f"{len(pen.context)} context bitmaps: at most {_lib.SAMPLE_MAX_CONTEXT}")
    for i, (bits, rpg) in enumerate(pen.context):
        if (bits.dtype != torch.int32 or bits.ndim != 2 or bits.shape[1] != words or not bits.is_contiguous() or bits.device != dev
                or rpg <= 0 or bits.shape[0] * rpg < seqs):
            raise ValueError(f"context bitmap {i}: int32 [groups, {words}] on {dev} with groups * rows_per_group >= {seqs}, got "
                             f"{tuple(bits.shape)} {bits.dtype} x {rpg}")
        p.context[i].bits, p.context[i].rows_per_group = bits.data_ptr(), int(rpg)
    p.n_context = len(pen.context)
    if pen.gen is not None:
        g, gl = pen.gen, pen.gen_len
        if (g.dtype != torch.int32 or g.ndim != 2 or g.shape[0] != seqs or not g.is_contiguous() or g.device != dev
                or gl is None or gl.dtype != torch.int32 or gl.shape != (seqs,) or gl.device != dev or not gl.is_contiguous()):
            raise ValueError(f"gen must be int32 [{seqs}, stride] and gen_len int32 [{seqs}], contiguous on {dev}")
        if g.shape[1] > _lib.SAMPLE_GEN_MAX:
            raise NotImplementedError(f"{g.shape[1]} generated tokens per row: the kernel counts up to {_lib.SAMPLE_GEN_MAX}")
        p.gen, p.gen_len, p.gen_stride = g.data_ptr(), gl.data_ptr(), g.shape[1]
        p.append_out = int(pen.append)
    elif pen.append:
        raise ValueError("append needs gen and gen_len")
    if pen.logit_bias is not None:
        ids, values = pen.logit_bias
        if (ids.dtype != torch.int64 or values.dtype != torch.float32 or ids.shape != values.shape or ids.ndim != 1
                or ids.device != dev or values.device != dev or not ids.is_contiguous() or not values.is_contiguous()):
            raise ValueError(f"logit_bias must be (ids int64 [K], values fp32 [K]) on {dev}: sampling.normalize_logit_bias")
        p.bias_ids, p.bias_values, p.n_bias = ids.data_ptr(), values.data_ptr(), ids.numel()
    given = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, repetition_penalty=pen.repetition_penalty,
                 frequency_penalty=pen.frequency_penalty, presence_penalty=pen.presence_penalty)
    arrays = [row_array(given[name], rows, dev, dtype, off, name) for name, dtype, off in ROW_FIELDS]
    arrays.append(row_array(seed, rows, dev, torch.int64, 0, "seed"))
    per_row = any(a is not None for a in arrays)
    if per_row and drafts is not None:
        raise NotImplementedError("drafts= with per-row sampling values: hyd_sample_tokens_penalized_drafts takes scalars")
    p.repetition_penalty = float(_scalar_or(pen.repetition_penalty, 1.0))
    p.frequency_penalty, p.presence_penalty = float(_scalar_or(pen.frequency_penalty, 0.0)), float(_scalar_or(pen.presence_penalty, 0.0))
    if seed is not None and key is None:
        key = (0, 0)
    _fill_rows(p, logits, outs, _scalar_or(temperature, 0.0), key, _scalar_or(top_k, 0), _scalar_or(top_p, 1.0), _scalar_or(min_p, 0.0))
    c = None
    if constraint is not None:
        dfa, state, advance = constraint
        c = _lib.TokenDfa()
        c.allowed, c.next, c.state = dfa.allowed.data_ptr(), dfa.next.data_ptr(), state.data_ptr()
        c.allowed_stride, c.next_stride, c.n_states, c.advance = dfa.allowed.shape[1], n, dfa.next.shape[0], int(bool(advance))
    if drafts is not None:
        _lib.check(_lib.load().hyd_sample_tokens_penalized_drafts(C.byref(p), drafts.data_ptr(), T, _stream()))
    elif per_row:
        _lib.check(_lib.load().hyd_sample_tokens_rows(C.byref(p), None if c is None else C.byref(c),
                                                     *(None if a is None else a.data_ptr() for a in arrays), _stream()))
    elif c is None:
        _lib.check(_lib.load().hyd_sample_tokens_penalized(C.byref(p), _stream()))
    else:
        _lib.check(_lib.load().hyd_sample_tokens_constrained(C.byref(p), C.byref(c), _stream()))
    return outs


def sample_tokens_constrained(logits: Tensor, temperature: float, key: Optional[tuple] = None, *, constraint: tuple,
                              penalties: Optional[Penalties] = None, top_k=None, top_p=None, min_p=None, seed=None):
    """hyd_sample_tokens_constrained, one launch: sample_tokens_penalized (penalties None: neutral ones, which is
    sample_tokens_filtered) on the logits with the tokens that a row's automaton state does not allow at -inf -- bit for bit --
    without a [B, V] mask.  constraint = (dfa, state, advance): dfa a constraint.TokenDFA on the logits' device, state int32 [B]
    on the device (rows outside [0, S) are unconstrained); advance: state[row] = next[state[row], token] after the draw, in place.
    hydragen_amd/sampling.py states the definition.  Returns ([B, 1] int64 tokens, [B] fp32 log-probs of the constrained
    distribution, [B] int32 kept counts).  Per-row values and seed=: as sample_tokens_penalized."""
    dfa, state, _ = constraint
    sampling.check_constraint(dfa, logits.shape[-1], logits.shape[0], state)
    if dfa.next.device != logits.device or state.device != logits.device:
        raise ValueError(f"constraint: the automaton is on {dfa.next.device}, the state on {state.device}, the logits on {logits.device}")
    return sample_tokens_penalized(logits, temperature, key, penalties=Penalties() if penalties is None else penalties, top_k=top_k,
                                   top_p=top_p, min_p=min_p, constraint=constraint, seed=seed)


def sample_tokens(logits: Tensor, temperature, key: Optional[tuple] = None, *, top_k=None, top_p=None, min_p=None,
                  return_logprobs: bool = False, penalties: Optional[Penalties] = None, constraint: Optional[tuple] = None,
                  seed=None, drafts: Optional[Tensor] = None):
    """[B, V] logits (fp16 / bf16 / fp32, rows contiguous) -> [B, 1] int64 tokens drawn from softmax(logits / temperature)
    (temperature 0: argmax) in one kernel.  top_k / top_p / min_p cut the UNSCALED softmax(logits) first (hydragen_amd/
    sampling.py states the rules); return_logprobs also returns the [B, 1] fp32 log softmax(logits) of each drawn token.
    Which entry point that is, sampling.sample_route says (these rows count as eligible: the kernels check their layout):
    hyd_sample_tokens with no cut and no log-prob; otherwise hyd_sample_tokens_filtered, whose draw uses the same noise (one
    key per call either way).  penalties (a Penalties with something switched on): hyd_sample_tokens_penalized; the log-prob is
    then log softmax(penalised logits), the distribution the draw's policy is defined by.  constraint = (dfa, state, advance)
    (sample_tokens_constrained): hyd_sample_tokens_constrained, which also advances `state` in place.  CPU logits with
    penalties or a constraint: their float64 definition in torch (no HIP kernel takes CPU tensors).  constraint None or
    neutral penalties: exactly the calls made without them.
    Per-row values (temperature, the cuts, the penalties' scalars as lists or [B] tensors) or seed= (one integer per row):
    sample_route's per_row routes -- always a kernel on GPU rows, through hyd_sample_tokens_rows (sample_tokens_penalized says
    what a row then returns); CPU rows: the per-row definition, sampling.reference_draw.
    drafts = fed int64 [B, T]: the rows are the B * T logits rows of a speculative step and active penalties hold one list per
    sequence -- hyd_sample_tokens_penalized_drafts (sample_tokens_penalized); without active penalties drafts changes nothing."""
    pen = penalties if penalties is not None and penalties.active() else None
    if drafts is not None and pen is not None:
        if not logits.is_cuda or constraint is not None:
            raise NotImplementedError("drafts= with penalties: GPU rows without a constraint (hyd_sample_tokens_penalized_drafts)")
        tok, lp, _ = sample_tokens_penalized(logits, temperature, key, penalties=pen, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed,
                                             drafts=drafts)
        return (tok, lp[:, None]) if return_logprobs else tok
    cuts = dict(top_k=top_k, top_p=top_p, min_p=min_p)
    per_row = seed is not None or any(sampling.is_per_row(v) for v in (temperature, top_k, top_p, min_p)) or (pen is not None and pen.per_row())
    draw = sampling.sample_route(logits.is_cuda, True, True, 1, constraint is not None, pen is not None,
                                 filters_active(top_k, top_p, min_p), return_logprobs, per_row=per_row).draw
    if per_row and not logits.is_cuda:
        draw = sampling.CONSTRAINED if constraint is not None else sampling.PENALIZED  # CPU rows: the definition in torch, below
    if per_row and logits.is_cuda:
        tok, lp, _ = sample_tokens_penalized(logits, temperature, key, penalties=Penalties() if pen is None else pen,
                                             constraint=constraint if draw == sampling.CONSTRAINED else None, seed=seed, **cuts)
        return (tok, lp[:, None]) if return_logprobs else tok
    if draw == sampling.PLAIN:
        outs = _draw_outputs(logits, stats=False)
        if logits.shape[0] > 0:
            p = _lib.SampleParams()
            _fill_rows(p, logits, outs, temperature, key)
            _lib.check(_lib.load().hyd_sample_tokens(C.byref(p), _stream()))
        return outs[0]
    if draw == sampling.FILTERED:
        tok, lp, _ = sample_tokens_filtered(logits, temperature, key, **cuts)
    elif logits.is_cuda and draw == sampling.CONSTRAINED:
        tok, lp, _ = sample_tokens_constrained(logits, temperature, key, constraint=constraint, penalties=pen, **cuts)
    elif logits.is_cuda:
        tok, lp, _ = sample_tokens_penalized(logits, temperature, key, penalties=pen, **cuts)
    else:
        dfa, state, advance = constraint if constraint is not None else (None, None, False)
        x = logits if pen is None else pen.apply(logits)
        tok, lp, drawn = sampling.reference_draw(x, temperature, dfa=dfa, state=state, seed=seed,
                                                 offset=0 if key is None else key[1], **cuts)
        if advance:
            state.copy_(sampling.advance_state(dfa, state, tok, drawn))
        if pen is not None and pen.append:
            pen.push(tok)
    return (tok, lp[:, None]) if return_logprobs else tok


def sample_tokens_filtered(logits: Tensor, temperature: float, key: Optional[tuple] = None, *, top_k: Optional[int] = None,
                           top_p: Optional[float] = None, min_p: Optional[float] = None):
    """hyd_sample_tokens_filtered: ([B, 1] int64 tokens, [B] fp32 log-probs, [B] int32 number of kept tokens)."""
    outs = _draw_outputs(logits, stats=True)
    if logits.shape[0] == 0:
        return outs
    check_filters(top_k, top_p, min_p)
    p = _lib.SampleFilterParams()
    _fill_rows(p, logits, outs, temperature, key, top_k, top_p, min_p)
    _lib.check(_lib.load().hyd_sample_tokens_filtered(C.byref(p), _stream()))
    return outs


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


def stop_update(tok: Tensor, t: int, spec: stopping.StopSpec, out: Tensor, length: Tensor, reason: Tensor, stop_index: Tensor,
                live: Tensor, start_pos: Tensor, shared_len: Optional[Tensor] = None, retire: bool = True,
                stop_tokens: Optional[Tensor] = None, max_len: Optional[Tensor] = None):
    """hyd_stop_update, one launch: judge the tokens `tok` [rows] (or [rows, 1]) int64 just drawn as step t of a generation whose
    state is (out int64 [rows, steps], length / reason / stop_index int32 [rows], live int32 [steps]; stopping.new_state), update
    that state in place and return (feed, next_pos) int64 [rows] for the next decode step; hydragen_amd/stopping.py states the
    rules.  start_pos int64 [rows]: the position step 0's token is fed at; shared_len int64 [rows] or None and retire: a finished
    row's position becomes shared_len - 1, which retires it from the unique K/V stream.  stop_tokens: spec.stop_table(device)[0]
    made once per generation (None: made here, one host-to-device copy).  max_len int32 [rows] on the device: a limit per row
    (hyd_stop_update_rows, reason 3; stopping.py rule (c')).  Nothing synchronises.  CPU tensors take
    stopping.stop_update_reference."""
    tok = tok.reshape(-1)
    rows = tok.shape[0]
    if tok.dtype != torch.int64 or out.ndim != 2 or out.shape[0] != rows or out.dtype != torch.int64 or out.stride(1) != 1:
        raise ValueError(f"tok must be int64 [rows] and out int64 [rows, steps] with a unit last stride, got {tuple(tok.shape)} {tok.dtype} "
                         f"and {tuple(out.shape)} {out.dtype}")
    steps = out.shape[1]
    for name, x, n in (("length", length, rows), ("reason", reason, rows), ("stop_index", stop_index, rows), ("live", live, steps)):
        if x.dtype != torch.int32 or x.shape != (n,) or not x.is_contiguous() or x.device != tok.device:
            raise ValueError(f"{name} must be a contiguous int32 [{n}] on {tok.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
    for name, x in (("start_pos", start_pos), ("shared_len", shared_len)):
        if x is not None and (x.dtype != torch.int64 or x.shape != (rows,) or not x.is_contiguous() or x.device != tok.device):
            raise ValueError(f"{name} must be a contiguous int64 [{rows}] on {tok.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
    if out.device != tok.device:
        raise ValueError(f"out is on {out.device}, tok on {tok.device}")
    if not 0 <= t < steps:
        raise ValueError(f"t {t} outside [0, {steps})")
    if max_len is not None and (max_len.dtype != torch.int32 or max_len.shape != (rows,) or not max_len.is_contiguous() or max_len.device != tok.device):
        raise ValueError(f"max_len must be a contiguous int32 [{rows}] on {tok.device}, got {tuple(max_len.shape)} {max_len.dtype} on {max_len.device}")
    if not tok.is_cuda:
        return stopping.stop_update_reference(tok, t, spec, out, length, reason, stop_index, live, start_pos, shared_len, retire, max_len)
    _require_gpu(tok)
    lib = _lib.load()
    tok = tok.contiguous()
    feed = torch.empty((rows,), dtype=torch.int64, device=tok.device)
    next_pos = torch.empty((rows,), dtype=torch.int64, device=tok.device)
    p = _lib.StopParams()
    if spec.stops:
        if stop_tokens is None:
            stop_tokens = spec.stop_table(tok.device)[0]
        if (stop_tokens.shape != (len(spec.stops), _lib.STOP_MAX_LEN) or stop_tokens.dtype != torch.int64 or not stop_tokens.is_contiguous()
                or stop_tokens.device != tok.device):
            raise ValueError(f"stop_tokens must be a contiguous int64 [{len(spec.stops)}, {_lib.STOP_MAX_LEN}] on {tok.device}")
        p.stop_tokens = stop_tokens.data_ptr()
    if len(spec.eos) > _lib.STOP_MAX_EOS or len(spec.stops) > _lib.STOP_MAX_SEQS:
        raise ValueError(f"{len(spec.eos)} EOS ids / {len(spec.stops)} stop sequences: at most {_lib.STOP_MAX_EOS} / {_lib.STOP_MAX_SEQS}")
    for i, e in enumerate(spec.eos):
        p.eos[i] = e
    for k, s_ in enumerate(spec.stops):
        p.stop_lens[k] = len(s_)
    p.tok, p.out, p.length, p.reason = tok.data_ptr(), out.data_ptr(), length.data_ptr(), reason.data_ptr()
    p.stop_index, p.live, p.start_pos = stop_index.data_ptr(), live.data_ptr(), start_pos.data_ptr()
    if shared_len is not None:
        p.shared_len = shared_len.data_ptr()
    p.feed, p.next_pos = feed.data_ptr(), next_pos.data_ptr()
    p.out_stride, p.pad = out.stride(0) if rows > 1 else steps, spec.pad
    p.rows, p.t, p.n_eos, p.n_stop = rows, t, len(spec.eos), len(spec.stops)
    p.include_stop, p.retire = int(spec.include_stop), int(bool(retire))
    if max_len is None:
        _lib.check(lib.hyd_stop_update(C.byref(p), _stream()))
    else:
        _lib.check(lib.hyd_stop_update_rows(C.byref(p), max_len.data_ptr(), _stream()))
    return feed, next_pos
