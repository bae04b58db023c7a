"""Sampling cuts in torch: the definition `hyd_sample_tokens_filtered` (csrc/sample_filter.hip) implements, evaluated in
float64.  It runs where sample_route (below) routes a stage to torch (the fan-out first token with num_samples > 1, CPU
tensors) and is the reference of the tests.

For one row of logits l with m = max(l) and p = softmax(l):
  * the cuts act on the UNSCALED softmax(l), not on softmax(l / T) (the reference's `apply_top_p`; HF applies the
    temperature first, so results differ from HF when T != 1);
  * top_k keeps l >= the k-th largest logit (ties kept, HF's TopKLogitsWarper rule); k >= n: no cut;
  * top_p then keeps, among the top-k survivors renormalised, l >= t*, where t* is the largest logit value whose top set
    {l >= t*} holds >= top_p of their mass: the crossing token and every token tied with it are kept (without ties this is
    the reference's "remove where the ascending cumsum <= 1 - top_p, keep >= 1 token");
  * min_p keeps p_i >= min_p * p_max, i.e. l_i - m >= ln(min_p);
  * -inf and NaN logits are never kept.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
from torch import Tensor


# ---- per-row values ---------------------------------------------------------------------------------------------------------
# Every sampling parameter below -- temperature, top_k, top_p, min_p and the three penalties -- is a scalar (or None = off) for
# all rows, or PER ROW: a list / tuple (None inside = off for that row) or a 1-d tensor with one entry per row; one entry
# alone is broadcast.  Row r of a per-row call is, by definition, row r of the scalar call with row r's values: the functions
# group the rows by their values and run the scalar definition on each group (every step of it acts on rows independently).
def is_per_row(v) -> bool:
    return isinstance(v, (list, tuple, Tensor))


def row_values(v, rows: Optional[int] = None, what: str = "value") -> list:
    """A per-row argument as a list of `rows` Python scalars (None kept); a scalar is repeated."""
    if not is_per_row(v):
        return [v] * (1 if rows is None else rows)
    if isinstance(v, Tensor):
        if v.ndim > 1:
            raise ValueError(f"{what}: per-row values are 1-d, got {tuple(v.shape)}")
        v = v.reshape(-1).tolist()
    v = list(v)
    if rows is not None and len(v) == 1:
        v = v * rows
    if rows is not None and len(v) != rows:
        raise ValueError(f"{what}: {len(v)} per-row values for {rows} rows")
    return v


def row_groups(rows: int, **params) -> Optional[list]:
    """None if every parameter is a scalar; else [(row indices int64 [k], {name: that group's scalar})], the rows with equal
    values together, in order of first appearance (one group if every row is equal)."""
    if not any(is_per_row(v) for v in params.values()):
        return None
    cols = {k: row_values(v, rows, k) for k, v in params.items()}
    groups: dict = {}
    for r in range(rows):
        groups.setdefault(tuple(cols[k][r] for k in params), []).append(r)
    return [(torch.tensor(idx, dtype=torch.int64), dict(zip(params, key))) for key, idx in groups.items()]


def _each(v):
    """The host values of an argument: a scalar, the entries of a list, and nothing of a tensor (tensors may live on a device and
    are not read back: the kernel sanitises what it reads, the torch definition checks each group's scalars)."""
    return () if isinstance(v, Tensor) else row_values(v) if is_per_row(v) else (v,)


def filters_active(top_k, top_p, min_p) -> bool:
    if any(isinstance(v, Tensor) for v in (top_k, top_p, min_p)):
        return True
    return any(bool(k) for k in _each(top_k)) or any(p is not None and p < 1.0 for p in _each(top_p)) or any(bool(m) for m in _each(min_p))


def check_filters(top_k, top_p, min_p) -> None:
    if is_per_row(top_k) or is_per_row(top_p) or is_per_row(min_p):  # element by element, the same messages
        for k in _each(top_k):
            check_filters(k, None, None)
        for p_ in _each(top_p):
            check_filters(None, p_, None)
        for m in _each(min_p):
            check_filters(None, None, m)
        return
    if top_k is not None and top_k < 0:
        raise ValueError(f"top_k {top_k} must be >= 0 (0 or None = off)")
    if top_p is not None and not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p {top_p} must be in (0, 1] (1 or None = off)")
    if min_p is not None and not (0.0 <= min_p <= 1.0):
        raise ValueError(f"min_p {min_p} must be in [0, 1] (0 or None = off)")


@torch.no_grad()
def kept_mask(logits: Tensor, top_k=None, top_p=None, min_p=None) -> Tensor:
    """[..., n] bool: the tokens the cuts keep (module docstring), computed in float64.  Per-row values: logits [B, n]."""
    check_filters(top_k, top_p, min_p)
    groups = row_groups(logits.shape[0], top_k=top_k, top_p=top_p, min_p=min_p) if logits.ndim == 2 else None
    if groups is not None:
        keep = torch.empty(logits.shape, dtype=torch.bool, device=logits.device)
        for idx, vals in groups:
            idx = idx.to(logits.device)
            keep[idx] = kept_mask(logits[idx], **vals)
        return keep
    x = logits.double()
    valid = ~(torch.isnan(x) | (x == -math.inf))
    xm = torch.where(valid, x, torch.full_like(x, -math.inf))
    m = xm.amax(dim=-1, keepdim=True)
    keep = valid
    n = x.shape[-1]
    if top_k:
        kth = torch.topk(xm, min(int(top_k), n), dim=-1).values[..., -1:]
        keep = keep & (xm >= kth)
    if top_p is not None and top_p < 1.0:
        w = torch.where(keep, torch.where(xm == m, torch.ones_like(x), torch.exp(xm - m)), torch.zeros_like(x))
        v = torch.where(keep, xm, torch.full_like(x, -math.inf))
        vs, order = torch.sort(v, dim=-1, descending=True)
        cs = torch.cumsum(torch.gather(w, -1, order), dim=-1)
        # mass of {l >= vs_i}: the cumsum at the last position of vs_i's tie group
        last = n - torch.searchsorted(vs.flip(-1).contiguous(), vs.contiguous(), right=False) - 1
        above = torch.gather(cs, -1, last)
        cross = above >= top_p * cs[..., -1:]
        first = torch.argmax(cross.to(torch.int8), dim=-1, keepdim=True)  # first position that reaches top_p
        keep = keep & (xm >= torch.gather(vs, -1, first))
    if min_p:
        keep = keep & ((xm == m) | (xm - m >= math.log(min_p)))
    return keep


@torch.no_grad()
def filter_logits(logits: Tensor, top_k=None, top_p=None, min_p=None) -> Tensor:
    """`logits` with every token the cuts remove (and every NaN) set to -inf, in the input dtype."""
    return logits.masked_fill(~kept_mask(logits, top_k, top_p, min_p), -math.inf)


# ---- penalties ------------------------------------------------------------------------------------------------------------
# Repetition / presence / frequency penalties and a sparse logit bias: the definition `hyd_sample_tokens_penalized`
# (csrc/sample_penalty.hip) implements, evaluated in float64.  For one row of logits l (length n), with
#   ctx  = the token ids of the row's CONTEXT: every shared level on the row's path and the row's own prompt, given as
#          presence bitmaps `(bits int32 [groups, ceil(n / 32)], rows_per_group)`; row b reads bitmap row b // rows_per_group,
#          token v is bit v % 32 of word v // 32;
#   c[v] = how often v occurs among the row's GENERATED tokens gen[b, :gen_len[b]] (entries outside [0, n) are ignored),
# the penalised logits x are, in this order:
#   1. repetition_penalty r > 0 (1 or None = off; the HF / vLLM rule, over prompt and output): for v in ctx or c[v] > 0,
#      x = l / r if l > 0 else l * r; else x = l;
#   2. frequency_penalty f, presence_penalty a (0 or None = off; any finite value; the OpenAI / vLLM rule, output only):
#      x -= f * c[v] + a * (c[v] > 0);
#   3. logit_bias (ids int64 [K], values fp32 [K]), ids distinct in [0, n), K <= BIAS_MAX, one list for all rows:
#      x[ids] += values; -inf bans a token (the cuts' rule "-inf and NaN are never kept" then applies).
# The cuts, the draw and the log-prob then act on x instead of l.
BIAS_MAX = 1024  # HYD_SAMPLE_BIAS_MAX
GEN_MAX = 2048   # HYD_SAMPLE_GEN_MAX: generated tokens per row the kernel counts
MAX_CONTEXT = 9  # HYD_SAMPLE_MAX_CONTEXT


def normalize_logit_bias(logit_bias, device=None):
    """dict[int, float] or (ids, values) -> (ids int64 [K], values fp32 [K]) tensors, or None for an empty / absent bias."""
    if logit_bias is None:
        return None
    if isinstance(logit_bias, dict):
        ids = torch.tensor([int(k) for k in logit_bias.keys()], dtype=torch.int64)
        values = torch.tensor([float(v) for v in logit_bias.values()], dtype=torch.float32)
    else:
        ids, values = logit_bias
        ids = torch.as_tensor(ids).to(torch.int64).reshape(-1)
        values = torch.as_tensor(values).to(torch.float32).reshape(-1)
    if ids.numel() == 0 and values.numel() == 0:
        return None
    if device is not None:
        ids, values = ids.to(device), values.to(device)
    return ids.contiguous(), values.contiguous()


def penalties_active(repetition_penalty=None, presence_penalty=None, frequency_penalty=None, logit_bias=None) -> bool:
    if isinstance(logit_bias, dict):
        has_bias = len(logit_bias) > 0
    else:
        has_bias = logit_bias is not None and len(logit_bias[0]) > 0
    if any(isinstance(v, Tensor) for v in (repetition_penalty, presence_penalty, frequency_penalty)):
        return True  # (per-row values on a device are not read back to find out)
    return (any(r is not None and r != 1.0 for r in _each(repetition_penalty)) or any(bool(v) for v in _each(presence_penalty))
            or any(bool(v) for v in _each(frequency_penalty)) or has_bias)


def check_penalties(repetition_penalty=None, presence_penalty=None, frequency_penalty=None, logit_bias=None,
                    n: Optional[int] = None) -> None:
    """Host validation (reads the bias list: call it before the decode loop, not inside).  n: the vocabulary size, if known.
    Per-row lists are checked element by element, with the same messages."""
    for r in _each(repetition_penalty):
        if r is not None and not (r > 0 and math.isfinite(r)):
            raise ValueError(f"repetition_penalty {r} must be a finite number > 0 (1 or None = off)")
    for name, vs in (("presence_penalty", presence_penalty), ("frequency_penalty", frequency_penalty)):
        for v in _each(vs):
            if v is not None and not math.isfinite(v):
                raise ValueError(f"{name} {v} must be finite (0 or None = off)")
    if logit_bias is None:
        return
    if not isinstance(logit_bias, dict) and not (isinstance(logit_bias, (tuple, list)) and len(logit_bias) == 2):
        raise ValueError("logit_bias must be a dict {token id: bias} or an (ids, values) pair")
    if not isinstance(logit_bias, dict) and len(logit_bias[0]) != len(logit_bias[1]):
        raise ValueError(f"logit_bias has {len(logit_bias[0])} ids and {len(logit_bias[1])} values")
    bias = normalize_logit_bias(logit_bias)
    if bias is None:
        return
    ids, values = (t.cpu() for t in bias)
    if ids.numel() > BIAS_MAX:
        raise ValueError(f"logit_bias has {ids.numel()} entries: at most {BIAS_MAX}")
    if ids.unique().numel() != ids.numel():
        raise ValueError("logit_bias ids must be distinct")
    if int(ids.min()) < 0 or (n is not None and int(ids.max()) >= n):
        raise ValueError(f"logit_bias ids must be in [0, {n if n is not None else 'vocabulary size'})")
    if bool((torch.isnan(values) | (values == math.inf)).any()):
        raise ValueError("logit_bias values must be finite or -inf (-inf bans a token); +inf and NaN are refused")


@torch.no_grad()
def token_bitmap_reference(ids: Tensor, lens: Optional[Tensor], n: int) -> Tensor:
    """[groups, L] token ids (+ [groups] lengths, None = all L) -> presence bitmap int32 [groups, ceil(n / 32)], in torch on any
    device (the definition of hyd_token_bitmap_build; it goes through a [groups, n] table, which the kernel does not)."""
    groups, L = ids.shape
    words = (n + 31) // 32
    ids = ids.long()
    live = (ids >= 0) & (ids < n)
    if lens is not None:
        live &= torch.arange(L, device=ids.device)[None, :] < lens.to(ids.device).long().reshape(-1, 1)
    present = torch.zeros((groups, words * 32 + 1), dtype=torch.int64, device=ids.device)
    present.scatter_(1, torch.where(live, ids, torch.full_like(ids, words * 32)), 1)
    weights = torch.ones(32, dtype=torch.int64, device=ids.device) << torch.arange(32, device=ids.device)
    packed = (present[:, : words * 32].reshape(groups, words, 32) * weights).sum(-1)
    return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)


@torch.no_grad()
def context_mask(context, rows: int, n: int) -> Tensor:
    """[rows, n] bool: the tokens of every row's context, from `context` = [(bits [groups, ceil(n / 32)], rows_per_group)]."""
    mask = None
    for bits, rpg in context:
        shifts = torch.arange(32, device=bits.device, dtype=torch.int64)
        unpacked = ((bits.long()[:, :, None] >> shifts) & 1).bool().reshape(bits.shape[0], -1)[:, :n]
        m = unpacked.repeat_interleave(int(rpg), dim=0)[:rows]
        if m.shape[0] != rows:
            raise ValueError(f"a context bitmap of {bits.shape[0]} groups x {rpg} rows does not cover {rows} rows")
        mask = m if mask is None else (mask | m)
    return mask


@torch.no_grad()
def penalize_logits(logits: Tensor, repetition_penalty=None, presence_penalty=None, frequency_penalty=None, logit_bias=None,
                    context=(), gen: Optional[Tensor] = None, gen_len: Optional[Tensor] = None) -> Tensor:
    """[rows, n] logits -> the penalised logits x in float64 (the comment block above), on the logits' device.  context:
    [(bits, rows_per_group)]; gen [rows, stride] integer tokens with gen_len [rows] (None: no generated tokens).  The three
    penalties may be per row (evaluated in float64 as given; the kernel takes per-row values as fp32, layer_ops.sample_tokens)."""
    check_penalties(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, logits.shape[-1])
    rows, n = logits.shape
    groups = row_groups(rows, repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty)
    if groups is not None:
        ctx = context_mask([(b.to(logits.device), k) for b, k in context], rows, n) if len(context) else None
        out = torch.empty(logits.shape, dtype=torch.float64, device=logits.device)
        for idx, vals in groups:
            idx = idx.to(logits.device)
            check_penalties(**vals)
            out[idx] = _penalize(logits[idx], vals["repetition_penalty"], vals["presence_penalty"], vals["frequency_penalty"],
                                 logit_bias, None if ctx is None else ctx[idx], None if gen is None else gen.to(logits.device)[idx],
                                 None if gen is None else gen_len.to(logits.device)[idx])
        return out
    ctx = context_mask([(b.to(logits.device), k) for b, k in context], rows, n) if len(context) and (repetition_penalty or 1.0) != 1.0 else None
    return _penalize(logits, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, ctx, gen, gen_len)


@torch.no_grad()
def draft_row_lists_reference(gen: Optional[Tensor], gen_len: Optional[Tensor], fed: Tensor):
    """The token lists behind the B * T logits rows of a speculative step (the definition hyd_sample_tokens_penalized_drafts
    implements without building them): gen integer [B, stride] with gen_len [B] (None: empty lists), fed integer [B, T] ->
    (lists int64 [B * T, stride + T - 1], lens int32 [B * T]), usable as penalize_logits' gen / gen_len.  Row r = b * T + i holds
    gen[b, 0 .. min(gen_len[b], stride)) followed by fed[b, 1 .. i] -- the drafts fed in front of the position the row draws;
    fed[b, 0] is the last emitted token and is already in gen.  Ids are copied as they are (the penalties ignore those outside
    [0, n)); slots past a row's length hold -1."""
    B, T = fed.shape
    stride = 0 if gen is None else gen.shape[1]
    lists = torch.full((B * T, stride + T - 1), -1, dtype=torch.int64, device=fed.device)
    lens = torch.zeros((B * T,), dtype=torch.int32, device=fed.device)
    for b in range(B):
        n = 0 if gen is None else max(0, min(int(gen_len[b]), stride))
        for i in range(T):
            r = b * T + i
            if n:
                lists[r, :n] = gen[b, :n].long()
            lists[r, n: n + i] = fed[b, 1: 1 + i].long()
            lens[r] = n + i
    return lists, lens


def _penalize(logits, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, ctx, gen, gen_len) -> Tensor:
    """penalize_logits with scalar penalties and the context as a [rows, n] bool mask (or None)."""
    rows, n = logits.shape
    x = logits.double()
    dev = x.device
    counts = torch.zeros((rows, n + 1), dtype=torch.float64, device=dev)
    if gen is not None and gen.shape[1] > 0:
        g = gen.to(dev).long()
        live = (g >= 0) & (g < n) & (torch.arange(g.shape[1], device=dev)[None, :] < gen_len.to(dev).long().reshape(-1, 1))
        counts.scatter_add_(1, torch.where(live, g, torch.full_like(g, n)), torch.ones(g.shape, dtype=torch.float64, device=dev))
    counts = counts[:, :n]
    seen = counts > 0
    r = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if r != 1.0:
        hit = seen if ctx is None else (seen | ctx)
        x = torch.where(hit, torch.where(x > 0, x / r, x * r), x)
    f, a = float(frequency_penalty or 0.0), float(presence_penalty or 0.0)
    if f or a:
        x = torch.where(seen, x - (f * counts + a * seen.double()), x)
    bias = normalize_logit_bias(logit_bias, dev)
    if bias is not None:
        x[:, bias[0]] += bias[1].double()
    return x


# ---- token automata ---------------------------------------------------------------------------------------------------------
# Constrained decoding: the definition `hyd_sample_tokens_constrained` (csrc/sample_constrain.hip) implements.  A token
# automaton over n tokens with S states is one table next int32 [S, n] (hydragen_amd/constraint.py builds them):
#   next[s, v] >= 0           token v is allowed in state s and leads to that state (< S);
#   next[s, v] == DFA_REJECT  v is not allowed in s;
#   next[s, v] == DFA_FREE    v is allowed, and the row is unconstrained from then on;
# and the bitmap allowed int32 [S, ceil(n / 32)] derived from it: bit v % 32 of word v // 32 is set iff next[s, v] != DFA_REJECT
# (the bit layout of token_bitmap_reference).  A row whose state lies outside [0, S) is unconstrained: its logits are taken as
# they are and its state does not change.  For a constrained row every sampling rule above (penalties, bias, cuts, draw,
# log-prob, kept) acts on the row with the logits of the tokens that are not allowed replaced by -inf; bits at positions >= n
# are ignored.  After the draw state[row] = next[state[row], token]; a row without any valid logit (token 0, kept 0, NaN
# log-prob) keeps its state.  A `dfa` below is anything with .next, .allowed, .num_states and .vocab_size (constraint.TokenDFA).
DFA_REJECT = -1  # HYD_DFA_REJECT
DFA_FREE = -2    # HYD_DFA_FREE


def check_constraint(dfa, vocab_size: int, batch: Optional[int] = None, state: Optional[Tensor] = None) -> None:
    """Host validation of an automaton against the logits' width (shapes and dtypes only: nothing is read from the device)."""
    nxt, allowed = dfa.next, dfa.allowed
    if nxt.ndim != 2 or nxt.dtype != torch.int32 or nxt.shape[0] <= 0 or not nxt.is_contiguous():
        raise ValueError(f"constraint: next must be a contiguous int32 [S, n] with S > 0, got {tuple(nxt.shape)} {nxt.dtype}")
    if nxt.shape[1] != vocab_size:
        raise ValueError(f"constraint: the automaton is over {nxt.shape[1]} tokens, the logits over {vocab_size}")
    words = (vocab_size + 31) // 32
    if allowed.shape != (nxt.shape[0], words) or allowed.dtype != torch.int32 or not allowed.is_contiguous() or allowed.device != nxt.device:
        raise ValueError(f"constraint: allowed must be a contiguous int32 [{nxt.shape[0]}, {words}] on {nxt.device}, got "
                         f"{tuple(allowed.shape)} {allowed.dtype} on {allowed.device}")
    if state is not None:
        if state.dtype != torch.int32 or state.ndim != 1 or not state.is_contiguous() or (batch is not None and state.shape[0] != batch):
            raise ValueError(f"constraint: state must be a contiguous int32 [{'B' if batch is None else batch}], got "
                             f"{tuple(state.shape)} {state.dtype}")


@torch.no_grad()
def allowed_mask(dfa, state: Tensor) -> Tensor:
    """[B, n] bool: what each row may emit, read from the BITMAP (what the kernel reads); unconstrained rows: all True."""
    S, n = dfa.next.shape
    st = state.long().to(dfa.allowed.device)
    on = (st >= 0) & (st < S)
    words = dfa.allowed[torch.where(on, st, torch.zeros_like(st))].long()  # [B, words]
    shifts = torch.arange(32, device=words.device, dtype=torch.int64)
    bits = ((words[:, :, None] >> shifts) & 1).bool().reshape(words.shape[0], -1)[:, :n]
    return bits | ~on[:, None]


@torch.no_grad()
def constrain_logits(logits: Tensor, dfa, state: Tensor) -> Tensor:
    """`logits` [B, n] with the tokens a row's state does not allow set to -inf, in the input dtype, on the logits' device."""
    check_constraint(dfa, logits.shape[-1], logits.shape[0])
    return logits.masked_fill(~allowed_mask(dfa, state).to(logits.device), -math.inf)


@torch.no_grad()
def advance_state(dfa, state: Tensor, tokens: Tensor, drawn: Optional[Tensor] = None) -> Tensor:
    """The states after `tokens` ([B] or [B, 1]): next[state, token] for constrained rows, the state itself for unconstrained
    ones and for rows where nothing was drawn (drawn [B] bool, None = every row drew: a row without a valid logit reports
    token 0 and keeps its state).  A REJECT or FREE entry leaves the row unconstrained.  Returns int32 [B] on the state's device."""
    S = dfa.next.shape[0]
    st = state.long()
    tok = tokens.reshape(-1).long().to(st.device)
    on = (st >= 0) & (st < S)
    if drawn is not None:
        on = on & drawn.reshape(-1).bool().to(st.device)
    nxt = dfa.next.to(st.device)[torch.where(on, st, torch.zeros_like(st)), tok].long()
    return torch.where(on, nxt, st).to(torch.int32)


# ---- one draw, as a route ------------------------------------------------------------------------------------------------------
# The draws: four entry points by their C names (CONSTRAINED and PENALIZED on CPU rows: their float64 definition,
# reference_draw; the others take GPU rows only) and TORCH: argmax at temperature 0, else softmax + multinomial.
CONSTRAINED, PENALIZED, FILTERED, PLAIN, TORCH = ("hyd_sample_tokens_constrained", "hyd_sample_tokens_penalized",
                                                  "hyd_sample_tokens_filtered", "hyd_sample_tokens", "torch")


class SampleRoute(NamedTuple):
    draw: str                      # the entry point that draws (one key of the device's generator per call), or TORCH
    torch_penalties: bool = False  # before the draw: Penalties.apply(rows, num_samples).float(); after it: Penalties.push
    torch_mask: bool = False       # before the draw: repeat per sample + constrain_logits; after it: advance_state
    torch_cuts: bool = False       # before the draw: filter_logits (top_p alone: the reference's apply_top_p)


def sample_route(cuda: bool, eligible: bool, rewritten: bool, num_samples: int, constraint: bool, penalties: bool, filters: bool,
                 logprobs: bool, fused_filters: bool = True, fused_penalties: bool = True, per_row: bool = False) -> SampleRoute:
    """THE table of the sampling routes: generation.draw_tokens runs a route, layer_ops.sample_tokens picks its entry point from one.
    cuda: the rows are on the GPU; rewritten: and 2-D with temperature >= 0, what a kernel needs of rows a torch stage has
    rewritten (contiguous); eligible: and of unit last stride as they are (a kernel takes them when num_samples == 1);
    constraint / penalties / filters: given / active; logprobs: wanted; fused_*: the model's two switches.  The penalties in
    torch hand on fp32 rows; mask and cuts keep the dtype: other rows reach the kernels in their own.  Penalties.push happens
    only for one sample per row and a Penalties that appends.
    per_row: a sampling value is given per row, or the rows have seeds of their own.  GPU rows: always a kernel route (FILTERED,
    PENALIZED or CONSTRAINED by what is given; no torch stage), drawn through hyd_sample_tokens_rows -- the caller makes rows a
    kernel cannot take as they are contiguous and, for num_samples > 1, repeats them per sample first, as the masked route does.
    CPU rows: the same three names, which on CPU rows mean the torch definition (reference_draw)."""
    if per_row:
        return SampleRoute(CONSTRAINED if constraint else PENALIZED if penalties else FILTERED)
    kernel = eligible and num_samples == 1
    if constraint and num_samples == 1 and (not cuda or (kernel and (not penalties or fused_penalties))):
        return SampleRoute(CONSTRAINED)  # one launch with everything in it
    if penalties and not constraint and kernel and fused_penalties:
        return SampleRoute(PENALIZED)
    # otherwise penalties and mask run in torch, and what is left is a draw with neither, on the rows they have rewritten
    if penalties:
        kernel = rewritten and num_samples == 1
    if constraint:
        kernel, logprobs = rewritten, True  # one sample per masked row; whether a row drew a token is read off its log-prob
    if kernel and (logprobs or (filters and fused_filters)):
        return SampleRoute(FILTERED, penalties, constraint)
    # cuts in torch; log-probs, if wanted (or forced on by the mask), are log softmax of the rows before the cuts
    return SampleRoute(PLAIN if kernel else TORCH, penalties, constraint, filters)


def apply_top_p(logits: Tensor, top_p: float, min_tokens_to_keep: int = 1, filter_value: float = -math.inf) -> Tensor:
    """The reference's top-p cut (its llama.py, modified from HF's TopPLogitsWarper): what a top_p alone runs in torch."""
    sorted_logits, sorted_indices = torch.sort(logits, descending=False)
    cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    remove = cumulative_probs <= (1 - top_p)
    remove[..., -min_tokens_to_keep:] = 0
    return logits.masked_fill(remove.scatter(1, sorted_indices, remove), filter_value)


@torch.no_grad()
def reference_draw(x: Tensor, temperature, top_k=None, top_p=None, min_p=None, dfa=None, state: Optional[Tensor] = None,
                   seed=None, offset: int = 0):
    """PENALIZED / CONSTRAINED in torch, for CPU rows: x [B, n] the (penalised: float64) logits, masked here if an automaton is
    given -> (tokens int64 [B, 1], fp32 log-probs [B], drawn bool [B]); a row without a valid logit: token 0, NaN, not drawn.
    temperature and the cuts may be per row: the rows that share a temperature are drawn by one torch.multinomial call, groups in
    order of first appearance (every row equal: the scalar call's single draw).  seed (one int per row) with offset: each row
    draws from a torch.Generator of its own, seeded from (seed[row], offset) alone -- the global generator is not advanced and
    the draw does not depend on the row's place in the batch.  (The kernels' Philox noise is another stream: seeded CPU and GPU
    draws agree in distribution, not in tokens.)"""
    xc = x if dfa is None else constrain_logits(x, dfa, state)
    keep = kept_mask(xc, top_k, top_p, min_p)
    drawn = keep.any(-1, keepdim=True)
    xf = xc.masked_fill(~keep, -math.inf)
    seeds = None if seed is None else [int(v) for v in row_values(seed, x.shape[0], "seed")]
    groups = row_groups(x.shape[0], temperature=temperature)
    if seeds is not None:  # one draw per row, from the row's own generator
        temps = row_values(temperature, x.shape[0], "temperature")
        groups = [(torch.tensor([r], dtype=torch.int64), dict(temperature=temps[r])) for r in range(x.shape[0])]
    if groups is not None:
        tok = torch.zeros((x.shape[0], 1), dtype=torch.int64, device=x.device)
        for idx, vals in groups:
            t = vals["temperature"] or 0.0
            idx = idx.to(x.device)
            if t == 0:
                tok[idx] = xf[idx].argmax(-1, keepdim=True)
                continue
            pr = torch.softmax(xf[idx].double() / t, -1)
            gen = None
            if seeds is not None:
                gen = torch.Generator(device=x.device)
                gen.manual_seed((seeds[int(idx[0])] * 0x9E3779B97F4A7C15 + int(offset)) % (1 << 63))
            tok[idx] = torch.multinomial(torch.where(drawn[idx], pr, torch.ones_like(pr)), 1, generator=gen)
    elif temperature == 0:
        tok = xf.argmax(-1, keepdim=True)
    else:
        pr = torch.softmax(xf.double() / temperature, -1)
        tok = torch.multinomial(torch.where(drawn, pr, torch.ones_like(pr)), 1)
    tok = torch.where(drawn, tok, torch.zeros_like(tok))
    lp = torch.log_softmax(xc.double(), -1).gather(1, tok).float()
    return tok, torch.where(drawn, lp, torch.full_like(lp, math.nan))[:, 0], drawn[:, 0]
