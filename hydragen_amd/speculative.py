"""Speculative decoding: several tokens per forward pass, verified in ONE multi-token decode step.

Each step feeds every row T = K + 1 tokens -- its last emitted token and K drafts -- and one forward pass over [B, T] gives T rows of
logits per row.  The sampler draws one token t_i from each of them with the call's temperature and cuts, and the row keeps
t_0 .. t_n, n = the number of leading drafts with draft_{i+1} == t_i.

Why this is lossless, for greedy AND sampled decoding: the logits behind fed token i are the model's distribution of the next token
given the context and fed tokens 0 .. i.  t_0 is therefore always a draw from the target distribution -- it is what a one-token step
would have drawn.  t_1 is a draw from the target distribution GIVEN that the token after the context is draft_1; it is kept only when
t_0 == draft_1, i.e. when the token actually emitted in front of it is the one it was conditioned on -- and so on down the row.
Every emitted token is thus a draw from the target distribution given a correct prefix; a draw behind a wrong draft was conditioned
on a token that was never emitted and is thrown away, which costs nothing but its slot.  No acceptance probability, no
resampling: the drafts are not sampled from a proposal distribution whose mass would have to be corrected for, they are only
compared with what the target drew.  (With temperature 0 the tokens are exactly those of one-token decoding up to the numerics
of the T-token kernels.)

The drafts come from the prompt (`draft="prompt_lookup"`): the completions of long-document QA, few-shot prompts and many samples of
one prompt copy from their shared prompt, so the tokens that followed the latest earlier occurrence of the row's last n-gram are
proposed -- no draft model.  Levels kept from EARLIER generate() calls (shared_cache_op="extend") are not searched: their token
ids are not given to the call that decodes.

Under a token automaton (generate(constraint=)) the drafts are first walked through it: a state that allows exactly one token forces
that token as the draft -- accepted with probability 1, the masked sampler can draw nothing else -- and `draft="constraint"` proposes
nothing but those (`constrain_drafts`, the states in `draft_accept`).

Stop sequences and the penalties' token lists ride on the accept (`draft_accept(stop=, gen=, gen_len=)`, hyd_draft_accept_stop): a
step emits several tokens per row, a stop sequence may complete at any of them, and only the accept knows which draws became output.
The draw behind the i-th fed token counts the drafts fed in front of it as generated (sampling.draft_row_lists_reference,
hyd_sample_tokens_penalized_drafts): it is conditioned on them, and a draw that ignored them would not be from the target distribution.

This module holds the definitions in torch (`prompt_lookup_reference`, `accept_reference`, `accept_stop_reference`,
`constrain_drafts_reference`, `accept_states_reference`, `assembled_causal_tail_attention`) and the Python faces of the kernels (`draft_lookup`, `draft_accept`,
`constrain_drafts`; the multi-token RoPE + append is fused_decode.rope_append_multi, the causal-tail attention
flash.flash_attention_seqlen / attention.hydragen_attention with causal_tail=True)."""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from .sampling import DFA_FREE, DFA_REJECT

MAX_DRAFTS = 7  # K: T = K + 1 <= 8 tokens per row and step
MAX_SEGMENTS = _lib.DRAFT_MAX_SEGMENTS  # of a lookup's table: the levels given to the call, the rows' prompts, the generated tokens


class _DraftStats(NamedTuple):
    steps: int
    proposed: Tensor
    accepted: Tensor


class DraftStats(_DraftStats):
    """Statistics of a speculative generation: decode steps run, and per row (int64 [B]) the drafts proposed to running rows and
    the drafts that became output -- a tuple of these three.  `forced` (an attribute, not a field: code that unpacks the three
    keeps working): per row the proposed drafts a forced automaton state wrote, None without constraint=."""

    def __new__(cls, steps, proposed, accepted, forced: Optional[Tensor] = None):
        self = super().__new__(cls, steps, proposed, accepted)
        self.forced = forced
        return self


class Segment(NamedTuple):
    """One piece of the rows' logical token sequences: ids int64 [rows, width]; lens int [rows] or None (= width); row b of a batch
    of B reads row b // (B // rows)."""
    ids: Tensor
    lens: Optional[Tensor] = None


def check_ngram(ngram) -> tuple:
    lo, hi = (int(x) for x in ngram)
    if not 1 <= lo <= hi <= _lib.DRAFT_MAX_NGRAM:
        raise ValueError(f"ngram = ({lo}, {hi}): 1 <= min <= max <= {_lib.DRAFT_MAX_NGRAM}")
    return lo, hi


def check_draft_tokens(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_DRAFTS:
        raise ValueError(f"draft_tokens = {k!r}: an int from 1 to {MAX_DRAFTS} (None or 0 switches speculative decoding off)")
    return k


def _check_segments(segments: Sequence[Segment], batch: int):
    if not 1 <= len(segments) <= _lib.DRAFT_MAX_SEGMENTS:
        raise ValueError(f"{len(segments)} segments: 1 to {_lib.DRAFT_MAX_SEGMENTS}")
    for i, (ids, lens) in enumerate(segments):
        if ids.ndim != 2 or ids.dtype != torch.int64 or ids.shape[0] < 1 or batch % ids.shape[0]:
            raise ValueError(f"segment {i}: ids must be int64 [rows, width] with rows dividing the batch {batch}, got {tuple(ids.shape)} {ids.dtype}")
        if lens is not None and (lens.shape != (ids.shape[0],) or lens.dtype not in (torch.int32, torch.int64)):
            raise ValueError(f"segment {i}: lens must be int32 / int64 [{ids.shape[0]}], got {tuple(lens.shape)} {lens.dtype}")


def logical_sequences(segments: Sequence[Segment], batch: int) -> list:
    """The rows' logical sequences as Python lists (the definition's view; the kernel never builds them)."""
    _check_segments(segments, batch)
    rows = []
    for b in range(batch):
        seq = []
        for ids, lens in segments:
            r = b // (batch // ids.shape[0])
            n = ids.shape[1] if lens is None else max(0, min(int(lens[r]), ids.shape[1]))
            seq += ids[r, :n].tolist()
        rows.append(seq)
    return rows


def prompt_lookup_reference(segments: Sequence[Segment], batch: int, k: int, ngram=(1, 3)):
    """The rule hyd_draft_lookup implements -> (drafts int64 [batch, k], n_proposed int32 [batch]).  For n = ngram max down to min:
    the last n tokens of the row's logical sequence (skipped when the sequence is shorter) are looked for among the earlier
    positions; an occurrence must end strictly before the last position; the latest one wins and the up-to-k tokens behind it
    are proposed, clipped at the sequence's end; the first n with an occurrence wins.  Slots without a proposal hold 0."""
    k = check_draft_tokens(k)
    lo, hi = check_ngram(ngram)
    drafts = torch.zeros((batch, k), dtype=torch.int64)
    n_prop = torch.zeros((batch,), dtype=torch.int32)
    for b, seq in enumerate(logical_sequences(segments, batch)):
        L = len(seq)
        for n in range(hi, lo - 1, -1):
            if L < n:
                continue
            tail = seq[L - n:]
            ends = [e for e in range(n - 1, L - 1) if seq[e - n + 1: e + 1] == tail]  # e <= L - 2: the trivial match is excluded
            if ends:
                follow = seq[ends[-1] + 1: ends[-1] + 1 + k]
                drafts[b, : len(follow)] = torch.tensor(follow, dtype=torch.int64)
                n_prop[b] = len(follow)
                break
    return drafts, n_prop


def draft_lookup(segments: Sequence[Segment], batch: int, k: int, ngram=(1, 3), out: Optional[Tensor] = None):
    """hyd_draft_lookup, one launch, no host synchronisation -> (drafts int64 [batch, k], n_proposed int32 [batch]); CPU tensors
    take prompt_lookup_reference.  out: an int64 [batch, >= k] tensor whose first k columns receive the drafts (a view of the
    next step's input, columns 1 ..)."""
    k = check_draft_tokens(k)
    lo, hi = check_ngram(ngram)
    _check_segments(segments, batch)
    dev = segments[0].ids.device
    if dev.type != "cuda":
        d, n = prompt_lookup_reference(segments, batch, k, (lo, hi))
        if out is not None:
            out[:, :k] = d
            d = out[:, :k]
        return d, n
    p = _lib.DraftLookupParams()
    keep = []
    for i, (ids, lens) in enumerate(segments):
        if ids.device != dev or (lens is not None and lens.device != dev):
            raise ValueError(f"segment {i} is not on {dev}")
        if ids.stride(1) != 1:
            ids = ids.contiguous()
        s = p.segments[i]
        s.ids, s.row_stride, s.len, s.div = (ids.data_ptr() if ids.numel() else None), ids.stride(0), ids.shape[1], batch // ids.shape[0]
        if lens is not None:
            lens = lens.contiguous()
            if lens.dtype == torch.int64:
                s.lens_i64 = lens.data_ptr()
            else:
                s.lens_i32 = lens.data_ptr()
        if not ids.numel():
            s.len, s.lens_i64, s.lens_i32 = 0, None, None
        keep += [ids, lens]
    if out is None:
        out = torch.empty((batch, k), dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or out.ndim != 2 or out.shape[0] != batch or out.shape[1] < k or out.stride(1) != 1 or out.device != dev:
        raise ValueError(f"out must be int64 [{batch}, >= {k}] with a unit last stride on {dev}")
    n_prop = torch.empty((batch,), dtype=torch.int32, device=dev)
    p.drafts, p.n_proposed, p.drafts_stride = out.data_ptr(), n_prop.data_ptr(), out.stride(0) if batch > 1 else max(k, out.shape[1])
    p.n_segments, p.B, p.K, p.ngram_min, p.ngram_max = len(segments), batch, k, lo, hi
    _lib.check(_lib.load().hyd_draft_lookup(C.byref(p), torch.cuda.current_stream().cuda_stream))
    del keep
    return out[:, :k], n_prop


# ---- acceptance ---------------------------------------------------------------------------------------------------------------
def new_state(rows: int, max_new_tokens: int, pad: int, device=None, logprobs: bool = False):
    """(out int64 [rows, max_new_tokens] of pad, length / reason int32 [rows] = 0, stop_index int32 [rows] = -1, out_logprobs f32
    [rows, max_new_tokens] = 0 or None): the state hyd_draft_accept keeps, as a generation starts it."""
    return (torch.full((rows, max_new_tokens), pad, dtype=torch.int64, device=device),
            torch.zeros((rows,), dtype=torch.int32, device=device), torch.zeros((rows,), dtype=torch.int32, device=device),
            torch.full((rows,), -1, dtype=torch.int32, device=device),
            torch.zeros((rows, max_new_tokens), dtype=torch.float32, device=device) if logprobs else None)


def accept_reference(fed: Tensor, sampled: Tensor, out: Tensor, length: Tensor, reason: Tensor, stop_index: Tensor, start_pos: Tensor,
                     shared_len: Optional[Tensor], eos: Sequence[int], pad: int, max_new_tokens: int, retire: bool = True,
                     logprobs: Optional[Tensor] = None, out_logprobs: Optional[Tensor] = None):
    """The rule hyd_draft_accept implements, row by row on CPU tensors, updating out / length / reason / stop_index (/ out_logprobs)
    in place -> (feed int64 [rows], next_pos int64 [rows], accepted int32 [rows], running rows).  fed / sampled int64 [rows, T]:
    column 0 of fed is the last emitted token, the others are drafts; sampled[b, i] was drawn behind fed[b, i].  A row with
    reason != 0 or length >= max_new_tokens has finished and does not change.  Otherwise n = the leading i < T - 1 with
    fed[b, i + 1] == sampled[b, i]; sampled[b, 0 .. n] is emitted, cut behind its first EOS id (kept, reason 1) and at
    max_new_tokens (reason 0); the next step feeds the last emitted token at start_pos + length - 1.  A finished row is fed pad
    at shared_len - 1 (retire), the position that takes it out of the unique K/V stream."""
    rows, T = fed.shape
    eos = list(eos)
    feed = torch.empty((rows,), dtype=torch.int64)
    next_pos = torch.empty((rows,), dtype=torch.int64)
    accepted = torch.zeros((rows,), dtype=torch.int32)
    live = 0
    for b in range(rows):
        ln, r, last = int(length[b]), int(reason[b]), pad
        if r == 0 and ln < max_new_tokens:
            n = 0
            while n < T - 1 and int(fed[b, n + 1]) == int(sampled[b, n]):
                n += 1
            toks = sampled[b, : min(n + 1, max_new_tokens - ln)].tolist()
            for i, t in enumerate(toks):
                if t in eos:
                    toks = toks[: i + 1]
                    r = 1
                    reason[b], stop_index[b] = 1, eos.index(t)
                    break
            e = len(toks)
            out[b, ln: ln + e] = torch.tensor(toks, dtype=torch.int64)
            if logprobs is not None and out_logprobs is not None:
                out_logprobs[b, ln: ln + e] = logprobs[b, :e]
            ln += e
            length[b] = ln
            accepted[b] = e - 1
            last = toks[-1]
        running = r == 0 and ln < max_new_tokens
        live += int(running)
        feed[b] = last if running else pad
        if running or not retire:
            next_pos[b] = int(start_pos[b]) + ln - 1
        else:
            next_pos[b] = (int(shared_len[b]) if shared_len is not None else 0) - 1
    return feed, next_pos, accepted, live


def accept_stop_reference(fed: Tensor, sampled: Tensor, out: Tensor, length: Tensor, reason: Tensor, stop_index: Tensor, start_pos: Tensor,
                          shared_len: Optional[Tensor], eos: Sequence[int], pad: int, max_new_tokens: int, retire: bool = True,
                          logprobs: Optional[Tensor] = None, out_logprobs: Optional[Tensor] = None, *, stop=None,
                          gen: Optional[Tensor] = None, gen_len: Optional[Tensor] = None, states: Optional[tuple] = None):
    """The rule hyd_draft_accept_stop implements, row by row on CPU tensors: accept_reference's arguments and return value, plus
    stop (a stopping.StopSpec of which only .stops and .include_stop are read -- EOS ids and pad are the arguments), the
    penalties' lists gen int32 [rows, stride] / gen_len int32 [rows], and states = (step_state_after, state) as in
    accept_states_reference; all updated in place.  A running row's CANDIDATE sequence is its kept output followed by the run
    sampled[b, 0 .. e0), e0 = min(n + 1, max_new_tokens - length).  The run ends at the first of its columns c at which the
    candidate holds an EOS id (reason 1, the lowest id index) or -- otherwise -- ends a stop sequence, window
    candidate[c + 1 - len_k .. c] never reaching in front of column 0 (reason 2, the lowest k): e = tokens up to and including
    that column, else e0.  The e tokens (and log-probs) are written; a stop match without include_stop pads its len_k columns
    and the row's length becomes c + 1 - len_k, which may lie below the length before the step.  accepted = e - 1, state =
    step_state_after[b, e - 1], gen receives the e tokens at gen_len .. (positions < stride only) and gen_len += e: all of the
    final e, before the trim.  Finished rows do not change."""
    rows, T = fed.shape
    eos = list(eos)
    stops = [list(s) for s in (stop.stops if stop is not None else ())]
    include = bool(stop.include_stop) if stop is not None else False
    feed = torch.empty((rows,), dtype=torch.int64)
    next_pos = torch.empty((rows,), dtype=torch.int64)
    accepted = torch.zeros((rows,), dtype=torch.int32)
    live = 0
    for b in range(rows):
        ln, r, last = int(length[b]), int(reason[b]), pad
        if r == 0 and ln < max_new_tokens:
            n = 0
            while n < T - 1 and int(fed[b, n + 1]) == int(sampled[b, n]):
                n += 1
            e = min(n + 1, max_new_tokens - ln)
            cand = out[b, :ln].tolist() + sampled[b, :e].tolist()
            which, trim = -1, 0
            for c in range(ln, ln + e):
                if cand[c] in eos:
                    r, which = 1, eos.index(cand[c])
                else:
                    hit = [k for k, s in enumerate(stops) if c + 1 >= len(s) and cand[c + 1 - len(s): c + 1] == s]
                    if hit:
                        r, which = 2, hit[0]
                        trim = 0 if include else len(stops[which])
                if r != 0:
                    e = c + 1 - ln
                    break
            out[b, ln: ln + e] = torch.tensor(cand[ln: ln + e], dtype=torch.int64)
            if logprobs is not None and out_logprobs is not None:
                out_logprobs[b, ln: ln + e] = logprobs[b, :e]
            if gen is not None:
                gl = int(gen_len[b])
                for i in range(e):
                    if 0 <= gl + i < gen.shape[1]:
                        gen[b, gl + i] = cand[ln + i]
                gen_len[b] = gl + e
            if states is not None:
                states[1][b] = states[0][b, e - 1]
            accepted[b] = e - 1
            last = cand[ln + e - 1]
            ln += e
            if trim:
                out[b, ln - trim: ln] = pad
                ln -= trim
            length[b] = ln
            if r != 0:
                reason[b], stop_index[b] = r, which
        running = r == 0 and ln < max_new_tokens
        live += int(running)
        feed[b] = last if running else pad
        if running or not retire:
            next_pos[b] = int(start_pos[b]) + ln - 1
        else:
            next_pos[b] = (int(shared_len[b]) if shared_len is not None else 0) - 1
    return feed, next_pos, accepted, live


def draft_accept(fed: Tensor, sampled: Tensor, out: Tensor, length: Tensor, reason: Tensor, stop_index: Tensor, live: Tensor,
                 start_pos: Tensor, shared_len: Optional[Tensor], eos: Sequence[int], pad: int, max_new_tokens: int,
                 retire: bool = True, logprobs: Optional[Tensor] = None, out_logprobs: Optional[Tensor] = None,
                 states: Optional[tuple] = None, stop=None, gen: Optional[Tensor] = None, gen_len: Optional[Tensor] = None,
                 stop_tokens: Optional[Tensor] = None):
    """hyd_draft_accept, one launch -> (feed, next_pos int64 [rows], accepted int32 [rows]); the rows still running are ADDED to
    live (int32 [1], a slot the caller zeroed).  The state tensors are those of new_state; CPU tensors take accept_reference.
    states = (step_state_after int32 [rows, T], state int32 [rows]): hyd_draft_accept_states -- a row that emits e >= 1 tokens
    also gets state[b] = step_state_after[b, e - 1] (accept_states_reference).  stop (a stopping.StopSpec: its stop sequences
    and include_stop) or gen / gen_len (int32 [rows, stride <= GEN_MAX] / [rows], the penalties' lists) given:
    hyd_draft_accept_stop, which judges every emitted token by the stop rules and appends the emitted tokens to the lists
    (accept_stop_reference); without them the calls are exactly those made before.  stop_tokens: stop.stop_table(device)[0],
    uploaded once by a loop that calls this every step (None: uploaded here).  Nothing else synchronises."""
    rows, T = fed.shape
    if (gen is None) != (gen_len is None):
        raise ValueError("gen and gen_len go together")
    if gen is not None and (gen.dtype != torch.int32 or gen.ndim != 2 or gen.shape[0] != rows or not gen.is_contiguous() or gen.device != fed.device
                            or gen.shape[1] > _lib.SAMPLE_GEN_MAX or gen_len.dtype != torch.int32 or gen_len.shape != (rows,)
                            or not gen_len.is_contiguous() or gen_len.device != fed.device):
        raise ValueError(f"gen must be a contiguous int32 [{rows}, <= {_lib.SAMPLE_GEN_MAX}] and gen_len int32 [{rows}] on {fed.device}")
    if stop is not None and (len(stop.stops) > _lib.STOP_MAX_SEQS or any(not 1 <= len(s) <= _lib.STOP_MAX_LEN for s in stop.stops)):
        raise ValueError(f"stop: at most {_lib.STOP_MAX_SEQS} sequences of 1 to {_lib.STOP_MAX_LEN} tokens")
    if states is not None:
        after, st = states
        if (after.dtype != torch.int32 or after.shape != (rows, T) or not after.is_contiguous() or after.device != fed.device
                or st.dtype != torch.int32 or st.shape != (rows,) or not st.is_contiguous() or st.device != fed.device):
            raise ValueError(f"states must be contiguous int32 ([{rows}, {T}], [{rows}]) on {fed.device}")
    if fed.dtype != torch.int64 or sampled.dtype != torch.int64 or sampled.shape != fed.shape:
        raise ValueError(f"fed / sampled must be int64 [rows, T], got {tuple(fed.shape)} {fed.dtype} / {tuple(sampled.shape)} {sampled.dtype}")
    if not 1 <= T <= MAX_DRAFTS + 1:
        raise ValueError(f"T = {T} tokens per row: 1 to {MAX_DRAFTS + 1}")
    if out.dtype != torch.int64 or out.ndim != 2 or out.shape[0] != rows or out.stride(1) != 1 or not 1 <= max_new_tokens <= out.shape[1]:
        raise ValueError(f"out must be int64 [{rows}, >= max_new_tokens = {max_new_tokens}] with a unit last stride, got {tuple(out.shape)} {out.dtype}")
    dev = fed.device
    for name, x, n in (("length", length, rows), ("reason", reason, rows), ("stop_index", stop_index, rows), ("live", live, 1)):
        if x.dtype != torch.int32 or x.shape != (n,) or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"{name} must be a contiguous int32 [{n}] on {dev}, got {tuple(x.shape)} {x.dtype} on {x.device}")
    for name, x in (("start_pos", start_pos), ("shared_len", shared_len)):
        if x is not None and (x.dtype != torch.int64 or x.shape != (rows,) or not x.is_contiguous() or x.device != dev):
            raise ValueError(f"{name} must be a contiguous int64 [{rows}] on {dev}")
    if len(eos) > _lib.STOP_MAX_EOS:
        raise ValueError(f"{len(eos)} EOS ids: at most {_lib.STOP_MAX_EOS}")
    if (logprobs is None) != (out_logprobs is None):
        raise ValueError("logprobs and out_logprobs go together")
    if logprobs is not None and (logprobs.dtype != torch.float32 or logprobs.shape != fed.shape or out_logprobs.dtype != torch.float32
                                 or out_logprobs.shape != out.shape or out_logprobs.stride() != out.stride()):
        raise ValueError("logprobs must be float32 [rows, T] and out_logprobs float32 with out's shape and strides")
    if dev.type != "cuda":
        rest = (out, length, reason, stop_index, start_pos, shared_len, eos, pad, max_new_tokens, retire, logprobs, out_logprobs)
        if stop is not None or gen is not None:
            feed, pos, acc, n = accept_stop_reference(fed, sampled, *rest, stop=stop, gen=gen, gen_len=gen_len, states=states)
        else:
            feed, pos, acc, n = (accept_reference(fed, sampled, *rest) if states is None else
                                 accept_states_reference(fed, sampled, *states, *rest))
        live += n
        return feed, pos, acc
    fed, sampled = fed.contiguous(), sampled.contiguous()
    feed = torch.empty((rows,), dtype=torch.int64, device=dev)
    next_pos = torch.empty((rows,), dtype=torch.int64, device=dev)
    accepted = torch.empty((rows,), dtype=torch.int32, device=dev)
    p = _lib.DraftAcceptParams()
    p.fed, p.sampled, p.out, p.length, p.reason = fed.data_ptr(), sampled.data_ptr(), out.data_ptr(), length.data_ptr(), reason.data_ptr()
    p.stop_index, p.accepted, p.live, p.start_pos = stop_index.data_ptr(), accepted.data_ptr(), live.data_ptr(), start_pos.data_ptr()
    if shared_len is not None:
        p.shared_len = shared_len.data_ptr()
    if logprobs is not None:
        logprobs = logprobs.contiguous()
        p.logprobs, p.out_logprobs = logprobs.data_ptr(), out_logprobs.data_ptr()
    p.feed, p.next_pos = feed.data_ptr(), next_pos.data_ptr()
    p.out_stride, p.pad = (out.stride(0) if rows > 1 else out.shape[1]), pad
    for i, e in enumerate(eos):
        p.eos[i] = e
    p.rows, p.T, p.n_eos, p.max_new_tokens, p.retire = rows, T, len(eos), max_new_tokens, int(bool(retire))
    if stop is not None or gen is not None:
        sp, table = None, None
        if stop is not None:
            sp = _lib.StopParams()
            lens = [len(s) for s in stop.stops]
            table = stop_tokens if stop_tokens is not None else stop.stop_table(dev)[0] if lens else None
            if table is not None and (table.dtype != torch.int64 or table.shape != (len(lens), _lib.STOP_MAX_LEN) or not table.is_contiguous()
                                      or table.device != dev):
                raise ValueError(f"stop_tokens must be stop.stop_table(device)[0]: a contiguous int64 [{len(lens)}, {_lib.STOP_MAX_LEN}] on {dev}")
            sp.stop_tokens = table.data_ptr() if lens else None
            for k, n in enumerate(lens):
                sp.stop_lens[k] = n
            sp.n_stop, sp.include_stop = len(lens), int(bool(stop.include_stop))
        after, st = (None, None) if states is None else (states[0].data_ptr(), states[1].data_ptr())
        _lib.check(_lib.load().hyd_draft_accept_stop(
            C.byref(p), None if sp is None else C.byref(sp), after, st, None if gen is None else gen.data_ptr(),
            None if gen is None else gen_len.data_ptr(), 0 if gen is None else gen.shape[1], torch.cuda.current_stream().cuda_stream))
        del table
    elif states is None:
        _lib.check(_lib.load().hyd_draft_accept(C.byref(p), torch.cuda.current_stream().cuda_stream))
    else:
        _lib.check(_lib.load().hyd_draft_accept_states(C.byref(p), states[0].data_ptr(), states[1].data_ptr(), torch.cuda.current_stream().cuda_stream))
    return feed, next_pos, accepted


# ---- drafts under a token automaton (constraint.TokenDFA) ---------------------------------------------------------------------
# A state that allows exactly one token FORCES it: a draft of that token is accepted with probability 1, because the masked sampler
# can draw nothing else (jump-forward decoding).  Per step: the drafts go into fed[:, 1:], constrain_drafts walks them through the
# automaton -- forced states replace drafts, a rejected draft ends the row's proposal -- and gives step_state [B, T], the state
# from which the draw behind each fed token is taken; the sampler draws the B * T logits rows with step_state flattened as its
# state array and advances it in place; accept (states=) then hands every row the state behind its last emitted token.
def constrain_drafts_reference(dfa, state: Tensor, fed: Tensor, n_proposed: Optional[Tensor] = None, only_forced: bool = False):
    """The rule hyd_draft_constrain implements, row by row on CPU tensors -> (step_state int32 [B, T], n_forced int32 [B]); fed
    (int64 [B, T], column 0 the last emitted token, whose effect is already in state) and n_proposed (int32 [B] or None) are
    updated in place.  Row b, s = state[b], step_state[b, 0] = s; for j = 0 .. K - 1:
      1. s is a state and dfa.forced[s] >= 0: fed[b, j + 1] = forced[s]; n_forced counts it; n_proposed[b] = max(., j + 1);
      2. otherwise, only_forced: the chain ends -- n_proposed[b] = min(., j), the remaining drafts keep what they hold, the
         remaining step states are -1;
      3. s is a state: t = fed[b, j + 1], e = next[s, t] (REJECT for t outside [0, n)).  REJECT: the draft can never be drawn --
         n_proposed[b] = min(., j), every later step state is -1; FREE: s = -2; e in [0, S): s = e; anything else: s = -1;
      4. s is no state: the row is unconstrained, s and the draft stay;
      5. step_state[b, j + 1] = s."""
    B, T = fed.shape
    S, n = dfa.next.shape
    nxt, forced = dfa.next.cpu(), dfa.forced.cpu()
    step_state = torch.empty((B, T), dtype=torch.int32)
    n_forced = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        s = int(state[b])
        step_state[b, 0] = s
        np_ = int(n_proposed[b]) if n_proposed is not None else 0
        ended = False
        for j in range(T - 1):
            if not ended:
                inside = 0 <= s < S
                t = int(forced[s]) if inside else -1
                if t >= 0:
                    fed[b, j + 1] = t
                    n_forced[b] += 1
                    np_ = max(np_, j + 1)
                elif only_forced:
                    ended = True
                else:
                    t = int(fed[b, j + 1])
                if not ended and inside:
                    e = int(nxt[s, t]) if 0 <= t < n else DFA_REJECT
                    if e == DFA_REJECT:
                        ended = True
                    else:
                        s = -2 if e == DFA_FREE else e if 0 <= e < S else -1
                if ended:
                    np_ = min(np_, j)
            step_state[b, j + 1] = -1 if ended else s
        if n_proposed is not None:
            n_proposed[b] = np_
    return step_state, n_forced


def constrain_drafts(dfa, state: Tensor, fed: Tensor, n_proposed: Optional[Tensor] = None, only_forced: bool = False,
                     step_state: Optional[Tensor] = None, n_forced: Optional[Tensor] = None):
    """hyd_draft_constrain, one launch, no host synchronisation -> (step_state int32 [B, T], n_forced int32 [B]); CPU tensors take
    constrain_drafts_reference.  fed int64 [B, T] with a unit last stride (a row stride wider than T is honoured) and n_proposed
    are updated in place; step_state / n_forced: buffers to write (a generation allocates them once)."""
    B, T = fed.shape
    if fed.dtype != torch.int64 or fed.ndim != 2 or not 2 <= T <= MAX_DRAFTS + 1:
        raise ValueError(f"fed must be int64 [B, T] with T = K + 1 in 2 .. {MAX_DRAFTS + 1}, got {tuple(fed.shape)} {fed.dtype}")
    dev = fed.device
    for name, x in (("state", state), ("n_proposed", n_proposed)):
        if x is not None and (x.dtype != torch.int32 or x.shape != (B,) or not x.is_contiguous() or x.device != dev):
            raise ValueError(f"{name} must be a contiguous int32 [{B}] on {dev}")
    if dev.type != "cuda":
        ss, nf = constrain_drafts_reference(dfa, state, fed, n_proposed, only_forced)
        if step_state is not None:
            step_state.copy_(ss)
            ss = step_state
        if n_forced is not None:
            n_forced.copy_(nf)
            nf = n_forced
        return ss, nf
    if fed.stride(1) != 1 or (B > 1 and fed.stride(0) < T):
        raise ValueError("fed must have a unit last stride and rows that do not overlap")
    if dfa.next.device != dev:
        raise ValueError(f"the automaton is on {dfa.next.device}, fed on {dev}")
    if step_state is None:
        step_state = torch.empty((B, T), dtype=torch.int32, device=dev)
    if n_forced is None:
        n_forced = torch.empty((B,), dtype=torch.int32, device=dev)
    if step_state.shape != (B, T) or step_state.dtype != torch.int32 or not step_state.is_contiguous() or step_state.device != dev:
        raise ValueError(f"step_state must be a contiguous int32 [{B}, {T}] on {dev}")
    if n_forced.shape != (B,) or n_forced.dtype != torch.int32 or not n_forced.is_contiguous() or n_forced.device != dev:
        raise ValueError(f"n_forced must be a contiguous int32 [{B}] on {dev}")
    forced = dfa.forced
    p = _lib.DraftConstrainParams()
    p.state, p.fed, p.forced, p.next = state.data_ptr(), fed.data_ptr(), forced.data_ptr(), dfa.next.data_ptr()
    if n_proposed is not None:
        p.n_proposed = n_proposed.data_ptr()
    p.step_state, p.n_forced = step_state.data_ptr(), n_forced.data_ptr()
    p.fed_stride, p.next_stride = (fed.stride(0) if B > 1 else max(T, fed.stride(0))), dfa.next.stride(0) if dfa.next.shape[0] > 1 else dfa.next.shape[1]
    p.B, p.K, p.n_states, p.n, p.only_forced = B, T - 1, dfa.next.shape[0], dfa.next.shape[1], int(bool(only_forced))
    _lib.check(_lib.load().hyd_draft_constrain(C.byref(p), torch.cuda.current_stream().cuda_stream))
    return step_state, n_forced


def accept_states_reference(fed: Tensor, sampled: Tensor, step_state_after: Tensor, state: Tensor, out: Tensor, length: Tensor,
                            reason: Tensor, stop_index: Tensor, *args, **kw):
    """The rule hyd_draft_accept_states implements: accept_reference (same arguments behind `state`, same return value), and a
    row that emits e >= 1 tokens in this call also gets state[b] = step_state_after[b, e - 1] -- step_state_after int32
    [rows, T] is the step's state array after the sampler advanced it: entry (b, i) is the state behind sampled[b, i].  A
    finished row, or one that emits nothing, keeps its state."""
    before = length.clone()
    ret = accept_reference(fed, sampled, out, length, reason, stop_index, *args, **kw)
    for b in range(fed.shape[0]):
        e = int(length[b]) - int(before[b])
        if e >= 1:
            state[b] = step_state_after[b, e - 1]
    return ret


# ---- the multi-token attention, assembled from existing operators ------------------------------------------------------------
def _hip_ops():
    from . import attention, flash

    return dict(
        seqlen=flash.flash_attention_seqlen,
        causal=lambda q, k, v: flash.flash_attention(q, k, v, causal=True),
        level=attention._level_pass,
        combine=attention._combine_many,
    )


def assembled_causal_tail_attention(q: Tensor, k: Tensor, v: Tensor, seq_lens: Tensor, shared_ks=(), shared_vs=(), shared_cu_seq_lens=None,
                                    shared_max_seq_lens=None, use_varlens=None, ops: Optional[dict] = None) -> Tensor:
    """The DEFINITION of a multi-token decode step's attention, from launches that existed before the causal-tail kernels: q
    [B, T, Hq, D] are the last T tokens of their sequences, k / v [B, S, Hkv, D] the unique caches with the T new keys already
    in place, seq_lens [B] their lengths (new keys included; a row shorter than T takes no part in the unique passes).
      1. the OLD keys: every query over the first seq_lens - T keys (flash_attention_seqlen, non-causal -- all of them are visible);
      2. the NEW keys: the T x T block k[b, seq_lens - T : seq_lens], causal (flash_attention(causal=True));
      3. one non-causal pass per shared level;
    merged by log-sum-exp (combine_lse).  Two launches per layer more than the fused causal call, and a gather: this is what
    the kernels are tested against and what shapes they refuse fall back on, not the product path.
    ops: the four operators (seqlen, causal, level, combine) -- the HIP ones by default; a test passes torch ones to check
    the assembly itself on the CPU."""
    ops = ops or _hip_ops()
    B, T, Hq, D = q.shape
    n_levels = len(shared_ks)
    shared_cu_seq_lens = shared_cu_seq_lens or [None] * n_levels
    shared_max_seq_lens = shared_max_seq_lens or [None] * n_levels
    use_varlens = use_varlens or [False] * n_levels
    sl = seq_lens.long()
    part = sl >= T  # rows that take part in the unique passes
    old = torch.where(part, sl - T, torch.zeros_like(sl))
    outs, lses = [], []
    for sk, sv, scu, smax, uv in zip(shared_ks, shared_vs, shared_cu_seq_lens, shared_max_seq_lens, use_varlens):
        o, l = ops["level"](q, sk, sv, scu, smax, uv)
        outs.append(o)
        lses.append(l)
    o_old, l_old = ops["seqlen"](q, k, v, old.to(seq_lens.dtype))
    outs.append(o_old)
    lses.append(l_old)
    idx = (old[:, None] + torch.arange(T, device=q.device)[None, :]).clamp_(max=k.shape[1] - 1)  # [B, T] (rows out of it: masked below)
    gi = idx[:, :, None, None].expand(B, T, k.shape[2], k.shape[3])
    o_new, l_new = ops["causal"](q, k.gather(1, gi), v.gather(1, gi))  # lse [B, Hq, T]
    l_new = l_new.transpose(1, 2).contiguous()
    o_new = torch.where(part[:, None, None, None], o_new, torch.zeros_like(o_new))
    l_new = torch.where(part[:, None, None], l_new, torch.full_like(l_new, float("-inf")))
    outs.append(o_new)
    lses.append(l_new)
    return ops["combine"](outs, lses)
