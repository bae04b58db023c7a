"""Stop conditions of a generation: the definition `hyd_stop_update` (include/hydragen_hip.h, csrc/stop_update.hip) implements,
in torch on CPU tensors, twice -- one decode step at a time (`stop_update_reference`, the kernel's own form) and as a scan
over a whole generation (`truncate_reference`) -- so that the tests can hold the two against each other and the kernel against
both.

Rules for row b's token of step t (t = 0: the token drawn from the prefill logits), in this order:
  (a) the row finished at an earlier step: out[b, t] = pad, nothing else changes;
  (b) otherwise out[b, t] = tok[b]; the token is one of the EOS ids: reason 1, stop_index = its place in the list, the EOS token
      is kept, length = t + 1;
  (c) otherwise the stop sequences in list order: sequence k of `len` tokens matches when t + 1 >= len and out[b, t + 1 - len .. t]
      equals it (never reaching back into the prompt, never across columns a finished row has padded); the lowest matching k
      gives reason 2, stop_index = k; include_stop False: the matched columns become pad and length = t + 1 - len, True: they
      stay and length = t + 1;
  (c') with a limit per row (hyd_stop_update_rows): otherwise, if t + 1 >= max_len[b], the row finishes at its own limit: reason 3,
      length = t + 1, stop_index stays -1 (an entry <= 0 finishes the row at step 0 with length 1; generate() refuses limits < 1).
      Rules (b) and (c) win at the same step: an EOS exactly at the limit is reason 1, and a stop sequence that would complete a
      step after the limit is never matched;
  (d) otherwise the row keeps running: length = t + 1.
Matching is on token ids.  It is not string matching: a stop string that the tokenizer splits differently in context (a merged
" \\n\\n" token, a word boundary inside a token) is not found; pass every tokenisation that should stop."""

from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import torch
from torch import Tensor

MAX_EOS, MAX_SEQS, MAX_LEN = 16, 32, 16  # HYD_STOP_MAX_EOS, HYD_STOP_MAX_SEQS, HYD_STOP_MAX_LEN
RUNNING, EOS, STOP, LIMIT = 0, 1, 2, 3    # finish reasons


class Finish(NamedTuple):
    """Per-row result of a generation with stop conditions, int32 [B] each: kept tokens, finish reason (0 = ran to
    max_new_tokens, 1 = EOS, 2 = stop sequence, 3 = the row's own limit of a per-row max_new_tokens) and which EOS id / stop
    sequence matched (-1: none)."""
    lengths: Tensor
    reasons: Tensor
    stop_index: Tensor


@dataclass(frozen=True)
class StopSpec:
    """Normalised stop conditions: EOS ids, stop sequences (tuples of token ids), the pad id and include_stop."""
    eos: tuple = ()
    stops: tuple = ()
    pad: int = 0
    include_stop: bool = False

    def stop_table(self, device=None):
        """(tokens int64 [n_stop, MAX_LEN] zero-filled, lens list) -- the layout hyd_stop_params.stop_tokens takes."""
        tab = torch.zeros((len(self.stops), MAX_LEN), dtype=torch.int64)
        for k, s in enumerate(self.stops):
            tab[k, : len(s)] = torch.tensor(s, dtype=torch.int64)
        return (tab if device is None else tab.to(device)), [len(s) for s in self.stops]


def _ints(x, what):
    if isinstance(x, Tensor):
        if x.ndim != 1 or x.is_floating_point() or x.dtype == torch.bool:
            raise ValueError(f"{what} must be a 1-d tensor of token ids, got {tuple(x.shape)} {x.dtype}")
        x = x.tolist()
    out = []
    for v in x:
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: token ids are ints, got {v!r}")
        out.append(int(v))
    return tuple(out)


def check_stop(eos_token_id=None, stop=None, pad_token_id: Optional[int] = None, include_stop: bool = False,
               vocab_size: Optional[int] = None) -> StopSpec:
    """Validate and normalise (the limits are the header's).  eos_token_id: None, an int or a list / tuple of ints; stop: None or a
    list of token-id sequences (lists, tuples or 1-d tensors, ragged); pad_token_id: None = the first EOS id if any, else 0."""
    if eos_token_id is None:
        eos = ()
    elif isinstance(eos_token_id, (list, tuple, Tensor)):
        eos = _ints(eos_token_id, "eos_token_id")
    else:
        eos = _ints([eos_token_id], "eos_token_id")
    if len(eos) > MAX_EOS:
        raise ValueError(f"{len(eos)} EOS ids: at most {MAX_EOS}")
    if stop is not None and (isinstance(stop, (str, bytes)) or (isinstance(stop, Tensor) and stop.ndim != 2)):
        raise ValueError("stop must be a list of token-id sequences (no tokenizer is involved: strings are not accepted)")
    stops = tuple(_ints(s, f"stop[{k}]") for k, s in enumerate(stop if stop is not None else ()))
    if len(stops) > MAX_SEQS:
        raise ValueError(f"{len(stops)} stop sequences: at most {MAX_SEQS}")
    for k, s in enumerate(stops):
        if not 1 <= len(s) <= MAX_LEN:
            raise ValueError(f"stop[{k}] holds {len(s)} tokens: 1 to {MAX_LEN}")
    pad = (eos[0] if eos else 0) if pad_token_id is None else pad_token_id
    if isinstance(pad, bool) or not isinstance(pad, int):
        raise ValueError(f"pad_token_id must be an int, got {pad!r}")
    ids = [("pad_token_id", pad)] + [("eos_token_id", e) for e in eos] + [(f"stop[{k}]", v) for k, s in enumerate(stops) for v in s]
    for what, v in ids:
        if v < 0 or (vocab_size is not None and v >= vocab_size):
            raise ValueError(f"{what} {v} is outside the vocabulary [0, {vocab_size if vocab_size is not None else 'V'})")
    return StopSpec(eos, stops, int(pad), bool(include_stop))


def new_state(rows: int, steps: int, spec: StopSpec, device=None):
    """(out int64 [rows, steps] of pad, length int32 [rows] = 0, reason int32 [rows] = 0, stop_index int32 [rows] = -1,
    live int32 [steps] = 0): the state hyd_stop_update keeps, as a generation starts it."""
    return (torch.full((rows, steps), spec.pad, dtype=torch.int64, device=device),
            torch.zeros((rows,), dtype=torch.int32, device=device), torch.zeros((rows,), dtype=torch.int32, device=device),
            torch.full((rows,), -1, dtype=torch.int32, device=device), torch.zeros((steps,), dtype=torch.int32, device=device))


def stop_update_reference(tok: Tensor, t: int, spec: StopSpec, out: Tensor, length: Tensor, reason: Tensor, stop_index: Tensor,
                          live: Tensor, start_pos: Tensor, shared_len: Optional[Tensor] = None, retire: bool = True,
                          max_len: Optional[Tensor] = None):
    """One step of the rules, row by row, updating out / length / reason / stop_index / live in place -> (feed, next_pos) int64
    [rows]: the token and the position of the next step (a finished row: pad, and -- retire -- shared_len - 1, the position at
    which hyd_rope_append_decode skips the row; -1 without shared_len).  max_len int [rows] or None: rule (c')."""
    rows = tok.shape[0]
    if not 0 <= t < out.shape[1]:
        raise ValueError(f"t {t} outside [0, {out.shape[1]})")
    feed = torch.empty((rows,), dtype=torch.int64)
    next_pos = torch.empty((rows,), dtype=torch.int64)
    for b in range(rows):
        tk = int(tok[b])
        if int(reason[b]) != RUNNING:
            out[b, t] = spec.pad
        else:
            out[b, t] = tk
            length[b] = t + 1
            if tk in spec.eos:
                reason[b], stop_index[b] = EOS, spec.eos.index(tk)
            else:
                for k, s in enumerate(spec.stops):
                    n = len(s)
                    if t + 1 >= n and out[b, t + 1 - n : t + 1].tolist() == list(s):
                        reason[b], stop_index[b] = STOP, k
                        if not spec.include_stop:
                            out[b, t + 1 - n : t + 1] = spec.pad
                            length[b] = t + 1 - n
                        break
            if int(reason[b]) == RUNNING and max_len is not None and t + 1 >= int(max_len[b]):
                reason[b] = LIMIT
        running = int(reason[b]) == RUNNING
        live[t] += int(running)
        feed[b] = tk if running else spec.pad
        if running or not retire:
            next_pos[b] = int(start_pos[b]) + t
        else:
            next_pos[b] = (int(shared_len[b]) if shared_len is not None else 0) - 1
    return feed, next_pos


def finish_steps(tokens: Tensor, spec: StopSpec, max_len: Optional[Tensor] = None):
    """max_len int [B] or None: rule (c'), a row not finished before step max(max_len, 1) - 1 finishes there with reason 3.
    For sampled tokens [B, T] (what a generation without stop conditions returns): (step int64 [B] at which each row
    finishes, T for a row that never does; reason int32 [B]; stop_index int32 [B]).  A scan over whole rows: every (step,
    condition) hit is computed at once and the earliest step -- at that step EOS before stops, then the lowest k -- is taken.
    Before a row finishes its output equals its tokens, so hits may be looked for in `tokens` itself."""
    B, T = tokens.shape
    tokens = tokens.long()
    never = T
    # hit[c][b, t]: condition c is met by the token of step t; conditions ordered EOS ids, then stop sequences
    hits = [tokens == e for e in spec.eos]
    for s in spec.stops:
        n = len(s)
        h = torch.zeros((B, T), dtype=torch.bool)
        if n <= T:
            win = tokens.unfold(1, n, 1)  # [B, T - n + 1, n]: window ending at step t = n - 1 + i
            h[:, n - 1 :] = (win == torch.tensor(s, dtype=torch.int64)).all(-1)
        hits.append(h)
    step = torch.full((B,), never, dtype=torch.int64)
    reason = torch.zeros((B,), dtype=torch.int32)
    index = torch.full((B,), -1, dtype=torch.int32)
    if hits and T:
        cube = torch.stack(hits, 0)  # [C, B, T]
        any_t = cube.any(0)
        fin = any_t.any(1)
        first_t = any_t.int().argmax(1)  # first step with any hit
        at = cube[:, torch.arange(B), first_t]  # [C, B] the conditions met at that step
        first_c = at.int().argmax(0)  # the first in priority order
        step = torch.where(fin, first_t, step)
        is_eos = first_c < len(spec.eos)
        reason = torch.where(fin, torch.where(is_eos, EOS, STOP), 0).to(torch.int32)
        index = torch.where(fin, torch.where(is_eos, first_c, first_c - len(spec.eos)), -1).to(torch.int32)
    if max_len is not None and T:
        at = max_len.reshape(-1).long().clamp(min=1) - 1  # the step of the limit
        cut = (at < step) & (at < T)                      # (a condition met AT the limit's step wins)
        step = torch.where(cut, at, step)
        reason = torch.where(cut, torch.full_like(reason, LIMIT), reason)
        index = torch.where(cut, torch.full_like(index, -1), index)
    return step, reason, index


def truncate_reference(tokens: Tensor, spec: StopSpec, max_len: Optional[Tensor] = None):
    """The whole-generation definition: sampled tokens [B, T] -> (out int64 [B, T], length, reason, stop_index int32 [B]), what a
    generation with `spec` keeps of them.  Columns at and past a row's length hold pad."""
    B, T = tokens.shape
    step, reason, index = finish_steps(tokens, spec, max_len)
    lens = torch.tensor([len(s) for s in spec.stops] + [0], dtype=torch.int64)
    cut = torch.zeros((B,), dtype=torch.int64)
    if not spec.include_stop:
        cut = lens[torch.where(reason == STOP, index.long(), torch.full_like(step, len(spec.stops)))]  # (EOS / running rows: the 0)
    length = torch.where(reason == RUNNING, torch.full_like(step, T), step + 1 - cut)
    keep = torch.arange(T)[None, :] < length[:, None]
    out = torch.where(keep, tokens.long(), torch.full_like(tokens.long(), spec.pad))
    return out, length.to(torch.int32), reason, index


def live_reference(tokens: Tensor, spec: StopSpec, max_len: Optional[Tensor] = None) -> Tensor:
    """int32 [T]: the rows still running after each step (hyd_stop_params.live), from the scan."""
    step, _, _ = finish_steps(tokens, spec, max_len)
    return (step[None, :] > torch.arange(tokens.shape[1])[:, None]).sum(1).to(torch.int32)
