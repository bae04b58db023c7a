"""Scoring given tokens: the definition `hyd_token_logprobs` (csrc/token_logprob.hip) implements, evaluated in float64, and the
result type of `HydragenLlamaForCausalLM.score()`.  `token_logprobs_reference` is the fallback for CPU tensors and the
reference of the tests.

For one row of logits l (length n) and its target token t, with the VALID logits those that are neither NaN nor -inf and
m = their max:
  * logprob = l_t - m - ln sum exp(l - m) over the valid logits (the sum as 1, the first maximum's term, + the others, through
    log1p: a log-prob of -1e-12 keeps its digits; tests/test_scoring_stress.py holds it to a plain ranking); t outside [0, n): NaN (padding); l_t NaN: NaN; l_t -inf:
    -inf; a row without a valid logit: NaN;
  * greedy = t is the lowest-index maximum of the valid logits (torch.argmax's tie rule: what generate(temperature=0) picks);
  * top-N: the N largest valid logits ordered by (value descending, index ascending) and their log-probs; rows with fewer
    than N valid logits pad with id -1 and log-prob -inf.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

TOP_LOGPROBS_MAX = 20  # HYD_TOP_LOGPROBS_MAX


def check_top_n(top_n: int) -> int:
    if not 0 <= int(top_n) <= TOP_LOGPROBS_MAX:
        raise ValueError(f"top_logprobs {top_n} must be in [0, {TOP_LOGPROBS_MAX}]")
    return int(top_n)


@torch.no_grad()
def token_logprobs_reference(logits: Tensor, targets: Tensor, top_n: int = 0):
    """[R, n] logits, [R] int64 targets -> (logprobs [R] f32, greedy [R] bool, top_ids [R, N] int64, top_logprobs [R, N] f32),
    every output computed in float64 (module docstring)."""
    top_n = check_top_n(top_n)
    assert logits.ndim == 2 and targets.shape == (logits.shape[0],), f"{tuple(logits.shape)} {tuple(targets.shape)}"
    x = logits.double()
    R, n = x.shape
    valid = ~(torch.isnan(x) | (x == -math.inf))
    xm = torch.where(valid, x, torch.full_like(x, -math.inf))
    nvalid = valid.sum(-1)
    has = nvalid > 0
    m = torch.where(has, xm.amax(-1), torch.zeros(R, dtype=x.dtype, device=x.device))
    # the max's own term is exactly 1 (l == m, also for m = +inf)
    w = torch.where(valid, torch.where(xm == m[:, None], torch.ones_like(x), torch.exp(xm - m[:, None])), torch.zeros_like(x))
    first_max = torch.argmax(((xm == m[:, None]) & valid).to(torch.int8), dim=-1)  # argmax returns the first: lowest index
    # ln(1 + the other terms): where the maximum holds nearly all the mass (one logit 30 above the rest: ln sum = 1e-12), log(sum)
    # keeps only the digits of the sum above 2^-52 and depends on the order of the additions -- 5e-4 relative in such a log-prob
    w.scatter_(1, first_max[:, None], 0.0)
    lse = torch.log1p(w.sum(-1))

    def lp_of(v):
        d = torch.where(v == m.reshape(-1, *([1] * (v.ndim - 1))), torch.zeros_like(v), v - m.reshape(-1, *([1] * (v.ndim - 1))))
        return d - lse.reshape(-1, *([1] * (v.ndim - 1)))

    t = targets.long().to(x.device)
    tin = (t >= 0) & (t < n)
    lt = x.gather(1, t.clamp(0, n - 1)[:, None])[:, 0]
    lp = torch.where(tin & has, lp_of(lt), torch.full_like(lt, math.nan))
    greedy = tin & has & (t == first_max)
    if top_n == 0:
        return lp.float(), greedy, torch.empty((R, 0), dtype=torch.int64, device=x.device), \
            torch.empty((R, 0), dtype=torch.float32, device=x.device)
    # (value desc, index asc): a stable sort of the values descending keeps equal values in index order
    order = torch.sort(xm, dim=-1, descending=True, stable=True).indices[:, :min(top_n, n)]
    vals = xm.gather(1, order)
    ok = torch.arange(order.shape[1], device=x.device)[None, :] < nvalid[:, None]
    ids = torch.where(ok, order, torch.full_like(order, -1))
    tlp = torch.where(ok, lp_of(vals), torch.full_like(vals, -math.inf))
    if order.shape[1] < top_n:  # n < N
        pad = top_n - order.shape[1]
        ids = torch.cat([ids, torch.full((R, pad), -1, dtype=ids.dtype, device=x.device)], 1)
        tlp = torch.cat([tlp, torch.full((R, pad), -math.inf, dtype=tlp.dtype, device=x.device)], 1)
    return lp.float(), greedy, ids, tlp.float()


@dataclass
class ScoreResult:
    """What `HydragenLlamaForCausalLM.score()` returns; T = max(target_lens), entries past a row's length are padding."""
    logprobs: Tensor                      # [B, T] f32, NaN past the row's length
    token_greedy: Tensor                  # [B, T] bool, False past the row's length
    sum: Tensor                           # [B] f64: sum of the row's target log-probs
    is_greedy: Tensor                     # [B] bool: every target token is the greedy token (lm-eval's flag)
    top_ids: Optional[Tensor] = None      # [B, T, N] int64 with top_logprobs = N > 0 (-1 past the row's length)
    top_logprobs: Optional[Tensor] = None  # [B, T, N] f32 (-inf past the row's length)
