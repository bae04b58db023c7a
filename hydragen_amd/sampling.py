"""Sampling cuts in torch: the definition `hyd_sample_tokens_filtered` (csrc/sample_filter.hip) implements, evaluated in
float64.  It is the fallback for tensors the kernel does not take (the fan-out first token with num_samples > 1, CPU
tensors) and the reference of the tests.

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
from typing import Optional

import torch
from torch import Tensor


def filters_active(top_k: Optional[int], top_p: Optional[float], min_p: Optional[float]) -> bool:
    return bool(top_k) or (top_p is not None and top_p < 1.0) or bool(min_p)


def check_filters(top_k: Optional[int], top_p: Optional[float], min_p: Optional[float]) -> None:
    if top_k is not None and top_k < 0:
        raise ValueError(f"top_k {top_k} must be >= 0 (0 or None = off)")
    if top_p is not None and not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p {top_p} must be in (0, 1] (1 or None = off)")
    if min_p is not None and not (0.0 <= min_p <= 1.0):
        raise ValueError(f"min_p {min_p} must be in [0, 1] (0 or None = off)")


@torch.no_grad()
def kept_mask(logits: Tensor, top_k: Optional[int] = None, top_p: Optional[float] = None,
              min_p: Optional[float] = None) -> Tensor:
    """[..., n] bool: the tokens the cuts keep (module docstring), computed in float64."""
    check_filters(top_k, top_p, min_p)
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
def filter_logits(logits: Tensor, top_k: Optional[int] = None, top_p: Optional[float] = None,
                  min_p: Optional[float] = None) -> Tensor:
    """`logits` with every token the cuts remove (and every NaN) set to -inf, in the input dtype."""
    return logits.masked_fill(~kept_mask(logits, top_k, top_p, min_p), -math.inf)
