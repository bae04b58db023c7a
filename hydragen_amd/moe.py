"""
Mixture-of-experts MLP: the DEFINITION of routing and of the expert products, and the elementwise error bound that goes with it.
A preparatory module: nothing in the model shell uses it yet -- `from_hf_model` still refuses mixture-of-experts checkpoints and
`LlamaConfig` has no experts -- because there is no GPU path.  This is what a device-routed expert kernel will be held to.

    logits = round16(x @ router_w^T)
    ids, weights = the k largest logits of a row, descending, ties to the lower index; softmax(logits)[ids], renormalized or not
    act[t, j] = round16(silu(x[t] @ Wg[e_j]^T) * (x[t] @ Wu[e_j]^T))          (gate_up[e] = Wg[e] rows, then Wu[e] rows)
    y[t] = sum_j weights[t, j] * (act[t, j] @ Wd[e_j]^T)                      (in j order; rounded once by whoever compares)

The weight layouts are transformers 5's (`experts.gate_up_proj` [E, 2 I, H], `experts.down_proj` [E, H, I], `gate.weight` [E, H]).
"""

from __future__ import annotations

import torch
from torch import Tensor


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


def _routed(x: Tensor, router_w: Tensor, k: int, renormalize: bool):
    return route_reference(torch.nn.functional.linear(x, router_w), k, renormalize)  # the product stays a 16-bit F.linear


def moe_reference(x: Tensor, router_w: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool) -> Tensor:
    """The definition in float64: x [T, H], router_w [E, H], gate_up [E, 2 I, H], down [E, H, I] (all of one 16-bit dtype) ->
    [T, H] float64.  Two 16-bit roundings per token and expert on the way -- the router logits and act -- exactly where the
    kernels round; the output's own rounding is left to the caller of the comparison."""
    ids, w = _routed(x, router_w, k, renormalize)
    out = x.new_zeros(x.shape, dtype=torch.float64)
    for j, y, *_ in _slot_terms(x, gate_up, down, ids):
        out += w[:, j, None] * y
    return out


def moe_error_bound(x: Tensor, router_w: Tensor, gate_up: Tensor, down: Tensor, k: int, renormalize: bool) -> Tensor:
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
    row and 2^-25 for the output."""
    ids, w = _routed(x, router_w, k, renormalize)
    H, I = x.shape[1], down.shape[2]
    u16, tiny = (2.0 ** -8, 0.0) if x.dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    out = x.new_zeros(x.shape, dtype=torch.float64)
    bound = x.new_zeros(x.shape, dtype=torch.float64)
    for j, y, s_act, s_gu, s_wd in _slot_terms(x, gate_up, down, ids):
        wj = w[:, j, None]
        out += wj * y
        bound += wj * ((I * 2.0 ** -23 + u16) * s_act + H * 2.0 ** -23 * s_gu + (k + 5) * 2.0 ** -23 * y.abs() + tiny * s_wd)
    return bound + u16 * out.abs() + tiny
