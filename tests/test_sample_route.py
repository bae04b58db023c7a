"""sampling.sample_route against an independent restatement of its table, over every combination of its inputs, and the
executor (generation.draw_tokens behind sample_from_logits) on CPU logits against the direct composition of the float64 definitions."""
import itertools
import math

import pytest
import torch

from hydragen_amd import sampling
from hydragen_amd.layer_ops import Penalties
from hydragen_amd.llama import HydragenLlamaForCausalLM
from hydragen_amd.sampling import CONSTRAINED, DFA_FREE, DFA_REJECT, FILTERED, PENALIZED, PLAIN, TORCH


def _expected_route(cuda, eligible, rewritten, ns, C, P, F, L, ff, fp):
    """(draw, penalties in torch + push, mask in torch + advance, cuts in torch), row by row of the table.  rewritten: what
    `eligible` (K without num_samples) is of rows that a torch stage has made contiguous."""
    K = eligible and ns == 1
    if C:
        if ns == 1 and (not cuda or (K and (not P or fp))):
            return CONSTRAINED, False, False, False
        # one sample per masked row, log-probs forced on: the filtered kernel wherever a kernel can run
        return (FILTERED, P, True, False) if rewritten else (TORCH, P, True, F)
    if P:
        if K and fp:
            return PENALIZED, False, False, False
        K = rewritten and ns == 1  # "neither" on the result of the torch stage
    if K and (L or (F and ff)):
        return FILTERED, P, False, False
    return (PLAIN if K else TORCH), P, False, F


def test_route_table_over_every_input():
    n = 0
    for args in itertools.product((False, True), (False, True), (False, True), (1, 3), *[(False, True)] * 6):
        assert tuple(sampling.sample_route(*args)) == _expected_route(*args), args
        n += 1
    assert n == 1024
    r = sampling.sample_route(*args)
    with pytest.raises(AttributeError):  # frozen
        r.draw = PLAIN


# ---- CPU draws at temperature 0 --------------------------------------------------------------------------------------------------
V, LEAF, S = 65, 4, 8


class _Shell:
    """sample_from_logits without a model around it: the two switches and the methods themselves."""
    fused_sampling_filters = fused_sampling_penalties = True
    sample_route = HydragenLlamaForCausalLM.sample_route
    sample_from_logits = HydragenLlamaForCausalLM.sample_from_logits


def _automaton():
    from hydragen_amd.constraint import TokenDFA

    g = torch.Generator().manual_seed(11)
    nxt = torch.randint(0, S, (S, V), generator=g, dtype=torch.int32)
    nxt[torch.rand((S, V), generator=g) < 0.6] = DFA_REJECT
    nxt[2] = DFA_REJECT  # a state that allows nothing
    nxt[5, 7], nxt[5, 64] = DFA_FREE, 3
    return TokenDFA(nxt)


@pytest.fixture(scope="module")
def logits():
    return torch.randn(LEAF, V, generator=torch.Generator().manual_seed(5)) * 3.0


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("cuts", [None, dict(top_k=5, top_p=0.8, min_p=0.05), dict(top_p=0.6)])
@pytest.mark.parametrize("P", [False, True])
@pytest.mark.parametrize("C", [False, True])
def test_cpu_draws_equal_the_composed_definitions(logits, C, P, cuts, ns):
    B = LEAF * ns
    cuts = cuts or {}
    dfa = _automaton()
    state0 = torch.tensor([0, 2, 5, -1, 1, 3, 2, S, 4, 6, 7, 5], dtype=torch.int32)[:B].contiguous()
    state = state0.clone()
    g = torch.Generator().manual_seed(9)
    ctx_ids = torch.randint(0, V, (2, 10), generator=g)
    bits = sampling.token_bitmap_reference(ctx_ids, None, V)
    gen0 = torch.randint(0, V, (B, 6), generator=g, dtype=torch.int32)
    len0 = torch.tensor([2, 0, 5, 3] * ns, dtype=torch.int32)
    pen_args = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.7,
                    logit_bias=(torch.tensor([1, 30, 64]), torch.tensor([2.0, -math.inf, -1.5])))

    def penalties(append):
        return Penalties(**pen_args, context=[(bits, 2 * ns)], gen=gen0.clone(), gen_len=len0.clone(), append=append) if P else None

    pen = penalties(True)

    tok, lp = _Shell().sample_from_logits(logits, 0.0, ns, return_logprobs=True, penalties=pen,
                                          constraint=(dfa, state) if C else None, **cuts)
    only = _Shell().sample_from_logits(logits, 0.0, ns, penalties=penalties(False), constraint=(dfa, state0.clone()) if C else None, **cuts)

    # the definitions, composed directly: penalise (the samples of a leaf row have generated nothing yet), mask, cut, argmax
    x = logits.double()
    if P:
        x = sampling.penalize_logits(logits, **pen_args, context=[(bits, 2)], gen=gen0 if ns == 1 else None, gen_len=len0 if ns == 1 else None)
    x = x.repeat_interleave(ns, 0)
    if C:
        x = sampling.constrain_logits(x, dfa, state0)
    keep = sampling.kept_mask(x, **cuts)
    drawn = keep.any(-1)
    want = torch.where(drawn, x.masked_fill(~keep, -math.inf).argmax(-1), torch.zeros(B, dtype=torch.long))
    want_lp = torch.log_softmax(x, -1).gather(1, want[:, None])[:, 0]
    assert C or bool(drawn.all())

    assert tok.shape == lp.shape == (LEAF, ns) and tok.dtype == torch.int64 and lp.dtype == torch.float32
    assert torch.equal(only, tok)  # without return_logprobs: the tokens alone
    assert torch.equal(tok.reshape(-1), want)
    assert torch.equal(torch.isnan(lp.reshape(-1)), ~drawn)
    # fp32 log-probs of a 65-wide row: a few ulp of values of magnitude < 64
    assert (lp.reshape(-1)[drawn].double() - want_lp[drawn]).abs().max() < 2e-5
    if C:
        nxt = dfa.next.long()
        on = (state0 >= 0) & (state0 < S) & drawn
        want_state = [int(nxt[int(s), int(t)]) if o else int(s) for s, t, o in zip(state0, want, on)]
        assert state.tolist() == want_state and state.dtype == torch.int32
    if P:
        if ns == 1:  # one sample per row and append: the token goes behind the row's list
            want_gen = gen0.clone()
            want_gen[torch.arange(B), len0.long()] = want.int()
            assert torch.equal(pen.gen, want_gen) and torch.equal(pen.gen_len, len0 + 1)
        else:  # the fan-out draw pushes nothing: the decode loop pushes what it feeds
            assert torch.equal(pen.gen, gen0) and torch.equal(pen.gen_len, len0)
