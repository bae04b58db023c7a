"""-m gpu: generate(draft_tokens=) on the paths tests/test_speculative_gpu.py leaves out.  Steps that accept SOME of their drafts (the
next step then overwrites the rejected K/V rows), sampled decoding with drafts (the [B * T, V] sampling route, return_logprobs) and
unique prompts of ragged lengths, whose rows start at different cache indices.  Models, seeds, LOGIT_ERR / GAP and the float64
model are test_speculative_gpu.py's."""
import numpy as np
import pytest
import torch

from hydragen_amd import speculative
from tests.test_speculative_gpu import GAP, LOGIT_ERR, NEW, PROMPT, compared, cpu_model, e2e, ref_logits64, spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOCAB = 512


# ---- 1. partial acceptance, greedy ----------------------------------------------------------------------------------------------
def corrupted(G, K):
    """G with about a third of the positions replaced by a token plain decoding does not emit there (mask drawn on the CPU)"""
    wrong = torch.rand(G.shape, generator=torch.Generator().manual_seed(100 + K)) < 1 / 3
    return torch.where(wrong, (G + 1) % VOCAB, G), wrong


def simulate(G, draft, K, start=None, poll=1):
    """generate()'s draft loop on the host with G as every draw: speculative.accept_reference driven the way
    generation._decode_steps_draft drives hyd_draft_accept -> (steps, proposed [B], accepted [B], the accepted counts of every step of every running row).  A draw
    behind a wrong draft is thrown away whatever it is, so G stands for it as well."""
    B, mx = G.shape
    T = K + 1
    out, length, reason, stop_index, _ = speculative.new_state(B, mx, 0)
    start = torch.zeros(B, dtype=torch.int64) if start is None else start
    accept = lambda fed, smp: speculative.accept_reference(fed, smp, out, length, reason, stop_index, start, None, (), 0, mx, True)  # noqa: E731
    feed, _, _, live = accept(G[:, :1], G[:, :1])
    proposed, accepted, per_step = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), []
    steps, pending = 0, None
    for step in range(1, mx):
        ln = length.long()
        running = ln < mx
        proposed += (mx - 1 - ln).clamp(min=0).clamp(max=K)
        fed = torch.cat([feed[:, None], draft.gather(1, (ln[:, None] + torch.arange(K)[None, :]).clamp(max=mx - 1))], 1)
        smp = G.gather(1, (ln[:, None] + torch.arange(T)[None, :]).clamp(max=mx - 1))
        feed, _, acc, live = accept(fed, smp)
        accepted += acc
        per_step += acc[running].tolist()
        steps += 1
        if pending is not None:
            if pending == 0:
                break
            pending = None
        if steps % poll == 0 and step + 1 < mx:
            pending = live
    assert torch.equal(out, G)
    return steps, proposed, accepted, per_step


def test_the_host_simulation_reproduces_the_closed_counts():
    """perfect drafts: ceil((NEW - 1) / T) steps and every proposal accepted; all wrong: NEW - 1 steps, nothing accepted"""
    G = torch.randint(0, VOCAB, (3, NEW), generator=torch.Generator().manual_seed(0))
    for K in (1, 3, 7):
        steps, prop, acc, _ = simulate(G, G, K)
        assert torch.equal(prop, acc) and bool((prop == NEW - 1 - -(-(NEW - 1) // (K + 1))).all()) and steps == -(-(NEW - 1) // (K + 1)) + 1
        steps, prop, acc, _ = simulate(G, (G + 1) % VOCAB, K)
        assert int(acc.sum()) == 0 and steps == NEW - 1


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_partly_accepted_drafts_return_plain_decoding(heads, kv_heads, K):
    """A step that accepts n of its K drafts leaves K - n rejected K/V rows behind the row's length; the next step starts behind the
    last accepted token and overwrites them.  Tokens equal plain decoding's over each row's compared prefix, and for rows that are not
    cut the statistics equal the host simulation's."""
    model, prompts, G, _, gap = e2e(heads, kv_heads)
    n = compared(gap)
    uncut = n == NEW
    draft, wrong = corrupted(G, K)
    assert 0.2 < float(wrong.float().mean()) < 0.45
    model.stop_poll_steps = 1
    try:
        out, stats = spec(model, prompts, draft_tokens=K, draft=draft.to(DEV))
    finally:
        del model.stop_poll_steps
    out = out.cpu()
    assert out.shape == (6, NEW)
    for b in range(6):
        assert torch.equal(out[b, : n[b]], G[b, : n[b]]), (b, out[b].tolist(), G[b].tolist())
    steps, prop, acc, per_step = simulate(G, draft, K)
    assert torch.equal(stats.accepted.cpu()[uncut], acc[uncut]) and torch.equal(stats.proposed.cpu()[uncut], prop[uncut])
    assert bool((stats.accepted <= stats.proposed).all())
    if bool(uncut.all()):
        assert stats.steps == steps, (stats.steps, steps)
    # the run holds steps that accept none, all, and (K > 1: with one draft there is nothing in between) SOME of their drafts
    assert 0 in per_step and K in per_step and (K == 1 or any(0 < a < K for a in per_step))
    print(f"heads {heads}/{kv_heads} K={K}: steps {stats.steps}, accepted per step {sorted(set(per_step))}, accepted {int(acc.sum())} of {int(prop.sum())}")


def test_partly_accepted_drafts_under_graph_replay():
    model, prompts, G, _, gap = e2e(4, 4)
    n = compared(gap)
    draft, _ = corrupted(G, 3)
    eager, se = spec(model, prompts, draft_tokens=3, draft=draft.to(DEV))
    model.graph(True)
    try:
        graphed, sg = spec(model, prompts, draft_tokens=3, draft=draft.to(DEV))
    finally:
        model.graph(False)
    for b in range(6):
        assert torch.equal(eager[b, : n[b]], graphed[b, : n[b]]) and torch.equal(graphed.cpu()[b, : n[b]], G[b, : n[b]])
    if bool((n == NEW).all()):
        assert torch.equal(se.accepted, sg.accepted) and torch.equal(se.proposed, sg.proposed)
    assert 0 < int(sg.accepted.sum()) < int(sg.proposed.sum())


# ---- 2. sampling with drafts ----------------------------------------------------------------------------------------------------
# The largest |plain decode logits - float64 model| on the SAMPLED token paths of the test below, plain decoding teacher-forced on
# them.  LOGIT_ERR (0.008) was measured on the greedy paths and does not hold here: a sampled path leaves the greedy one at its first
# token and reaches other activations.  Measured (profiles/speculative.md): 0.00469 (4/4 heads) and 0.00957 (8/2) at the
# largest; the larger, rounded up as LOGIT_ERR was.
SAMPLED_LOGIT_ERR = 0.010
def sampled(model, prompts, seed, **kw):
    torch.manual_seed(seed)
    return model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, return_logprobs=True, return_draft_stats=True, **kw)


def forced_plain_logits(model, prompts, tokens):
    """plain (one-token) decoding teacher-forced on `tokens`: the fp32 logits behind every position [B, NEW, V]"""
    _, logits = model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, return_logits=True, token_overrides=tokens)
    return (logits if isinstance(logits, torch.Tensor) else torch.stack(list(logits), 1)).float().cpu()


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("cuts", [{}, {"top_k": 8, "top_p": 0.9}, {"temperature": 0.02}], ids=["uncut", "top_k8_top_p0.9", "cold"])
@pytest.mark.parametrize("draft", ["given", "prompt_lookup"])
def test_sampled_decoding_with_drafts_reports_the_models_logprobs(heads, kv_heads, cuts, draft):
    """Temperature 1: the tokens are random, so what is checked is what they were drawn FROM.  return_logprobs is log softmax(logits)
    of every returned token (unscaled, unfiltered); the float64 model over prompt + returned tokens gives the same quantity exactly.
    Bound: a log-softmax moves by at most twice the largest logit error (the token's logit and the log-sum-exp, one error each).
    That error is plain decoding's on THESE token paths (teacher-forced through token_overrides), asserted within SAMPLED_LOGIT_ERR
    first -- the drafted run does not set its own bound.  B_lp = 2 SAMPLED_LOGIT_ERR.  `cold` (temperature 0.02) draws plain decoding's
    token most of the time, so that given drafts ARE accepted and log-probs of accepted draws are checked as well."""
    model, prompts, G, _, _ = e2e(heads, kv_heads)
    kw = dict(dict(temperature=1.0, draft_tokens=3), **cuts)
    if draft == "given":
        kw["draft"] = G.to(DEV)
    out, lp, stats = sampled(model, prompts, 7, **kw)
    out, lp = out.cpu(), lp.cpu()
    assert out.shape == (6, NEW) and lp.shape == (6, NEW) and out.dtype == torch.int64
    assert bool(((out >= 0) & (out < VOCAB)).all()) and bool((stats.accepted <= stats.proposed).all()) and stats.steps <= NEW - 1
    full = torch.cat([prompts.cpu().repeat_interleave(3, 0), out], 1)
    want = ref_logits64(model, full)[:, PROMPT - 1 : PROMPT - 1 + NEW]
    plain_err = float((forced_plain_logits(model, prompts, out.to(DEV)).double() - want).abs().max())
    want_lp = torch.log_softmax(want, -1).gather(2, out[..., None])[..., 0]
    lp_err = float((lp.double() - want_lp).abs().max())
    print(f"heads {heads}/{kv_heads} {draft} {cuts}: plain logit error on the sampled paths {plain_err:.5f}, drafted log-prob error {lp_err:.5f} "
          f"(bound {2 * SAMPLED_LOGIT_ERR}), accepted {int(stats.accepted.sum())} of {int(stats.proposed.sum())} in {stats.steps} steps")
    assert plain_err <= SAMPLED_LOGIT_ERR
    assert lp_err <= 2 * SAMPLED_LOGIT_ERR
    assert bool((lp <= 0).all())
    if "top_k" in cuts:  # every returned token lies among the 8 most probable of its step (to the logit error: a tie at the cut may fall either way)
        kth = want.topk(8, -1).values[..., -1]
        assert bool((want.gather(2, out[..., None])[..., 0] >= kth - GAP).all())
    # the same seed, the same call: the same tokens, log-probs and statistics
    out2, lp2, stats2 = sampled(model, prompts, 7, **kw)
    assert torch.equal(out2.cpu(), out) and torch.equal(lp2.cpu(), lp)
    assert stats2.steps == stats.steps and torch.equal(stats2.accepted, stats.accepted) and torch.equal(stats2.proposed, stats.proposed)
    if "temperature" not in cuts:  # (and at temperature 1 another seed draws other tokens: the draw is random)
        out3, _, _ = sampled(model, prompts, 8, **kw)
        assert not torch.equal(out3.cpu(), out)


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
def test_top_k_1_at_temperature_1_with_drafts_is_greedy(heads, kv_heads):
    model, prompts, G, _, gap = e2e(heads, kv_heads)
    n = compared(gap)
    for draft in (G.to(DEV), "prompt_lookup"):
        out, lp, stats = sampled(model, prompts, 3, temperature=1.0, top_k=1, draft_tokens=3, draft=draft)
        for b in range(6):
            assert torch.equal(out.cpu()[b, : n[b]], G[b, : n[b]]), (b, out[b].tolist(), G[b].tolist())
        assert bool((stats.accepted <= stats.proposed).all())
    # (the given drafts are plain decoding's tokens: where no row is cut, every one is accepted)


# ---- 3. ragged starts -------------------------------------------------------------------------------------------------------------
# One shared level (two sequences of 24 tokens, three rows each) and per-row unique prompts of ragged lengths: the rows' first decode
# steps write at cache indices 3 .. 33, and the drafted steps cross 16 and 32 at different steps in different rows.
SHARED, WIDTH, RAGGED_NEW = 24, 33, 12
RAGGED_LENS = [3, 14, 16, 17, 31, 33]
# Head geometries: 4/4 and 4/2 (grouped-query, g = 2), hidden size 256.  The 8/2 model (hidden 512) of the other tests is not used
# here: its plain decoding reads 0.0081 .. 0.0096 from the float64 model on these ragged inputs (8 seeds measured,
# profiles/speculative.md) -- LOGIT_ERR = 0.008 is its figure on SEEDS' inputs, 0.00795, rounded up, and has no room for other inputs.
# Seed of the weights and the prompts per head geometry, searched on the CPU with the float64 model as SEEDS was (seeds 0 .. 799 for 4/4,
# 0 .. 2399 for 4/2).  Six DIFFERENT rows
# make 6 x RAGGED_NEW greedy decisions (SEEDS' prompts make 2 x 24), and over 6 x 24 no seed in 1200 keeps them apart; over 6 x 12 these
# do.  Smallest top-2 gap of the float64 model's greedy decode per row, the two smallest rows: RAGGED_GAPS -- at most the one row
# below 2 GAP can be cut by plain decoding's own error (tests/test_speculative.py repeats that check without a GPU).
RAGGED_GEOMETRIES = [(4, 4), (4, 2)]
RAGGED_SEEDS = {(4, 4): 241, (4, 2): 2018}
RAGGED_GAPS = {(4, 4): (0.0225, 0.0527), (4, 2): (0.0222, 0.0356)}


def ragged_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, VOCAB, (2, SHARED), generator=g), torch.randint(1, VOCAB, (6, WIDTH), generator=g)


_RAGGED = {}


def ragged(heads, kv_heads):
    """The model, the inputs, plain decoding's tokens G and logits of the ragged inputs, once per head geometry."""
    if (heads, kv_heads) not in _RAGGED:
        from tests.test_model_gpu import make_model

        seed = RAGGED_SEEDS[(heads, kv_heads)]
        model = make_model(torch.float16, head_dim=64, kv_heads=kv_heads, layers=2, heads=heads)
        with torch.no_grad():
            for p, c in zip(model.parameters(), cpu_model(heads, kv_heads, seed).parameters()):
                p.copy_(c)
        model.setup_caches(max_unique_batch_size=6, max_unique_seq_length=WIDTH + RAGGED_NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[SHARED])
        shared, uniq = ragged_inputs(seed)
        kw = dict(input_ids=[shared.to(DEV), uniq.to(DEV)], seq_lens=[torch.tensor([SHARED, SHARED], device=DEV), torch.tensor(RAGGED_LENS, device=DEV)],
                  num_return_sequences=1, max_new_tokens=RAGGED_NEW, temperature=0)
        G, logits = model.generate(return_logits=True, **kw)
        logits = (logits if isinstance(logits, torch.Tensor) else torch.stack(list(logits), 1)).float().cpu()
        top2 = logits.topk(2, -1).values
        _RAGGED[(heads, kv_heads)] = (model, kw, shared, uniq, G.cpu(), logits, top2[..., 0] - top2[..., 1])
    return _RAGGED[(heads, kv_heads)]


@pytest.mark.parametrize("heads, kv_heads", RAGGED_GEOMETRIES)
def test_ragged_plain_decode_stays_within_the_measured_logit_error(heads, kv_heads):
    """The condition of the comparison below, as test_plain_decode_stays_within_the_measured_logit_error states it."""
    model, kw, shared, uniq, G, logits, gap = ragged(heads, kv_heads)
    err = 0.0
    for b, ln in enumerate(RAGGED_LENS):
        full = torch.cat([shared[b // 3], uniq[b, :ln], G[b]])[None]
        want = ref_logits64(model, full)[0, SHARED + ln - 1 : SHARED + ln - 1 + RAGGED_NEW]
        err = max(err, float((logits[b].double() - want).abs().max()))
    n = compared(gap)
    print(f"ragged, heads {heads}/{kv_heads}: max |plain decode logits - float64 model| = {err:.4f}, smallest top-2 gap {float(gap.min()):.4f}, compared {n.tolist()}")
    assert err <= LOGIT_ERR
    assert int((n < RAGGED_NEW).sum()) <= 1


@pytest.mark.parametrize("heads, kv_heads", RAGGED_GEOMETRIES)
def test_ragged_starts_with_drafts_return_plain_decoding(heads, kv_heads):
    model, kw, shared, uniq, G, _, gap = ragged(heads, kv_heads)
    n = compared(gap)
    uncut = n == RAGGED_NEW
    K = 3
    draft, _ = corrupted(G, K)
    model.stop_poll_steps = 1
    try:
        runs = {"perfect": model.generate(draft_tokens=K, draft=G.to(DEV), return_draft_stats=True, **kw),
                "corrupted": model.generate(draft_tokens=K, draft=draft.to(DEV), return_draft_stats=True, **kw),
                "prompt lookup": model.generate(draft_tokens=K, return_draft_stats=True, **kw)}
    finally:
        del model.stop_poll_steps
    for name, (out, stats) in runs.items():
        out = out.cpu()
        assert out.shape == (6, RAGGED_NEW), name
        for b in range(6):
            assert torch.equal(out[b, : n[b]], G[b, : n[b]]), (name, b, out[b].tolist(), G[b].tolist())
        assert bool((stats.accepted <= stats.proposed).all()) and stats.steps <= RAGGED_NEW - 1, name
    for name, d in (("perfect", G), ("corrupted", draft)):
        steps, prop, acc, per_step = simulate(G, d, K)
        s = runs[name][1]
        assert torch.equal(s.accepted.cpu()[uncut], acc[uncut]) and torch.equal(s.proposed.cpu()[uncut], prop[uncut]), name
        assert not bool(uncut.all()) or s.steps == steps, name
    assert any(0 < a < K for a in per_step)
