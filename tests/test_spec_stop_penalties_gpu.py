"""-m gpu: hyd_draft_accept_stop against speculative.accept_stop_reference and against one-token hyd_stop_update launches (exactly,
over the generations of tests/spec_stop_cases.py), hyd_sample_tokens_penalized_drafts against hyd_sample_tokens_penalized on the
expanded lists (bit for bit), and generate(draft_tokens=) with stop sequences, penalties and logit bias against plain decoding."""
import pytest
import torch

from hydragen_amd import layer_ops, sampling, speculative, stopping
from tests import spec_stop_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_REF = {}


def reference(K, name, include_stop):
    """(steps, the reference's records) of one generation, computed once and shared by the tests that need it."""
    key = (K, name, include_stop)
    if key not in _REF:
        vocab, max_new = cases.RANGES[name]
        steps = cases.step_inputs(K, vocab, max_new, seed=100 * K + ord(name))
        _REF[key] = (steps, cases.run(cases.reference_accept(cases.spec(include_stop), max_new), steps, max_new))
    return _REF[key]


def device_accept(spec, max_new, stop_tokens):
    def accept(fed, sampled, lp, after, st):
        live = torch.zeros((1,), dtype=torch.int32, device=DEV)
        feed, pos, acc = speculative.draft_accept(fed, sampled, st.out, st.length, st.reason, st.stop_index, live, st.start_pos, st.shared_len,
                                                  spec.eos, spec.pad, max_new, True, lp, st.out_lp, states=(after, st.state), stop=spec,
                                                  gen=st.gen, gen_len=st.gen_len, stop_tokens=stop_tokens)
        return feed, pos, acc, int(live)
    return accept


# ---- hyd_draft_accept_stop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_stop", [False, True])
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_draft_accept_stop_equals_the_definition_after_every_step(K, name, include_stop):
    spec = cases.spec(include_stop)
    max_new = cases.RANGES[name][1]
    steps, ref = reference(K, name, include_stop)
    got = cases.run(device_accept(spec, max_new, spec.stop_table(DEV)[0]), steps, max_new, DEV)
    for s, (a, b) in enumerate(zip(got, ref)):
        for key in b:  # out, length, reason, stop_index, out_lp, gen, gen_len, state; feed, next_pos, accepted, live
            same = a[key] == b[key] if key == "live" else torch.equal(a[key], b[key])
            assert same, (key, "step", s)
    assert ref[-1]["live"] == 0 and {1, 2} <= set(ref[-1]["reason"].tolist())


@pytest.mark.parametrize("include_stop", [False, True])
@pytest.mark.parametrize("name", ["a", "b"])
def test_the_same_generations_through_one_token_hyd_stop_update_launches(name, include_stop):
    """The accepted draws of the reference's run, row by row in order, launched one column at a time through the EXISTING
    hyd_stop_update: the same output matrix, lengths, finish reasons and stop indices as the speculative accept's."""
    K = 3
    spec = cases.spec(include_stop)
    max_new = cases.RANGES[name][1]
    steps, ref = reference(K, name, include_stop)
    spec_dev = cases.run(device_accept(spec, max_new, None), steps, max_new, DEV)[-1]
    stream = torch.full((cases.ROWS, max_new), spec.pad, dtype=torch.int64)
    filled = [0] * cases.ROWS
    before = cases.new_state(cases.ROWS, max_new).snapshot()
    for rec, (_, sampled, _, _) in zip(ref, steps):
        for b in range(cases.ROWS):
            if int(before["reason"][b]) == 0 and int(before["length"][b]) < max_new:
                e = int(rec["accepted"][b]) + 1
                stream[b, filled[b]: filled[b] + e] = sampled[b, :e]
                filled[b] += e
        before = rec
    out, length, reason, index, live = stopping.new_state(cases.ROWS, max_new, spec, DEV)
    table = spec.stop_table(DEV)[0]
    start = torch.zeros((cases.ROWS,), dtype=torch.int64, device=DEV)
    stream = stream.to(DEV)
    for t in range(max_new):
        layer_ops.stop_update(stream[:, t].contiguous(), t, spec, out, length, reason, index, live, start, None, False, table)
    for key, x in (("out", out), ("length", length), ("reason", reason), ("stop_index", index)):
        assert torch.equal(x.cpu(), ref[-1][key]) and torch.equal(x.cpu(), spec_dev[key]), key


@pytest.mark.parametrize("with_states", [False, True])
def test_without_stops_and_lists_the_call_is_the_existing_accept_byte_for_byte(with_states):
    """stop with no sequence and gen = NULL through hyd_draft_accept_stop against hyd_draft_accept / hyd_draft_accept_states on the
    same inputs: every buffer after every step."""
    K, (vocab, max_new) = 3, cases.RANGES["a"]
    steps = cases.step_inputs(K, vocab, max_new, seed=7)
    none = stopping.StopSpec(eos=cases.EOS, stops=(), pad=cases.PAD)

    def accept(stop):
        def call(fed, sampled, lp, after, st):
            live = torch.zeros((1,), dtype=torch.int32, device=DEV)
            feed, pos, acc = speculative.draft_accept(fed, sampled, st.out, st.length, st.reason, st.stop_index, live, st.start_pos, st.shared_len,
                                                      cases.EOS, cases.PAD, max_new, True, lp, st.out_lp,
                                                      states=(after, st.state) if with_states else None, stop=stop)
            return feed, pos, acc, int(live)
        return call

    new, old = cases.run(accept(none), steps, max_new, DEV), cases.run(accept(None), steps, max_new, DEV)
    for a, b in zip(new, old):
        for key in b:
            assert a[key] == b[key] if key == "live" else torch.equal(a[key], b[key]), key
    assert int((old[-1]["reason"] == 1).sum()) > 0


# ---- hyd_sample_tokens_penalized_drafts -----------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# one vocabulary on each side of the LDS-bitmap threshold (kCtxWords * 32 = 262144 tokens), neither a multiple of 8
@pytest.mark.parametrize("n", [31997, 300001])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("T", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_penalized_drafts_equal_the_existing_sampler_on_the_expanded_lists(B, T, dtype, n):
    from tests.penalty_cases import DT

    g = torch.Generator().manual_seed(1000 * B + 10 * T + n % 7)
    rows, stride = B * T, 16
    logits = (torch.randn(rows, n, generator=g) * 3.0).to(DT[dtype])
    top = torch.topk(logits.float(), 8, dim=-1).indices  # the tokens whose penalties decide a row
    # per sequence: a list that is empty / full / partly filled, drawn from the top tokens of the sequence's rows (so that it
    # overlaps with the context, the bias ids and the drafts), with an id outside [0, n)
    gen = top[::T].repeat(1, 2)[:, :stride].to(torch.int32).contiguous()
    gen[:, 3] = -1
    gen_len = torch.tensor([5, 0, stride][:B] if B > 1 else [stride + 9], dtype=torch.int32)  # (B = 1: beyond the stride, clamped)
    fed = torch.randint(0, n, (B, T), generator=g)
    for i in range(1, T):
        fed[:, i] = top[torch.arange(B) * T + i, (i // 2) % 8]  # drafts from the top of the row they precede ...
    if T >= 3:
        fed[:, 2] = fed[:, 1]  # ... one of them twice ...
    if T == 8:
        fed[0, 4], fed[-1, 5] = -3, n + 5  # ... and ids outside [0, n)
    shared = sampling.token_bitmap_reference(torch.cat([top[0, :3], torch.randint(0, n, (40,), generator=g)])[None], None, n)
    own = sampling.token_bitmap_reference(torch.cat([top[::T, 1:3], torch.randint(0, n, (B, 20), generator=g)], 1), None, n)
    bias = (torch.cat([top[0, :2], fed[0, 1:2].clamp(0, n - 1), torch.tensor([n - 1])]).unique().to(DEV), None)
    bias = (bias[0], torch.linspace(-2.0, 2.0, bias[0].numel()).to(DEV))
    lists, lens = sampling.draft_row_lists_reference(gen, gen_len, fed)
    assert int(lens.max()) <= lists.shape[1] and bool(((lists >= -(2 ** 31)) & (lists < 2 ** 31)).all())

    def pen(context, gen_, len_):
        return layer_ops.Penalties(1.3, 0.6, 0.4, bias, [(b.to(DEV), k) for b, k in context], gen=gen_.to(DEV).contiguous(), gen_len=len_.to(DEV))

    per_seq = pen([(shared, B), (own, 1)], gen, gen_len)                       # one context row shared by the B sequences: a group
    per_row = pen([(shared, B * T), (own, T)], lists.to(torch.int32), lens)    # the definition: explicit lists, rows_per_group * T
    x, f = logits.to(DEV), fed.to(DEV)
    for temperature, top_p in ((0.0, None), (1.0, 0.9)):
        key = (1234, 8 * T)
        want = layer_ops.sample_tokens_penalized(x, temperature, key, penalties=per_row, top_p=top_p)
        got = layer_ops.sample_tokens_penalized(x, temperature, key, penalties=per_seq, top_p=top_p, drafts=f)
        for a, b, what in zip(got, want, ("tokens", "logprobs", "kept")):
            assert bits_equal(a, b), (what, temperature, a.tolist(), b.tolist())
        if T == 1:  # ... and T = 1 is the plain call
            plain = layer_ops.sample_tokens_penalized(x, temperature, key, penalties=per_seq, top_p=top_p)
            assert all(bits_equal(a, b) for a, b in zip(got, plain))
    # the drafts matter on these rows: they are top tokens of the rows they precede, so leaving them out of the lists changes the
    # penalised distribution of a T > 1 step (its log-probs; the drawn token only where the top-2 gap is small enough)
    if T > 1:
        blind = layer_ops.sample_tokens_penalized(x, 0.0, (1234, 8 * T), penalties=pen([(shared, B * T), (own, T)], gen.repeat_interleave(T, 0),
                                                                                     gen_len.repeat_interleave(T, 0)))
        want = layer_ops.sample_tokens_penalized(x, 0.0, (1234, 8 * T), penalties=per_row)
        assert not bits_equal(blind[1], want[1])


# ---- generate() ----------------------------------------------------------------------------------------------------------------------
def _e2e(heads, kv_heads):
    from tests.test_speculative_gpu import e2e

    return e2e(heads, kv_heads)


def _stop_check(model, prompts, G, n, stops, eos, **kw):
    """generate(draft_tokens=, stop=) against stopping.truncate_reference of plain decoding G, on the rows whose every decision up
    to the stop lies in front of the first top-2 gap below GAP (test_speculative_gpu.compared)."""
    from tests.test_speculative_gpu import NEW

    for include in (False, True):
        sp = stopping.check_stop(eos, stops, 7, include, 512)
        w_out, w_len, w_reason, w_index = stopping.truncate_reference(G, sp)
        step = stopping.finish_steps(G, sp)[0]  # the column that ends a row (NEW: none)
        ok = (n == NEW) | (step < n)
        assert int(ok.sum()) >= 4 and int((w_reason[ok] == 2).sum()) >= 2
        out, fin, stats = model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, eos_token_id=eos, stop=stops,
                                         pad_token_id=7, include_stop=include, return_finish=True, return_draft_stats=True, **kw)
        out = out.cpu()
        for b in torch.nonzero(ok).flatten().tolist():
            ln = int(w_len[b])
            assert int(fin.lengths[b]) == ln and int(fin.reasons[b]) == int(w_reason[b]) and int(fin.stop_index[b]) == int(w_index[b]), (b, include)
            assert torch.equal(out[b, :ln], w_out[b, :ln]) and bool((out[b, ln:] == 7).all()), (b, include)
    return stats


def _stops_from(G):
    """Stop sequences cut out of plain decoding's own output: a long one that spans steps, a pair, and a single token of another
    row; plus one that never occurs."""
    return [G[0, 9:14].tolist(), G[3, 6:8].tolist(), [int(G[4, 15])], [511, 510, 509]]


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("K", [3, 7])
def test_generate_with_drafts_and_stops_returns_plain_decoding_cut_by_the_definition(heads, kv_heads, K):
    from tests.test_speculative_gpu import compared

    model, prompts, G, _, gap = _e2e(heads, kv_heads)
    n = compared(gap)
    stops = _stops_from(G)
    for name, kw in (("perfect", dict(draft=G.to(DEV))), ("all wrong", dict(draft=((G + 1) % 512).to(DEV))), ("prompt lookup", {})):
        stats = _stop_check(model, prompts, G, n, stops, None, draft_tokens=K, **kw)
        assert bool((stats.accepted <= stats.proposed).all()), name
    assert int(_stop_check(model, prompts, G, n, stops, [int(G[1, 20])], draft_tokens=K, draft=G.to(DEV)).accepted.sum()) > 0


def test_generate_with_drafts_and_stops_under_graph_decode():
    from tests.test_speculative_gpu import compared

    model, prompts, G, _, gap = _e2e(4, 4)
    model.graph(True)
    try:
        stats = _stop_check(model, prompts, G, compared(gap), _stops_from(G), None, draft_tokens=3, draft=G.to(DEV))
    finally:
        model.graph(False)
    assert int(stats.accepted.sum()) > 0


def test_generate_with_drafts_and_stops_on_an_fp8_unique_cache():
    """The fp8 cache changes the logits, so the comparison is with plain decoding ON THAT CACHE, on the rows where both runs stop
    in front of its first narrow decision."""
    from hydragen_amd.kv_quant import FP8_DTYPE
    from tests.test_model_gpu import make_model
    from tests.test_speculative_gpu import GAP, NEW, PROMPT, SEEDS, cpu_model, cpu_prompts

    seed = SEEDS[(8, 2)]
    model = make_model(torch.float16, head_dim=64, kv_heads=2, layers=2, heads=8)
    with torch.no_grad():
        for p, c in zip(model.parameters(), cpu_model(8, 2, seed).parameters()):
            p.copy_(c)
    model.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[PROMPT],
                       kv_cache_dtype=FP8_DTYPE)
    prompts = cpu_prompts(seed).to(DEV)
    G, logits = model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, return_logits=True)
    logits = torch.stack(list(logits), 1) if not isinstance(logits, torch.Tensor) else logits
    top2 = logits.float().topk(2, -1).values
    below = ((top2[..., 0] - top2[..., 1]) < GAP).cpu()
    n = torch.where(below.any(1), below.int().argmax(1), torch.full((6,), NEW))
    G = G.cpu()
    b = int(n.argmax())  # stop sequences from the rows that are compared longest
    stops = [G[b, 4:7].tolist(), G[(b + 3) % 6, 2:4].tolist(), [int(G[b, 1])], [511, 510, 509]]
    sp = stopping.check_stop(None, stops, 7, False, 512)
    step = stopping.finish_steps(G, sp)[0]
    ok = (n == NEW) | (step < n)
    assert int(ok.sum()) >= 2
    w_out, w_len, w_reason, _ = stopping.truncate_reference(G, sp)
    out, fin = model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, stop=stops, pad_token_id=7,
                              return_finish=True, draft_tokens=3, draft=G.to(DEV))
    for r in torch.nonzero(ok).flatten().tolist():
        ln = int(w_len[r])
        assert int(fin.lengths[r]) == ln and int(fin.reasons[r]) == int(w_reason[r]) and torch.equal(out.cpu()[r, :ln], w_out[r, :ln]), r


def test_penalties_count_the_fed_drafts():
    """presence_penalty 1e4, logit_bias {c1: +200, c2: +100}, temperature 0, drafts [c1, c2, c2, c2, ...]: the first token is c1, the
    second c2 (an accepted draft), and behind the FED c2 the draw must already count it -- a sampler that counts emitted tokens
    only draws c2 again there, the accept takes it, and the row repeats c2.  No logit of these models comes near 100."""
    model, prompts, _, _, _ = _e2e(4, 4)
    c1, c2, new = 17, 401, 12
    draft = torch.full((6, new), c2, dtype=torch.int64, device=DEV)
    draft[:, 0] = c1
    out, stats = model.generate([prompts], num_return_sequences=3, max_new_tokens=new, temperature=0, presence_penalty=1e4,
                                logit_bias={c1: 200.0, c2: 100.0}, draft_tokens=3, draft=draft, return_draft_stats=True)
    assert out.shape == (6, new)
    for row in out.tolist():
        assert row[:2] == [c1, c2] and len(set(row)) == new, row
    assert bool((stats.accepted >= 1).all())


def test_penalised_drafts_return_plain_penalised_decoding():
    """repetition_penalty 1.3 with frequency_penalty 0.5, greedy, drafts = the plain penalised run's own output: equal tokens up to
    a row's first position whose top-2 gap of the PENALISED logits (the plain run's returned logits through
    sampling.penalize_logits, float64) is below GAP."""
    from tests.test_speculative_gpu import GAP, NEW

    model, prompts, _, _, _ = _e2e(8, 2)
    kw = dict(num_return_sequences=3, max_new_tokens=NEW, temperature=0, repetition_penalty=1.3, frequency_penalty=0.5)
    P, logits = model.generate([prompts], return_logits=True, **kw)
    logits = torch.stack(list(logits), 1) if not isinstance(logits, torch.Tensor) else logits
    P, logits = P.cpu(), logits.float().cpu()
    ctx = [(sampling.token_bitmap_reference(prompts.cpu(), None, 512), 3)]
    gap = torch.empty((6, NEW), dtype=torch.float64)
    for t in range(NEW):
        x = sampling.penalize_logits(logits[:, t], 1.3, None, 0.5, None, ctx, P[:, :t] if t else None, torch.full((6,), t) if t else None)
        top2 = x.topk(2, -1).values
        gap[:, t] = top2[:, 0] - top2[:, 1]
        assert torch.equal(x.argmax(-1)[gap[:, t] > GAP], P[:, t][gap[:, t] > GAP])  # (the plain run is what its logits say)
    below = gap < GAP
    n = torch.where(below.any(1), below.int().argmax(1), torch.full((6,), NEW))
    print("compared positions per row:", n.tolist())
    assert int(n.sum()) >= NEW, n.tolist()
    for K in (3, 7):
        out, stats = model.generate([prompts], draft_tokens=K, draft=P.to(DEV), return_draft_stats=True, **kw)
        for b in range(6):
            assert torch.equal(out.cpu()[b, : n[b]], P[b, : n[b]]), (K, b, out[b].tolist(), P[b].tolist())
        assert int(stats.accepted.sum()) > 0


def test_what_a_speculative_step_still_refuses_is_named():
    from hydragen_amd.constraint import TokenDFA

    model, prompts, G, _, _ = _e2e(4, 4)
    kw = dict(num_return_sequences=3, max_new_tokens=8, draft_tokens=3)
    dfa = TokenDFA.from_choices([[1, 2, 3]], 512, eos=[511]).to(DEV)
    for more, words in ((dict(constraint=dfa, presence_penalty=0.5), "penalties"), (dict(constraint=dfa, logit_bias={3: 1.0}), "constraint"),
                        (dict(constraint=dfa, draft="constraint", stop=[[1, 2]]), "stop together with constraint"),
                        (dict(return_logprobs=True, top_logprobs=2), "top_logprobs"), (dict(return_logits=True), "return_logits"),
                        (dict(token_overrides=G[:, :8].to(DEV)), "token_overrides"), (dict(temperature=[0.5] * 5 + [1.0]), "per-row"),
                        (dict(seed=[1, 2, 3, 4, 5, 6]), "per-row"), (dict(max_new_tokens=[8, 8, 8, 8, 8, 4]), "per-row")):
        with pytest.raises(NotImplementedError, match=words):
            model.generate([prompts], **dict(kw, **more))
