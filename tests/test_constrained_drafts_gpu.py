"""-m gpu: speculative decoding under a token automaton on the MI355X.  hyd_dfa_forced_tokens, hyd_draft_constrain and
hyd_draft_accept_states against their definitions (exactly), and generate(constraint=, draft_tokens=) against
generate(constraint=)."""
import ctypes as C

import pytest
import torch

from hydragen_amd import _lib, sampling, speculative
from hydragen_amd.constraint import TokenDFA, forced_tokens, forced_tokens_reference
from tests.test_constrained_drafts import bitmap, forced_steps, hand_rows, random_dfa
from tests.test_speculative_gpu import GAP, NEW, PROMPT, cpu_model, cpu_prompts, ref_logits64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- hyd_dfa_forced_tokens -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 1000, 32005])
def test_forced_tokens_equal_the_definition(n):
    """S = 37: the hand-written row kinds, then random rows of 0 .. 3 bits.  Two row strides: ceil(n / 32), and the next multiple
    of 4 words above it with the padding words full of bits -- between them the 16-byte and the 4-byte loads both run."""
    S, words = 37, (n + 31) // 32
    rows, _ = hand_rows(n)
    g = torch.Generator().manual_seed(n)
    while len(rows) < S:
        rows.append(torch.randint(0, n, (int(torch.randint(0, 4, (1,), generator=g)),), generator=g).tolist())
    tight = bitmap(rows, n)
    want = forced_tokens_reference(tight, n)
    assert int((want >= 0).sum()) >= 8 and int((want < 0).sum()) >= 8
    wide = torch.full((S, (words // 4 + 1) * 4), -1, dtype=torch.int32)
    wide[:, :words] = tight
    for allowed in (tight, wide):
        got = forced_tokens(allowed.to(DEV), n)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (n, allowed.shape)
    view = wide.to(DEV)[:, :words]  # the same rows as a view: the stride is the parent's
    assert view.stride(0) > words and torch.equal(forced_tokens(view, n).cpu(), want)


def test_token_dfa_makes_forced_on_its_device():
    dfa = random_dfa(3)
    on = dfa.to(DEV)
    assert on.forced.device.type == "cuda" and torch.equal(on.forced.cpu(), dfa.forced) and on.forced is on.forced
    assert torch.equal(dfa.to(DEV).forced.cpu(), dfa.forced)  # (made on the CPU first: copied with the automaton)


# ---- hyd_draft_constrain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("B", [6, 130])
def test_draft_constrain_equals_the_definition(B, K):
    S, n, T = 8, 50, K + 1
    for seed, only, counted in ((0, False, True), (1, True, True), (2, False, False), (3, True, False)):
        dfa = random_dfa(10 * K + seed)
        on = dfa.to(DEV)
        g = torch.Generator().manual_seed(100 * B + 10 * K + seed)
        state = torch.randint(0, S, (B,), generator=g).to(torch.int32)
        state[:3] = torch.tensor([-1, -2, S + 3], dtype=torch.int32)
        wide = torch.randint(-2, n + 2, (B, T + 3), generator=g)  # fed is columns 0 .. T - 1 of a wider buffer
        # half of the drafts are ones the automaton takes, so that chains run on behind the first draft
        for b in range(B):
            s = int(state[b])
            for j in range(K):
                ok = (dfa.next[s] != sampling.DFA_REJECT).nonzero()[:, 0] if 0 <= s < S else torch.arange(n)
                if float(torch.rand((), generator=g)) < 0.7:
                    wide[b, j + 1] = ok[int(torch.randint(0, len(ok), (1,), generator=g))]
                t = int(wide[b, j + 1])
                s = int(dfa.next[s, t]) if 0 <= s < S and 0 <= t < n else s
        n_prop = torch.randint(0, K + 1, (B,), generator=g).to(torch.int32) if counted else None
        want_fed, want_np = wide.clone(), None if n_prop is None else n_prop.clone()
        want_ss, want_nf = speculative.constrain_drafts_reference(dfa, state, want_fed[:, :T], want_np, only)
        dev_wide, dev_np = wide.to(DEV), None if n_prop is None else n_prop.to(DEV)
        ss, nf = speculative.constrain_drafts(on, state.to(DEV), dev_wide[:, :T], dev_np, only)
        torch.cuda.synchronize()
        what = (B, K, seed, only, counted)
        assert torch.equal(ss.cpu(), want_ss) and torch.equal(nf.cpu(), want_nf), what
        assert torch.equal(dev_wide.cpu(), want_fed), what  # the drafts as rewritten, and nothing else of the buffer
        assert n_prop is None or torch.equal(dev_np.cpu(), want_np), what
        if B > 64 and not only:
            assert int(want_nf.sum()) > 0 and int((want_ss == -1).sum()) > 0 and int((want_ss == -2).sum()) >= K + 1


def constrain_params(**kw):
    B, K, S, n = 4, 3, 8, 50
    keep = dict(state=torch.zeros(B, dtype=torch.int32, device=DEV), fed=torch.zeros((B, K + 1), dtype=torch.int64, device=DEV),
                n_proposed=torch.zeros(B, dtype=torch.int32, device=DEV), forced=torch.full((S,), -1, dtype=torch.int32, device=DEV),
                next=torch.zeros((S, n), dtype=torch.int32, device=DEV), step_state=torch.zeros((B, K + 1), dtype=torch.int32, device=DEV),
                n_forced=torch.zeros(B, dtype=torch.int32, device=DEV))
    p = _lib.DraftConstrainParams()
    for name, t in keep.items():
        setattr(p, name, t.data_ptr())
    p.fed_stride, p.next_stride, p.B, p.K, p.n_states, p.n = K + 1, n, B, K, S, n
    for name, v in kw.items():
        setattr(p, name, v(getattr(p, name)) if callable(v) else v)
    return p, keep


@pytest.mark.parametrize("kw", [dict(state=None), dict(fed=None), dict(forced=None), dict(next=None), dict(step_state=None), dict(n_forced=None),
                                dict(B=-1), dict(K=0), dict(K=8), dict(n_states=0), dict(n_states=-3), dict(next_stride=49), dict(n=0),
                                dict(fed_stride=3), dict(fed=lambda a: a + 4), dict(step_state=lambda a: a + 2)])
def test_draft_constrain_refuses_bad_arguments(kw):
    lib = _lib.load()
    p, keep = constrain_params(**kw)  # (the addresses are those of live buffers, or inside them: nothing is made up)
    assert lib.hyd_draft_constrain(C.byref(p), None) == -1, lib.hyd_last_error_string().decode()
    ok, keep = constrain_params(B=0)
    assert lib.hyd_draft_constrain(C.byref(ok), None) == 0  # nothing to do: no launch
    ok, keep = constrain_params(n_proposed=None)
    assert lib.hyd_draft_constrain(C.byref(ok), torch.cuda.current_stream().cuda_stream) == 0  # n_proposed may be NULL
    torch.cuda.synchronize()
    f = _lib.DfaForcedParams()
    assert lib.hyd_dfa_forced_tokens(C.byref(f), None) == -1


# ---- hyd_draft_accept_states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("rows", [6, 130])
def test_draft_accept_states_equals_the_definition_over_a_generation(K, rows, monkeypatch):
    """The generation-long simulation of test_draft_accept_equals_the_definition_over_a_generation with the rows' automaton states
    carried: the device state, the hand-backs AND the states equal accept_states_reference's after every step; and through
    hyd_draft_accept_states with both pointers NULL every buffer is hyd_draft_accept's, byte for byte."""
    g = torch.Generator().manual_seed(10 * K + rows)
    T, mx, pad, eos = K + 1, 19, 15, (3, 11)
    start = torch.arange(rows) * 5 + 40
    shared = torch.arange(rows) % 4 + 30
    lib = _lib.load()
    plain_entry = lib.hyd_draft_accept
    for retire, with_lp in ((True, True), (False, False)):
        cpu = speculative.new_state(rows, mx, pad, None, with_lp)
        dev = speculative.new_state(rows, mx, pad, DEV, with_lp)
        nul = speculative.new_state(rows, mx, pad, DEV, with_lp)    # hyd_draft_accept_states(p, NULL, NULL)
        old = speculative.new_state(rows, mx, pad, DEV, with_lp)    # hyd_draft_accept(p)
        live = torch.zeros((3, mx), dtype=torch.int32, device=DEV)
        st_cpu = torch.arange(rows, dtype=torch.int32) + 1000
        st_dev = st_cpu.to(DEV)
        for step in range(mx):
            t = 1 if step == 0 else T
            sampled = torch.randint(0, 14, (rows, t), generator=g)
            sampled[torch.rand(rows, t, generator=g) < 0.03] = 11
            fed = torch.randint(0, 14, (rows, t), generator=g)
            agree = torch.rand(rows, t, generator=g) < 0.66
            fed[:, 1:] = torch.where(agree[:, 1:], sampled[:, :-1], fed[:, 1:])
            lp = -torch.rand(rows, t, generator=g) if with_lp else None
            after = torch.randint(-2, 50, (rows, t), generator=g).to(torch.int32)
            want = speculative.accept_states_reference(fed, sampled, after, st_cpu, *cpu[:4], start, shared, eos, pad, mx, retire, lp, cpu[4])
            args = lambda s, k: (fed.to(DEV), sampled.to(DEV), *s[:4], live[k, step : step + 1], start.to(DEV), shared.to(DEV), eos, pad, mx,  # noqa: E731
                                 retire, None if lp is None else lp.to(DEV), s[4])
            got = speculative.draft_accept(*args(dev, 0), states=(after.to(DEV), st_dev))
            ref = speculative.draft_accept(*args(old, 1))
            with monkeypatch.context() as m:
                m.setattr(lib, "hyd_draft_accept", lambda p, s: lib.hyd_draft_accept_states(p, None, None, s))
                same = speculative.draft_accept(*args(nul, 2))
            assert lib.hyd_draft_accept is plain_entry
            for a, b, c, d, name in zip(got, want[:3], same, ref, ("feed", "next_pos", "accepted")):
                assert torch.equal(a.cpu(), b) and torch.equal(c, d) and torch.equal(c, a), (name, step)
            assert int(live[0, step]) == want[3] == int(live[1, step]) == int(live[2, step])
            assert torch.equal(st_dev.cpu(), st_cpu), step
            for a, b, c, d, name in zip(dev, cpu, nul, old, ("out", "length", "reason", "stop_index", "logprobs")):
                assert (a is None and b is None) or (torch.equal(a.cpu(), b) and torch.equal(c, d) and torch.equal(c, a)), (name, step)
        assert int((st_cpu < 1000).sum()) > rows // 2 and (rows < 64 or int(cpu[1].max()) == mx and int((cpu[2] == 1).sum()) > 0)


def test_draft_accept_states_refuses_a_single_pointer():
    lib = _lib.load()
    buf = torch.zeros(4 * 24, dtype=torch.int64, device=DEV)  # every pointer of the block is this live buffer: the calls below never launch

    def accept_params(**kw):
        p = _lib.DraftAcceptParams()
        for f in ("fed", "sampled", "out", "length", "reason", "stop_index", "accepted", "live", "start_pos", "shared_len", "feed", "next_pos"):
            setattr(p, f, buf.data_ptr())
        p.rows, p.T, p.n_eos, p.max_new_tokens, p.out_stride = 4, 4, 1, 24, 24
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    st = buf.data_ptr()
    assert lib.hyd_draft_accept_states(C.byref(accept_params()), st, None, None) == -1 and "go together" in lib.hyd_last_error_string().decode()
    assert lib.hyd_draft_accept_states(C.byref(accept_params()), None, st, None) == -1
    assert lib.hyd_draft_accept_states(C.byref(accept_params()), st + 2, st, None) == -1 and "aligned" in lib.hyd_last_error_string().decode()
    assert lib.hyd_draft_accept_states(C.byref(accept_params(T=9)), st, st, None) == -1
    assert lib.hyd_draft_accept_states(C.byref(accept_params(fed=None)), st, st, None) == -1
    assert lib.hyd_draft_accept_states(C.byref(accept_params(rows=0)), st, st, None) == 0  # nothing to do: no launch
    assert lib.hyd_draft_accept_states(C.byref(accept_params(rows=0)), None, None, None) == 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
# fp16 models of tests/test_speculative_gpu.py (cpu_model: 2 layers, 512 tokens, hidden = heads x 64) and its prompts.  Seeds of the
# weights and prompts per head geometry, searched on the CPU with the float64 model alone (ref_logits64, constrained greedy decoding
# of both automata below, seeds 0 .. 399 in order, test_speculative_gpu's own seeds first): the first ones on which, for BOTH
# automata, at least 3/4 of all generated positions lie in front of a row's first top-2 gap (among the allowed tokens) below GAP and
# every row is compared past its first state that is not forced.
SEEDS = {(4, 4): 115, (8, 2): 81}
EOS = 511
# choices that share prefixes and then have long unique tails: behind the branching token every state is forced
TAILS = [[40 + 13 * c + i for i in range(12)] for c in range(5)]
CHOICES = [[7, 8, 20] + TAILS[0], [7, 8, 21] + TAILS[1], [7, 9] + TAILS[2], [7, 9, 22, 23] + TAILS[3], [30] + TAILS[4]]
# a number pattern over a byte vocabulary (tokens 0 .. 255 are the bytes): the literal pieces are forced, the digits are not
AMOUNT = r"\$[1-9][0-9]{2},[0-9]{3}\.[0-9]{2} USD"
BYTE_VOCAB = [bytes([i]) for i in range(256)] + [None] * 256


def automaton(name):
    if name == "choices":
        return TokenDFA.from_choices(CHOICES, 512, eos=[EOS])
    return TokenDFA.from_regex(AMOUNT, BYTE_VOCAB, eos=[EOS])


@torch.no_grad()
def reference_decode(model, prompts, dfa, new=NEW):
    """Constrained greedy decoding with the float64 model on the CPU -> (tokens [B, new] padded with EOS behind a row's end, lengths
    [B] (the EOS counts), gap [B, new]: the top-2 gap among the allowed tokens at every generated position (inf where one token is
    allowed), forced [B, new] bool: the position was drawn in a forced state)."""
    B = prompts.shape[0]
    ids = prompts.clone()
    state = torch.zeros(B, dtype=torch.int32)
    toks = torch.full((B, new), EOS, dtype=torch.int64)
    gap = torch.full((B, new), float("inf"), dtype=torch.float64)
    forced = torch.zeros((B, new), dtype=torch.bool)
    length = torch.zeros(B, dtype=torch.int64)
    done = torch.zeros(B, dtype=torch.bool)
    for p in range(new):
        masked = sampling.constrain_logits(ref_logits64(model, ids)[:, -1], dfa, state)
        top = masked.topk(2, -1).values
        run = ~done
        toks[run, p] = masked.argmax(-1)[run]
        gap[run, p] = (top[:, 0] - top[:, 1])[run]
        inside = (state >= 0) & (state < dfa.num_states)
        forced[run, p] = (inside & (dfa.forced[state.long().clamp(0, dfa.num_states - 1)] >= 0))[run]
        length[run] += 1
        state = torch.where(run, sampling.advance_state(dfa, state, toks[:, p]), state)
        done |= toks[:, p] == EOS
        ids = torch.cat([ids, toks[:, p : p + 1]], 1)
    return toks, length, gap, forced


def compared(length, gap):
    """Per row, how many leading positions are compared: up to the first one whose top-2 gap among the allowed tokens is below GAP."""
    below = gap < GAP
    first = torch.where(below.any(1), below.int().argmax(1), torch.full_like(length, gap.shape[1]))
    return torch.minimum(first, length)


def reference_meets_the_condition(length, gap, forced):
    n = compared(length, gap)
    unforced = (~forced) & (torch.arange(gap.shape[1])[None, :] < length[:, None])
    first_unforced = torch.where(unforced.any(1), unforced.int().argmax(1), length - 1)
    return int(n.sum()) * 4 >= int(length.sum()) * 3 and bool((n > first_unforced).all())


_SETUP = {}


def setup(heads, kv_heads):
    """The GPU model with the CPU model's weights, its prompts, and per automaton the float64 reference's decode -- once per geometry."""
    if (heads, kv_heads) not in _SETUP:
        from tests.test_model_gpu import make_model

        seed = SEEDS[(heads, kv_heads)]
        cpu = cpu_model(heads, kv_heads, seed)
        model = make_model(torch.float16, head_dim=64, kv_heads=kv_heads, layers=2, heads=heads)
        with torch.no_grad():
            for p, c in zip(model.parameters(), cpu.parameters()):
                p.copy_(c)
        model.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[PROMPT])
        prompts = cpu_prompts(seed)
        refs = {}
        for name in ("choices", "amount"):
            dfa = automaton(name)
            toks, length, gap, forced = reference_decode(cpu, prompts.repeat_interleave(3, 0), dfa)
            assert reference_meets_the_condition(length, gap, forced), (heads, kv_heads, name)
            refs[name] = (dfa.to(DEV), toks, length, compared(length, gap))
        _SETUP[(heads, kv_heads)] = (model, prompts.to(DEV), refs)
    return _SETUP[(heads, kv_heads)]


def gen(model, prompts, dfa, **kw):
    kw.setdefault("temperature", 0)
    return model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, eos_token_id=[EOS], constraint=dfa,
                          return_constraint_state=True, return_finish=True, **kw)


def drafted(model, prompts, dfa, K, draft, **kw):
    model.stop_poll_steps = 1
    try:
        return gen(model, prompts, dfa, draft_tokens=K, draft=draft, return_draft_stats=True, **kw)
    finally:
        del model.stop_poll_steps


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("name", ["choices", "amount"])
def test_generate_with_drafts_returns_constrained_decoding(heads, kv_heads, name):
    """Tokens and final states of generate(constraint=, draft_tokens=K, draft=d) are those of generate(constraint=), compared up to the
    first position at which the float64 model's top-2 gap among the allowed tokens is below GAP (setup asserts how much that is)."""
    model, prompts, refs = setup(heads, kv_heads)
    dfa, ref_toks, ref_len, n = refs[name]
    want, fin, want_state = gen(model, prompts, dfa)
    want, want_len, want_state = want.cpu(), fin.lengths.cpu().long(), want_state.cpu()
    whole = n == ref_len  # rows compared to their end: lengths and final states are compared too
    for b in range(6):
        assert torch.equal(want[b, : n[b]], ref_toks[b, : n[b]]), (b, want[b].tolist(), ref_toks[b].tolist())
    assert torch.equal(want_len[whole], ref_len[whole])
    for K in (1, 3, 7):
        for d in ("constraint", "prompt_lookup"):
            out, fin, state, stats = drafted(model, prompts, dfa, K, d)
            out = out.cpu()
            for b in range(6):
                assert torch.equal(out[b, : n[b]], want[b, : n[b]]), (K, d, b, out[b].tolist(), want[b].tolist())
            assert torch.equal(fin.lengths.cpu().long()[whole], want_len[whole]) and torch.equal(state.cpu()[whole], want_state[whole]), (K, d)
            proposed, accepted, forced = stats.proposed.cpu(), stats.accepted.cpu(), stats.forced.cpu()
            assert bool((accepted <= proposed).all()) and bool((forced <= proposed).all()), (K, d)
            assert int(forced.sum()) > 0  # both automata have forced states on every row's path
            if d == "constraint":  # (accepted < proposed where a step's chain runs on behind the row's EOS: the sink is forced too)
                assert torch.equal(forced, proposed) and int(accepted.sum()) > 0, (K, d)


@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_a_fully_forced_choice_is_accepted_whole(K, temperature):
    """One choice of 20 tokens + EOS: every state is forced, so the output is the choice whatever the weights and the temperature,
    every draft is accepted, and the step count is the closed form (forced_steps, checked against accept_states_reference in
    tests/test_constrained_drafts.py): DraftStats.steps counts the decode steps the host enqueued -- the ceil((len - 1) / (K + 1))
    that emit and, with stop_poll_steps = 1, exactly one more before the host reads that no row is running; the CPU loop counts the
    first token's step instead.  max_new_tokens = len, so that only drafts that can become output count as proposed."""
    model, prompts, _ = setup(4, 4)
    choice = [(37 * i + 11) % 500 + 1 for i in range(20)]
    dfa = TokenDFA.from_choices([choice], 512, eos=[EOS]).to(DEV)
    total = len(choice) + 1
    torch.manual_seed(K)
    model.stop_poll_steps = 1
    try:
        out, fin, state, stats = model.generate([prompts], num_return_sequences=3, max_new_tokens=total, temperature=temperature,
                                                eos_token_id=[EOS], constraint=dfa, draft_tokens=K, draft="constraint",
                                                return_constraint_state=True, return_finish=True, return_draft_stats=True)
    finally:
        del model.stop_poll_steps
    assert out.tolist() == [choice + [EOS]] * 6 and fin.lengths.tolist() == [total] * 6 and fin.reasons.tolist() == [1] * 6
    assert dfa.choice_of(state).tolist() == [0] * 6
    assert stats.steps == forced_steps(total, K), stats.steps
    emitting = stats.steps - 1
    assert stats.accepted.tolist() == stats.proposed.tolist() == stats.forced.tolist() == [total - 1 - emitting] * 6


@pytest.mark.parametrize("name", ["choices", "amount"])
@pytest.mark.parametrize("d", ["constraint", "prompt_lookup"])
def test_sampled_rows_are_accepted_by_a_walk_of_the_automaton(name, d):
    """temperature 1, top-p 0.9: whatever is drawn, every emitted row walks through the automaton on the CPU, and the returned
    states are the walk's."""
    model, prompts, refs = setup(4, 4)
    dfa = refs[name][0]
    nxt = dfa.next.cpu()
    for K in (3, 7):
        torch.manual_seed(10 * K)
        out, fin, state, stats = drafted(model, prompts, dfa, K, d, temperature=1.0, top_p=0.9)
        out, lens = out.cpu(), fin.lengths.cpu()
        for b in range(6):
            s = 0
            for t in out[b, : lens[b]].tolist():
                assert 0 <= s < dfa.num_states and int(nxt[s, t]) != sampling.DFA_REJECT, (K, b, out[b].tolist())
                s = int(nxt[s, t])
            assert s == int(state[b]), (K, b)
            assert int(fin.reasons[b]) == 1 and out[b, lens[b] - 1] == EOS  # both automata end within NEW tokens
        assert int(stats.accepted.sum()) > 0


def test_choose_with_forced_drafts_returns_the_same_choices():
    model, prompts, refs = setup(4, 4)
    _, _, ref_len, n = refs["choices"]
    whole = (n == ref_len).to(DEV)
    idx, toks = model.choose([prompts], CHOICES, EOS, num_return_sequences=3)
    idx3, toks3 = model.choose([prompts], CHOICES, EOS, num_return_sequences=3, draft_tokens=3, draft="constraint")
    assert bool(whole.any()) and torch.equal(idx3[whole], idx[whole]) and bool((idx[whole] >= 0).all())
    for b in range(6):
        assert torch.equal(toks3[b, : n[b]], toks[b, : n[b]])


def test_graph_decode_on_and_off_return_the_same_tokens():
    model, prompts, refs = setup(4, 4)
    dfa, _, _, n = refs["amount"]
    eager = drafted(model, prompts, dfa, 3, "constraint")
    model.graph(True)
    try:
        graphed = drafted(model, prompts, dfa, 3, "constraint")
    finally:
        model.graph(False)
    for b in range(6):
        assert torch.equal(eager[0][b, : n[b]], graphed[0][b, : n[b]])
    assert int(graphed[3].accepted.sum()) > 0


def test_refusals():
    model, prompts, refs = setup(4, 4)
    dfa = refs["choices"][0]
    with pytest.raises(ValueError, match="needs constraint"):
        model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, draft_tokens=3, draft="constraint")
    for kw, words in ((dict(repetition_penalty=1.2), "penalties"), (dict(logit_bias={3: -1.0}), "logit_bias"), (dict(stop=[[1, 2]]), "stop"),
                      (dict(return_logprobs=True, top_logprobs=2), "top_logprobs"), (dict(return_logits=True), "return_logits"),
                      (dict(disable_attention=True), "disable_attention")):
        with pytest.raises(NotImplementedError, match=words):
            model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, constraint=dfa, draft_tokens=3, draft="constraint", **kw)
