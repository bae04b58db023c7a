"""-m gpu: hyd_sample_tokens_constrained (csrc/sample_constrain.hip) against the kernels that already exist, bit for bit -- the
constrained draw IS hyd_sample_tokens_filtered / hyd_sample_tokens_penalized on logits filled with -inf where the row's automaton
state does not allow a token -- and generate(constraint=) on the tiny model.

The automaton of the kernel tests has 8 states, not 7: "exactly one token" is three states, one per placement (v = 0, v = V - 1,
the first bit of the last partial word), so that every launch sees all three."""
import math
import re

import pytest
import torch

from hydragen_amd import _lib, layer_ops, sampling
from hydragen_amd.constraint import TokenDFA, pack_allowed
from hydragen_amd.layer_ops import Penalties
from hydragen_amd.sampling import DFA_FREE, DFA_REJECT
from tests import penalty_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
GRID = [(20, None, None), (1, None, None), (None, 0.9, None), (None, 0.5, None), (None, None, 0.05), (50, 0.95, None),
        (None, 0.95, 0.01), (40, 0.8, 0.1), (1000, 0.99, None)]  # tests/test_sampling_penalties_gpu.py's cut combinations
CUTS = [(None, None, None)] + GRID
KEY = (5, 8)
S = 8
REJECT_ALL, ONE_FIRST, ONE_LAST, ONE_WORD, PERCENT, HALF, ALL, NOT_BEST = range(S)
SLOTS = list(range(S)) + [-1, S]  # rows are dealt over the states and two states outside the automaton


def _same(a, b):
    """Bit equality of (tokens, log-probs, kept) triples: NaN log-probs compare by their bits."""
    return (torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2]))


def _automaton(V, rows, seed, best):
    """(dfa on the GPU with poisoned padding bits, state int32 [rows], mask bool [rows, V] from `next`).  `best`: the token the
    NOT_BEST state bans (the test plants it as the arg-max of the rows in that state)."""
    g = torch.Generator().manual_seed(seed)
    ok = torch.zeros((S, V), dtype=torch.bool)
    ok[ONE_FIRST, 0] = ok[ONE_LAST, V - 1] = ok[ONE_WORD, ((V - 1) // 32) * 32] = True
    ok[PERCENT] = torch.rand(V, generator=g) < 0.01
    ok[HALF] = torch.rand(V, generator=g) < 0.5
    ok[ALL] = True
    ok[NOT_BEST] = True
    ok[NOT_BEST, best] = False
    target = torch.randint(0, S, (S, V), generator=g)
    target = torch.where(torch.rand(S, V, generator=g) < 0.1, torch.full_like(target, DFA_FREE), target)
    dfa = TokenDFA(torch.where(ok, target, torch.full_like(target, DFA_REJECT)).to(torch.int32)).to(DEV)
    if V % 32:  # bits at positions >= V are ignored: set them
        dfa.allowed[:, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32, device=DEV)
        assert not torch.equal(dfa.allowed, pack_allowed(dfa.next))
    state = torch.tensor([SLOTS[i % len(SLOTS)] for i in range(rows)], dtype=torch.int32, device=DEV)
    return dfa, state, sampling.allowed_mask(TokenDFA(dfa.next), state)


def _logits(V, pad, rows, dtype, best):
    g = torch.Generator(device=DEV).manual_seed(V + pad)
    x = (torch.randn(rows, V + pad, device=DEV, generator=g) * 3.0).to(dtype)
    x[NOT_BEST :: len(SLOTS), best] = 30.0  # the banned token of the NOT_BEST rows is their arg-max
    return x[:, :V]


def _check_states_and_tokens(dfa, st0, mask, got, st_after):
    tok, lp, kept = got
    drew = kept > 0
    assert torch.equal(st_after, sampling.advance_state(dfa, st0, tok, drew))
    assert (tok >= 0).all() and (tok < dfa.vocab_size).all() and mask.gather(1, tok)[drew].all()  # never a banned token
    dead = st0 == REJECT_ALL
    assert dead.any() and (tok[dead] == 0).all() and (kept[dead] == 0).all() and torch.isnan(lp[dead]).all()
    assert torch.equal(st_after[dead], st0[dead]) and drew[~dead].all()


# ---- neutral penalties: the filtered kernel on masked logits, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("V, pad, rows", [(1000, 0, 96), (31997, 0, 96), (32000, 24, 96), (128256, 0, 96), (262176, 0, 4)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_constrained_is_the_filtered_sampler_on_masked_logits(V, pad, rows, dtype):
    best = V // 3
    x = _logits(V, pad, rows, dtype, best)
    if rows < len(SLOTS):  # the wide rows: reject-all, the last word, 50 %, unconstrained
        slots = torch.tensor([REJECT_ALL, ONE_WORD, HALF, -1], dtype=torch.int32, device=DEV)
    dfa, st0, mask = _automaton(V, rows, V, best)
    if rows < len(SLOTS):
        st0 = slots
        mask = sampling.allowed_mask(TokenDFA(dfa.next), st0)
    masked = x.masked_fill(~mask, -math.inf)
    unc = (st0 < 0) | (st0 >= S)
    for T in (0.0, 0.9):
        for top_k, top_p, min_p in CUTS:
            cuts = dict(top_k=top_k, top_p=top_p, min_p=min_p)
            want = layer_ops.sample_tokens_filtered(masked, T, key=KEY, **cuts)
            st = st0.clone()
            got = layer_ops.sample_tokens_constrained(x, T, key=KEY, constraint=(dfa, st, True), **cuts)
            assert _same(got, want), (T, cuts)
            _check_states_and_tokens(dfa, st0, mask, got, st)
            # neutral penalties given explicitly, and an empty list of generated tokens: the same bits
            empty = Penalties(1.0, 0.0, 0.0, gen=torch.full((rows, 8), 5, dtype=torch.int32, device=DEV),
                              gen_len=torch.zeros(rows, dtype=torch.int32, device=DEV))
            assert _same(layer_ops.sample_tokens_constrained(x, T, key=KEY, constraint=(dfa, st0.clone(), True), penalties=empty, **cuts), want)
    # unconstrained rows are the unconstrained kernel's rows
    plain = layer_ops.sample_tokens_filtered(x, 0.9, key=KEY, top_k=50, top_p=0.95)
    st = st0.clone()
    got = layer_ops.sample_tokens_constrained(x, 0.9, key=KEY, constraint=(dfa, st, False), top_k=50, top_p=0.95)
    assert unc.any() and all(torch.equal(u[unc], v[unc]) for u, v in zip(got, plain))
    assert torch.equal(st, st0)  # advance = 0: the state is untouched
    # twice in a row: the same bits
    assert _same(layer_ops.sample_tokens_constrained(x, 0.9, key=KEY, constraint=(dfa, st0.clone(), True), top_k=50, top_p=0.95), got)
    # the same rows launched alone (temperature 0: the noise is keyed by the row index)
    sub = torch.arange(rows, device=DEV)[:: max(rows // 12, 1)]
    whole = layer_ops.sample_tokens_constrained(x, 0.0, constraint=(dfa, st0.clone(), True), top_k=50, top_p=0.9)
    alone = layer_ops.sample_tokens_constrained(x[sub].contiguous(), 0.0, constraint=(dfa, st0[sub].contiguous(), True), top_k=50, top_p=0.9)
    assert _same(alone, tuple(t[sub] for t in whole))


def test_constraint_none_takes_the_old_entry_points(monkeypatch):
    lib = _lib.load()
    calls = []
    real = lib.hyd_sample_tokens_constrained

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "hyd_sample_tokens_constrained", spy)
    x = _logits(1000, 0, 16, torch.bfloat16, 3)
    dfa, st, _ = _automaton(1000, 16, 1, 3)
    assert torch.equal(layer_ops.sample_tokens(x, 0.9, key=KEY, constraint=None), layer_ops.sample_tokens(x, 0.9, key=KEY))
    a = layer_ops.sample_tokens(x, 0.9, key=KEY, top_p=0.9, penalties=Penalties(1.3), constraint=None)
    assert torch.equal(a, layer_ops.sample_tokens(x, 0.9, key=KEY, top_p=0.9, penalties=Penalties(1.3))) and calls == []
    layer_ops.sample_tokens(x, 0.9, key=KEY, constraint=(dfa, st, True))
    assert len(calls) == 1


# ---- with penalties: the penalised kernel on masked logits, bit for bit ------------------------------------------------------------
def _dev(name):
    """tests/penalty_cases.py's case on the GPU: (logits, Penalties)."""
    case = PC.build(name)
    n = case["logits"].shape[1]
    ctx = [(layer_ops.token_bitmap(ids.to(DEV), lens.to(DEV), n), rpg) for (_, rpg), (ids, lens, _) in zip(case["context"], case["context_ids"])]
    pen = Penalties(case["r"], case["a"], case["f"], sampling.normalize_logit_bias(case["bias"], DEV), ctx,
                    None if case["gen"] is None else case["gen"].to(DEV), None if case["gen"] is None else case["gen_len"].to(DEV))
    return case["logits"].to(DEV), pen


@pytest.mark.parametrize("name", list(PC.CASES))
def test_constrained_is_the_penalised_sampler_on_masked_logits(name):
    x, pen = _dev(name)
    rows, V = x.shape
    best = V // 3
    x[NOT_BEST :: len(SLOTS), best] = 30.0
    dfa, st0, mask = _automaton(V, rows, PC.CASES[name]["seed"], best)
    if rows < len(SLOTS):
        st0 = torch.tensor([REJECT_ALL, ONE_WORD, HALF, -1, PERCENT, NOT_BEST, ALL][:rows], dtype=torch.int32, device=DEV)
        mask = sampling.allowed_mask(TokenDFA(dfa.next), st0)
    masked = x.masked_fill(~mask, -math.inf)
    unc = (st0 < 0) | (st0 >= S)
    dead = st0 == REJECT_ALL
    for T in (0.0, 0.9):
        for top_k, top_p, min_p in CUTS:
            cuts = dict(top_k=top_k, top_p=top_p, min_p=min_p)
            want = layer_ops.sample_tokens_penalized(masked, T, key=KEY, penalties=pen, **cuts)
            st = st0.clone()
            got = layer_ops.sample_tokens_constrained(x, T, key=KEY, constraint=(dfa, st, True), penalties=pen, **cuts)
            assert _same(got, want), (T, cuts)
            tok, lp, kept = got
            drew = kept > 0
            assert torch.equal(st, sampling.advance_state(dfa, st0, tok, drew)) and mask.gather(1, tok)[drew].all()
            if dead.any():
                assert (tok[dead] == 0).all() and (kept[dead] == 0).all() and torch.isnan(lp[dead]).all() and torch.equal(st[dead], st0[dead])
    if unc.any():
        plain = layer_ops.sample_tokens_penalized(x, 0.9, key=KEY, penalties=pen, top_p=0.9)
        got = layer_ops.sample_tokens_constrained(x, 0.9, key=KEY, constraint=(dfa, st0.clone(), False), penalties=pen, top_p=0.9)
        assert all(torch.equal(u[unc], v[unc]) for u, v in zip(got, plain))


def test_wide_rows_with_penalties_and_the_append():
    """Rows wider than the context bitmap the penalty map keeps in LDS (262144 tokens), and append_out next to the state update."""
    V, rows = 262176, 4
    best = V // 3
    x = _logits(V, 0, rows, torch.bfloat16, best)
    dfa, _, _ = _automaton(V, rows, 17, best)
    st0 = torch.tensor([REJECT_ALL, ONE_WORD, HALF, -1], dtype=torch.int32, device=DEV)
    mask = sampling.allowed_mask(TokenDFA(dfa.next), st0)
    masked = x.masked_fill(~mask, -math.inf)
    top = torch.topk(x.float(), 8, dim=-1).indices
    ctx = [(layer_ops.token_bitmap(top[:, :3].contiguous(), None, V), 1)]

    def pen(append):
        return Penalties(1.3, 0.2, 0.4, sampling.normalize_logit_bias({int(top[2, 0]): -math.inf, V - 1: 2.0}, DEV), ctx,
                         torch.cat([top[:, 3:6].to(torch.int32), torch.full((rows, 2), -1, dtype=torch.int32, device=DEV)], 1).contiguous(),
                         torch.full((rows,), 3, dtype=torch.int32, device=DEV), append)

    for T in (0.0, 0.9):
        for top_k, top_p, min_p in CUTS:
            cuts = dict(top_k=top_k, top_p=top_p, min_p=min_p)
            want = layer_ops.sample_tokens_penalized(masked, T, key=KEY, penalties=pen(False), **cuts)
            st = st0.clone()
            assert _same(layer_ops.sample_tokens_constrained(x, T, key=KEY, constraint=(dfa, st, True), penalties=pen(False), **cuts), want)
            assert torch.equal(st, sampling.advance_state(dfa, st0, want[0], want[2] > 0))
    a, b = pen(True), pen(True)
    want = layer_ops.sample_tokens_penalized(masked, 0.9, key=KEY, penalties=a, top_p=0.9)
    st = st0.clone()
    got = layer_ops.sample_tokens_constrained(x, 0.9, key=KEY, constraint=(dfa, st, True), penalties=b, top_p=0.9)
    assert _same(got, want) and torch.equal(a.gen, b.gen) and torch.equal(a.gen_len, b.gen_len) and b.gen_len.tolist() == [4] * rows
    assert torch.equal(st, sampling.advance_state(dfa, st0, got[0], got[2] > 0))
    with pytest.raises(ValueError, match="state"):
        layer_ops.sample_tokens_constrained(x, 0.9, constraint=(dfa, st0[:3].contiguous(), True))
    with pytest.raises(ValueError, match="tokens"):
        layer_ops.sample_tokens_constrained(x[:, : V - 1], 0.9, constraint=(dfa, st0, True))


# ---- the model shell -------------------------------------------------------------------------------------------------------
EOS = 511


def _model(dtype=torch.bfloat16, seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    model = HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=DEV, seed=seed, std=0.05)
    model.setup_caches(max_unique_batch_size=8, max_unique_seq_length=48, max_shared_batch_sizes=[1, 2], max_shared_seq_lengths=[256, 40])
    return model


def _prompt(seed, shape=(1, 40)):
    return torch.randint(1, 500, shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


CHOICES = [[5, 6, 7], [5, 6], [9], [300, 301, 302, 303], [5, 8]]


@pytest.mark.parametrize("graph", [False, True])
def test_generate_choices(graph):
    model = _model()
    model.graph(graph)
    dfa = TokenDFA.from_choices(CHOICES, 512, eos=[EOS]).to(DEV)
    torch.manual_seed(3)
    out, fin, states = model.generate(input_ids=_prompt(1), num_return_sequences=8, max_new_tokens=8, temperature=1.0, eos_token_id=[EOS],
                                      constraint=dfa, return_finish=True, return_constraint_state=True)
    assert states.dtype == torch.int32 and states.shape == (8,) and fin.reasons.tolist() == [1] * 8
    picked = dfa.choice_of(states).tolist()
    for r in range(8):
        assert picked[r] >= 0 and out[r, : int(fin.lengths[r])].tolist() == CHOICES[picked[r]] + [EOS], (r, out[r], picked[r])
    # two prompt groups with their own choice sets, through constraint_state (the leaf batch's start states, repeated per sample)
    groups = [[[11, 12], [13]], [[13, 14, 15], [11], [12, 12]]]
    g = TokenDFA.from_choices(groups, 512, eos=[EOS]).to(DEV)
    kw = dict(input_ids=[_prompt(2), _prompt(3, (2, 6))], num_return_sequences=4, temperature=1.0)
    out, fin, states = model.generate(max_new_tokens=6, eos_token_id=[EOS], constraint=g, return_finish=True, return_constraint_state=True,
                                      constraint_state=torch.tensor(g.start_states), **kw)
    picked = g.choice_of(states).tolist()
    assert fin.reasons.tolist() == [1] * 8
    for r in range(8):
        assert out[r, : int(fin.lengths[r])].tolist() == groups[r // 4][picked[r]] + [EOS], (r, out[r], picked[r])
    # the convenience wrapper: greedy by default, the same answer for the samples of a prompt, an index within the row's own set
    idx, toks = model.choose(kw["input_ids"], groups, EOS, num_return_sequences=4)
    assert idx.shape == (8,) and (idx >= 0).all() and (idx[:4] == idx[0]).all() and (idx[4:] == idx[4]).all()
    for r in range(8):
        want = groups[r // 4][int(idx[r])] + [EOS]
        assert toks[r, : len(want)].tolist() == want
    with pytest.raises(ValueError, match="constraint_state"):
        model.generate(max_new_tokens=6, constraint=g, constraint_state=torch.zeros(3, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="token_overrides"):
        model.generate(max_new_tokens=6, constraint=g, token_overrides=torch.zeros((8, 6), dtype=torch.long, device=DEV), **kw)
    model.graph(False)


@pytest.mark.parametrize("graph", [False, True])
def test_generate_greedy_attains_the_masked_maximum_and_logprobs(graph):
    model = _model()
    model.graph(graph)
    dfa = TokenDFA.from_choices(CHOICES, 512, eos=[EOS]).to(DEV)
    lens = torch.tensor([6, 3, 4, 6, 1, 2, 5, 6], device=DEV)
    out, logits, lp, states = model.generate(input_ids=[_prompt(4), _prompt(5, (8, 6))], seq_lens=[torch.tensor([40], device=DEV), lens],
                                             max_new_tokens=7, temperature=0.0, constraint=dfa, return_logits=True, return_logprobs=True,
                                             return_constraint_state=True)
    st = torch.zeros(8, dtype=torch.int32, device=DEV)
    for j, lg in enumerate(logits):
        masked = sampling.constrain_logits(lg, dfa, st)
        at = masked.gather(1, out[:, j : j + 1])[:, 0]
        assert torch.equal(at, masked.amax(-1)) and (at > -math.inf).all()  # the token attains the maximum of the masked logits
        want = torch.log_softmax(masked.double(), -1).gather(1, out[:, j : j + 1])[:, 0]
        assert (lp[:, j].double() - want).abs().max() < 1e-4  # the CONSTRAINED distribution
        st = sampling.advance_state(dfa, st, out[:, j])
    assert torch.equal(st, states) and (dfa.choice_of(states) >= 0).all()  # 7 steps: every row is behind its choice's EOS
    assert (out[:, -1] == EOS).all()
    model.graph(False)


NUMBER = r"-?(0|[1-9][0-9]{0,3})(\.[0-9]{1,2})?"
BYTE_VOCAB = [bytes([i]) for i in range(256)] + [None] * 256  # tokens 0..255 are the bytes, the rest (EOS included) carry none


@pytest.mark.parametrize("graph", [False, True])
def test_generate_regex_number(graph):
    model = _model()
    model.graph(graph)
    dfa = TokenDFA.from_regex(NUMBER, BYTE_VOCAB, eos=[EOS]).to(DEV)
    torch.manual_seed(5)
    out, fin = model.generate(input_ids=_prompt(6), num_return_sequences=8, max_new_tokens=12, temperature=1.0, top_p=0.98,
                              eos_token_id=[EOS], constraint=dfa, return_finish=True)
    assert fin.reasons.tolist() == [1] * 8  # at most 8 bytes match: every row has finished
    seen = set()
    for r in range(8):
        n = int(fin.lengths[r])
        data = bytes(out[r, : n - 1].tolist())
        assert out[r, n - 1] == EOS and re.fullmatch(NUMBER.encode(), data), (r, data)
        seen.add(data)
    assert len(seen) > 1
    model.graph(False)


@pytest.mark.parametrize("graph", [False, True])
def test_generate_constraint_with_repetition_penalty_and_stop(graph):
    model = _model()
    model.graph(graph)
    dfa = TokenDFA.from_regex(r"[a-p]+", BYTE_VOCAB, eos=[EOS]).to(DEV)
    shared, unique = _prompt(7), _prompt(8, (8, 6))
    lens = torch.tensor([6, 3, 4, 6, 1, 2, 5, 6], device=DEV)
    kw = dict(input_ids=[shared, unique], seq_lens=[torch.tensor([40], device=DEV), lens], max_new_tokens=10, temperature=0.0,
              repetition_penalty=1.7, constraint=dfa, return_logits=True)
    out, logits = model.generate(**kw)
    ctx = [(layer_ops.token_bitmap(shared, None, 512), 8), (layer_ops.token_bitmap(unique, lens, 512), 1)]
    st = torch.zeros(8, dtype=torch.int32, device=DEV)
    skipped = 0
    for j, lg in enumerate(logits):
        x = sampling.penalize_logits(lg, 1.7, context=ctx, gen=out[:, :j].to(torch.int32), gen_len=torch.full((8,), j, dtype=torch.int32, device=DEV))
        x = sampling.constrain_logits(x, dfa, st)
        skip = PC.margin_rows(x)
        skipped += int(skip.sum())
        assert torch.equal(out[~skip, j], PC.greedy(x)[~skip])  # constraint and penalty
        st = sampling.advance_state(dfa, st, out[:, j])
    assert skipped <= 0.05 * out.numel()
    assert ((out >= ord("a")) & (out <= ord("p")) | (out == EOS)).all()
    # the same call with a stop sequence taken from row 0: it ends there (reason 2), the others go on as before until theirs
    stop = out[0, 2:4].tolist()
    out2, _, fin = model.generate(stop=[stop], return_finish=True, **kw)
    assert int(fin.reasons[0]) == 2 and int(fin.lengths[0]) <= 2 and out2[0, : int(fin.lengths[0])].tolist() == out[0, : int(fin.lengths[0])].tolist()
    for r in range(8):
        n = int(fin.lengths[r])
        assert out2[r, :n].tolist() == out[r, :n].tolist()
        row = out[r].tolist()
        hit = [i for i in range(len(row) - 1) if row[i : i + 2] == stop]
        assert (int(fin.reasons[r]) == 2) == bool(hit) and (not hit or n == hit[0])
    model.graph(False)
