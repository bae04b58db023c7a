"""-m "not gpu": per-row sampling values, seeds and token limits -- the torch definitions (hydragen_amd/sampling.py, stopping.py)
against their own scalar form, generate() on a tiny CPU model, and the refusals of hyd_sample_tokens_rows / hyd_stop_update_rows
that come before any launch."""
import ctypes as C
import math

import pytest
import torch

from hydragen_amd import _lib, sampling, stopping
from tests import abi_table
from tests.per_row_cases import NAMES, TABLE

B, N = 24, 97


def _rows():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, N, generator=g) * 3.0
    x[5] = -math.inf
    x[6] = 1.25
    x[7, ::2] = -math.inf
    x[7, 1::3] = math.nan
    return x


def _cols():
    return {name: [TABLE[r % len(TABLE)][i] for r in range(B)] for i, name in enumerate(NAMES)}


def _same(a, b):
    return torch.equal(torch.nan_to_num(a.double(), nan=12345.0), torch.nan_to_num(b.double(), nan=12345.0))


def _context_and_gen():
    g = torch.Generator().manual_seed(2)
    ctx = sampling.token_bitmap_reference(torch.randint(0, N, (B // 4, 9), generator=g), None, N)
    gen = torch.randint(0, N, (B, 8), generator=g).to(torch.int32)
    return [(ctx, 4)], gen, (torch.arange(B) % 9).clamp(max=8).to(torch.int32)


# ---- the definitions: a row of a per-row call is that row of the scalar call ---------------------------------------------------------
@pytest.mark.parametrize("as_tensor", [False, True])
def test_kept_mask_and_filter_logits_per_row(as_tensor):
    x, c = _rows(), _cols()
    wrap = (lambda v, dt: torch.tensor(v, dtype=dt)) if as_tensor else (lambda v, dt: v)
    k, p, m = wrap(c["top_k"], torch.int64), wrap(c["top_p"], torch.float64), wrap(c["min_p"], torch.float64)
    keep, filt = sampling.kept_mask(x, k, p, m), sampling.filter_logits(x, k, p, m)
    for r in range(B):
        want = (c["top_k"][r], c["top_p"][r], c["min_p"][r])
        assert torch.equal(keep[r], sampling.kept_mask(x[r : r + 1], *want)[0]), r
        assert _same(filt[r], sampling.filter_logits(x[r : r + 1], *want)[0]), r
    assert len({tuple(keep[r].tolist()) for r in range(B)}) > 6  # (the combinations do cut differently)
    # a scalar as a 1-element broadcast changes nothing
    assert torch.equal(sampling.kept_mask(x, [40], torch.tensor([0.9]), (0.05,)), sampling.kept_mask(x, 40, 0.9, 0.05))
    assert torch.equal(sampling.kept_mask(x, [None], None, [None]), sampling.kept_mask(x))


def test_penalize_logits_per_row():
    x, c = _rows(), _cols()
    ctx, gen, gen_len = _context_and_gen()
    got = sampling.penalize_logits(x, c["repetition_penalty"], c["presence_penalty"], c["frequency_penalty"], {3: -2.0, 96: 1.5}, ctx, gen, gen_len)
    whole = {}
    for r in range(B):
        key = (c["repetition_penalty"][r], c["presence_penalty"][r], c["frequency_penalty"][r])
        if key not in whole:  # the scalar call over the whole batch, once per combination
            whole[key] = sampling.penalize_logits(x, *key, {3: -2.0, 96: 1.5}, ctx, gen, gen_len)
        assert _same(got[r], whole[key][r]), r
    assert len(whole) >= 8
    one = sampling.penalize_logits(x, [TABLE[5][4]], torch.tensor([TABLE[5][6]]), (TABLE[5][5],), None, ctx, gen, gen_len)
    assert _same(one, sampling.penalize_logits(x, TABLE[5][4], TABLE[5][6], TABLE[5][5], None, ctx, gen, gen_len))


def test_reference_draw_per_row():
    x, c = _rows().double(), _cols()
    seeds = [1000 + 7 * r for r in range(B)]
    tok, lp, drawn = sampling.reference_draw(x, c["temperature"], c["top_k"], c["top_p"], c["min_p"], seed=seeds, offset=4)
    before = torch.random.get_rng_state()
    for r in range(B):
        t1, l1, d1 = sampling.reference_draw(x[r : r + 1], c["temperature"][r], c["top_k"][r], c["top_p"][r], c["min_p"][r], seed=[seeds[r]], offset=4)
        assert torch.equal(tok[r : r + 1], t1) and _same(lp[r : r + 1], l1) and torch.equal(drawn[r : r + 1], d1), r
    assert torch.equal(before, torch.random.get_rng_state())  # seeded draws leave the global generator alone
    assert not drawn[5] and tok[5, 0] == 0 and math.isnan(lp[5])
    # another offset or another seed: another draw (on the rows that sample)
    other = sampling.reference_draw(x, c["temperature"], c["top_k"], c["top_p"], c["min_p"], seed=seeds, offset=5)[0]
    assert (other != tok).any()
    # without seeds, every row equal: the scalar call's single draw from the global generator
    torch.manual_seed(3)
    a = sampling.reference_draw(x, [0.7] * B, [40], 0.9, None)[0]
    torch.manual_seed(3)
    assert torch.equal(a, sampling.reference_draw(x, 0.7, 40, 0.9, None)[0])
    # greedy rows of a mixed call are the greedy call's rows
    mixed = sampling.reference_draw(x, c["temperature"])[0]
    greedy = sampling.reference_draw(x, 0.0)[0]
    zero = torch.tensor([t == 0 for t in c["temperature"]])
    assert zero.any() and torch.equal(mixed[zero], greedy[zero])


def test_per_row_lists_are_checked_element_by_element():
    with pytest.raises(ValueError, match=r"top_k -1 must be >= 0"):
        sampling.check_filters([0, 5, -1], None, None)
    with pytest.raises(ValueError, match=r"top_p 1.5 must be in \(0, 1\]"):
        sampling.check_filters(None, [0.9, None, 1.5], None)
    with pytest.raises(ValueError, match=r"min_p -0.1 must be in \[0, 1\]"):
        sampling.check_filters(None, None, [0.0, -0.1])
    with pytest.raises(ValueError, match=r"repetition_penalty 0.0 must be a finite number > 0"):
        sampling.check_penalties([1.0, None, 0.0])
    with pytest.raises(ValueError, match=r"frequency_penalty inf must be finite"):
        sampling.check_penalties(None, None, [0.0, math.inf])
    sampling.check_filters([0, None, 40], [1.0, None, 0.5], [None, 0.05, 0.0])
    sampling.check_penalties([1.0, None, 1.3], [None, 0.5], [0.0, -0.5])
    with pytest.raises(ValueError, match="3 per-row values for 24 rows"):
        sampling.kept_mask(_rows(), [1, 2, 3])


def test_sample_route_per_row():
    for constraint, penalties, want in ((False, False, sampling.FILTERED), (False, True, sampling.PENALIZED), (True, False, sampling.CONSTRAINED),
                                        (True, True, sampling.CONSTRAINED)):
        for cuda in (True, False):
            for num_samples in (1, 4):
                for eligible in (True, False):
                    route = sampling.sample_route(cuda, eligible, eligible, num_samples, constraint, penalties, True, False, False, False, per_row=True)
                    assert route == sampling.SampleRoute(want)  # a kernel route, no torch stage, whatever the switches say
    assert sampling.sample_route(True, True, True, 1, False, False, False, False) == sampling.SampleRoute(sampling.PLAIN)  # the default: the table


# ---- stop conditions with a limit per row -------------------------------------------------------------------------------------------
def _stop_rows():
    g = torch.Generator().manual_seed(4)
    T = 10
    toks = torch.randint(20, 30, (12, T), generator=g)  # (no condition met by chance)
    spec = stopping.check_stop([7, 3], [[5], [1, 2, 4]], pad_token_id=11, include_stop=False, vocab_size=32)
    limits = torch.tensor([1, T, 4, 4, 4, 3, 6, 2, 12, 5, 5, 7], dtype=torch.int32)
    toks[2, 3] = 7                           # an EOS exactly at the limit: reason 1, not 3
    toks[3, 2:5] = torch.tensor([1, 2, 4])   # a stop sequence that would complete one step after the limit: never matched
    toks[4, 1:4] = torch.tensor([1, 2, 4])   # ... and one that completes at the limit: reason 2
    toks[5, 1] = 5                           # a one-token stop before the limit
    toks[6, 8] = 3                           # an EOS after the limit: never seen
    toks[8, 9] = 3                           # a limit past the width: the EOS at the last step counts
    return toks, spec, limits


@pytest.mark.parametrize("include_stop", [False, True])
def test_stop_definitions_agree_under_per_row_limits(include_stop):
    toks, spec, limits = _stop_rows()
    spec = stopping.StopSpec(spec.eos, spec.stops, spec.pad, include_stop)
    rows, T = toks.shape
    out, length, reason, index, live = stopping.new_state(rows, T, spec)
    start = torch.arange(rows) + 5
    for t in range(T):
        feed, pos = stopping.stop_update_reference(toks[:, t], t, spec, out, length, reason, index, live, start, None, True, limits)
        run = reason == 0
        assert torch.equal(feed, torch.where(run, toks[:, t], torch.full_like(feed, spec.pad)))
        assert torch.equal(pos, torch.where(run, start + t, torch.full_like(pos, -1)))  # a row cut by its limit is retired like any other
    o2, l2, r2, i2 = stopping.truncate_reference(toks, spec, limits)
    assert torch.equal(out, o2) and torch.equal(length, l2) and torch.equal(reason, r2) and torch.equal(index, i2)
    assert torch.equal(live, stopping.live_reference(toks, spec, limits))
    L = stopping.LIMIT
    assert reason.tolist() == [L, L, 1, L, 2, 2, L, L, 1, L, L, L]
    assert length.tolist()[:4] == [1, T, 4, 4] and length[4] == (4 if include_stop else 1) and length[6] == 6 and length[8] == T
    assert (index[reason == L] == -1).all()
    assert all((out[b, int(length[b]):] == spec.pad).all() for b in range(rows))
    # no limit: what it was
    assert all(torch.equal(a, b) for a, b in zip(stopping.truncate_reference(toks, spec), stopping.truncate_reference(toks, spec, None)))
    assert (stopping.truncate_reference(toks, spec)[2] != L).all()
    # a limit of 0 or less finishes the row at step 0 with length 1
    z = stopping.truncate_reference(toks, spec, torch.zeros(rows, dtype=torch.int32))
    assert (z[1] == 1).all() and (z[2] == L).all()


# ---- the new exports refuse before any launch ---------------------------------------------------------------------------------------
PTR, ODD = abi_table.PTR, abi_table.ODD
BAD_ARG = -1  # HYD_ERR_BAD_ARG
ARRAYS = ("temperature", "top_k", "top_p", "min_p", "repetition_penalty", "frequency_penalty", "presence_penalty", "seed")


def _no_device():
    if torch.cuda.is_available():
        pytest.skip("refusals are replayed on machines without a device only (an acceptance would launch on made-up addresses)")


def _rows_call(lib, kw, arrays):
    kw = dict(kw)
    null, no_dfa = kw.pop("null", False), kw.pop("no_dfa", False)
    c = abi_table.token_dfa(**{k[2:]: kw.pop(k) for k in list(kw) if k.startswith("c.")})
    p = None if null else C.byref(abi_table.sample_penalty(**kw))
    rc = lib.hyd_sample_tokens_rows(p, None if no_dfa else C.byref(c), *arrays, None)
    return {"rc": rc, "error": lib.hyd_last_error_string().decode() if rc else ""}


def test_sample_tokens_rows_refuses_what_the_wrapped_calls_refuse():
    """The recorded refusals of hyd_sample_tokens_constrained and hyd_sample_tokens_penalized (tests/golden/abi_table.json), replayed
    through hyd_sample_tokens_rows without arrays and with all eight: the same code and the same message, character for character."""
    _no_device()
    lib, table = _lib.load(), abi_table.load_fixture()
    cases = [c for c in abi_table.REFUSAL_CASES if c[1] in ("hyd_sample_tokens_constrained", "hyd_sample_tokens_penalized")]
    assert len(cases) > 40
    for cid, entry, kw in cases:
        kw = dict(kw, no_dfa=True) if entry == "hyd_sample_tokens_penalized" else kw
        for arrays in ([None] * 8, [PTR] * 8):
            assert _rows_call(lib, kw, arrays) == table[cid], (cid, arrays[0])


def test_sample_tokens_rows_refuses_null_params_and_misaligned_arrays():
    _no_device()
    lib = _lib.load()
    for arrays in ([None] * 8, [PTR] * 8):
        got = _rows_call(lib, dict(null=True), arrays)
        assert got["rc"] == BAD_ARG and "null params" in got["error"]
    for i, name in enumerate(ARRAYS):
        arrays = [None] * 8
        arrays[i] = PTR + (4 if name == "seed" else 2)  # (a seed aligned to 4 bytes only is refused too)
        for kw in (dict(), dict(no_dfa=True)):
            got = _rows_call(lib, kw, arrays)
            assert got["rc"] == BAD_ARG and name in got["error"] and "not aligned to its element size" in got["error"], (name, got)
    # rows == 0 succeeds without a launch, arrays or not
    assert _rows_call(lib, dict(rows=0), [PTR] * 8) == {"rc": 0, "error": ""}


def test_stop_update_rows_refuses_what_stop_update_refuses():
    _no_device()
    lib, table = _lib.load(), abi_table.load_fixture()
    cases = [c for c in abi_table.REFUSAL_CASES + abi_table.NOOP_CASES if c[1] == "hyd_stop_update"]
    assert len(cases) > 10
    for cid, _, kw in cases:
        kw = dict(kw)
        p = None if kw.pop("null", False) else C.byref(abi_table.stop(**kw))
        for max_len in (None, PTR):
            rc = lib.hyd_stop_update_rows(p, max_len, None)
            got = {"rc": rc, "error": lib.hyd_last_error_string().decode()} if rc else {"rc": rc}
            want = table[cid] if table[cid]["rc"] else {"rc": 0}
            assert got == want, (cid, max_len)
    rc = lib.hyd_stop_update_rows(C.byref(abi_table.stop()), ODD, None)
    assert rc == BAD_ARG and "max_len is not aligned to its element size" in lib.hyd_last_error_string().decode()


# ---- generate() on a tiny CPU model -----------------------------------------------------------------------------------------------
# (no attention kernel runs on the CPU: the model runs with disable_attention, which leaves embeddings, MLPs, the lm_head and the
# whole decode half of generate() -- what these tests are about; penalties need the levels' token sets, which that mode does not
# keep: their per-row form in generate() is tested on the GPU)
@pytest.fixture(scope="module")
def model():
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=64,
                      max_position_embeddings=128)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.float32, device="cpu", seed=0, std=0.3)
    for layer in m.model.layers:
        layer.self_attn.use_fused_decode = False
    m.setup_caches(max_unique_batch_size=8, max_unique_seq_length=24, max_shared_batch_sizes=[1, 4], max_shared_seq_lengths=[16, 16])
    return m


NEW = 6
LEAF_T = [0.0, 0.8, 0.0, 1.3]
LEAF_K = [None, 20, 5, None]
LEAF_MINP = [None, 0.02, None, 0.1]
LEAF_SEED = [11, 2 ** 63 + 5, 7, 2 ** 40]
LIMITS = [1, 6, 3, 5, 6, 2, 4, 4]


def _levels(perm=None):
    g = torch.Generator().manual_seed(6)
    ids = [torch.randint(0, 64, (1, 6), generator=g), torch.randint(0, 64, (4, 5), generator=g)]
    if perm is not None:
        ids[1] = ids[1][perm]
    return dict(input_ids=ids, num_return_sequences=2, max_new_tokens=NEW, disable_attention=True)


def _gen(model, torch_seed=3, **kw):
    torch.manual_seed(torch_seed)
    return model.generate(**dict(_levels(), **kw))


def test_generate_equal_rows_are_the_scalar_call(model):
    scalar = _gen(model, temperature=0.8, top_k=20, top_p=0.9, min_p=0.02)
    assert scalar.shape == (8, NEW)
    assert torch.equal(_gen(model, temperature=[0.8] * 4, top_k=[20] * 8, top_p=torch.tensor([0.9] * 4), min_p=[0.02] * 8), scalar)


def test_generate_greedy_rows_of_a_mixed_call(model):
    cuts = dict(top_k=LEAF_K, min_p=LEAF_MINP)
    mixed, greedy = _gen(model, temperature=LEAF_T, **cuts), _gen(model, temperature=0.0, **cuts)
    zero = torch.tensor([t == 0 for t in LEAF_T]).repeat_interleave(2)
    assert torch.equal(mixed[zero], greedy[zero]) and not torch.equal(mixed[~zero], greedy[~zero])


def test_generate_seeds_make_a_row_independent_of_its_place(model):
    cuts = dict(temperature=LEAF_T, top_k=LEAF_K, min_p=LEAF_MINP)
    seeded = _gen(model, seed=LEAF_SEED, **cuts)
    state = torch.random.get_rng_state()
    assert torch.equal(model.generate(**dict(_levels(), seed=LEAF_SEED, **cuts)), seeded)  # whatever torch drew before
    assert torch.equal(state, torch.random.get_rng_state())                                  # ... and nothing of it is drawn
    perm = [2, 0, 3, 1]
    permuted = model.generate(**dict(_levels(torch.tensor(perm)), seed=[LEAF_SEED[i] for i in perm],
                                     **{k: [v[i] for i in perm] for k, v in cuts.items()}))
    assert torch.equal(permuted, seeded[torch.tensor([2 * i + s for i in perm for s in (0, 1)])])
    per_row = model.generate(**dict(_levels(), seed=list(range(100, 108)), **cuts))
    assert not torch.equal(per_row[2::4], per_row[3::4])


def test_generate_per_row_limits(model):
    cuts = dict(temperature=LEAF_T, top_k=LEAF_K, min_p=LEAF_MINP, seed=LEAF_SEED)
    free = model.generate(**dict(_levels(), **cuts))
    out, fin = model.generate(**dict(_levels(), pad_token_id=63, return_finish=True, max_new_tokens=LIMITS, **cuts))
    lim = torch.tensor(LIMITS)
    assert out.shape == (8, max(LIMITS)) and torch.equal(fin.lengths.long(), lim)
    assert (fin.reasons == stopping.LIMIT).all() and (fin.stop_index == -1).all()
    before = torch.arange(NEW)[None, :] < lim[:, None]
    assert torch.equal(out, torch.where(before, free, torch.full_like(free, 63)))
    # one limit per prompt, repeated for its samples; a tensor is taken like a list
    out4, fin4 = model.generate(**dict(_levels(), pad_token_id=63, return_finish=True, max_new_tokens=torch.tensor([2, 6, 1, 3]), **cuts))
    assert fin4.lengths.tolist() == [2, 2, 6, 6, 1, 1, 3, 3] and torch.equal(out4[2:4], free[2:4])


def test_generate_refuses_per_row_arguments_it_cannot_honour(model):
    kw = _levels()
    for per_row in (dict(temperature=LEAF_T), dict(top_k=LEAF_K), dict(seed=LEAF_SEED), dict(max_new_tokens=[2, 6, 1, 3]),
                    dict(presence_penalty=[0.5, None, None, 0.1])):
        with pytest.raises(NotImplementedError, match="cannot be combined with draft_tokens or token_overrides"):
            model.generate(**dict(kw, **per_row), draft_tokens=2)
        with pytest.raises(NotImplementedError, match="cannot be combined with draft_tokens or token_overrides"):
            model.generate(**dict(kw, **per_row), token_overrides=torch.zeros((8, NEW), dtype=torch.long))
    with pytest.raises(ValueError, match=r"top_p 1.5 must be in \(0, 1\]"):
        model.generate(**kw, top_p=[0.9, 1.5, None, None])
    with pytest.raises(ValueError, match="temperature must be non-negative for every row"):
        model.generate(**kw, temperature=[0.5, -1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="max_new_tokens per row: integers >= 1"):
        model.generate(**dict(kw, max_new_tokens=[2, 0, 1, 3]))
    with pytest.raises(ValueError, match="holds 3 per-row values: 4 .* or 8"):
        model.generate(**kw, temperature=[0.5, 1.0, 0.0])
    with pytest.raises(ValueError, match="holds 5 per-row values"):
        model.generate(**kw, seed=[1, 2, 3, 4, 5])
