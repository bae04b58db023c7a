"""-m gpu: hyd_sample_tokens_penalized / hyd_token_bitmap_build (csrc/sample_penalty.hip) against the float64 definition of
the penalties (hydragen_amd/sampling.py) on the inputs of tests/penalty_cases.py (whose tie census runs without a GPU), and
generate(repetition_penalty / presence_penalty / frequency_penalty / logit_bias) on the tiny model."""
import math

import pytest
import torch

from hydragen_amd import layer_ops, sampling
from hydragen_amd.layer_ops import Penalties
from tests import penalty_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
SLACK = 1e-5  # tests/test_sampling_filters_gpu.py: the probability mass a boundary may sit from its threshold
GRID = [(20, None, None), (1, None, None), (None, 0.9, None), (None, 0.5, None), (None, None, 0.05), (50, 0.95, None),
        (None, 0.95, 0.01), (40, 0.8, 0.1), (1000, 0.99, None)]  # that file's cut combinations


def _dev(name):
    """The case on the GPU: (logits, Penalties with kernel-built bitmaps, the case)."""
    case = PC.build(name)
    n = case["logits"].shape[1]
    ctx = []
    for (ref, rpg), (ids, lens, _) in zip(case["context"], case["context_ids"]):
        bits = layer_ops.token_bitmap(ids.to(DEV), lens.to(DEV), n)
        assert torch.equal(bits.cpu(), ref)  # hyd_token_bitmap_build = its torch definition
        ctx.append((bits, rpg))
    pen = Penalties(case["r"], case["a"], case["f"], sampling.normalize_logit_bias(case["bias"], DEV), ctx,
                    None if case["gen"] is None else case["gen"].to(DEV), None if case["gen"] is None else case["gen_len"].to(DEV))
    return case["logits"].to(DEV), pen, case


def _x(logits, pen, rows=None):
    """The definition on the GPU, float64, for the given row indices (chunks keep the [rows, n] tables small)."""
    idx = torch.arange(logits.shape[0], device=DEV) if rows is None else rows
    out = []
    for s in range(0, idx.numel(), 128):
        i = idx[s : s + 128]
        ctx = [(bits[i // rpg], 1) for bits, rpg in pen.context]
        out.append(sampling.penalize_logits(logits[i], pen.repetition_penalty, pen.presence_penalty, pen.frequency_penalty,
                                            pen.logit_bias, ctx, None if pen.gen is None else pen.gen[i],
                                            None if pen.gen is None else pen.gen_len[i]))
    return torch.cat(out)


# ---- neutral penalties: the existing kernel, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("V, pad", [(1000, 0), (31997, 0), (32000, 24), (128256, 0)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_neutral_penalties_are_the_filtered_sampler_bit_for_bit(V, pad, dtype):
    g = torch.Generator(device=DEV).manual_seed(V + pad)
    x = (torch.randn(96, V + pad, device=DEV, generator=g) * 3.0).to(dtype)[:, :V]
    empty = Penalties(gen=torch.full((96, 8), 5, dtype=torch.int32, device=DEV), gen_len=torch.zeros(96, dtype=torch.int32, device=DEV))
    for T in (0.0, 0.9):
        for top_k, top_p, min_p in [(None, None, None)] + GRID:
            want = layer_ops.sample_tokens_filtered(x, T, key=(5, 8), top_k=top_k, top_p=top_p, min_p=min_p)
            for pen in (Penalties(), Penalties(1.0, 0.0, 0.0), empty):
                got = layer_ops.sample_tokens_penalized(x, T, key=(5, 8), penalties=pen, top_k=top_k, top_p=top_p, min_p=min_p)
                assert all(torch.equal(u, v) for u, v in zip(got, want)), (T, top_k, top_p, min_p)
    # the public operator takes the new entry point only when a penalty is on
    assert torch.equal(layer_ops.sample_tokens(x, 0.9, key=(5, 8), penalties=Penalties(1.0)), layer_ops.sample_tokens(x, 0.9, key=(5, 8)))


# ---- against the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_temperature_zero_bans_and_logprobs(name):
    logits, pen, _ = _dev(name)
    rows = logits.shape[0]
    x = _x(logits, pen)
    skip = PC.margin_rows(x)
    assert int(skip.sum()) <= 0.01 * rows  # (the census bounds it at 0.5 % without a GPU)
    tok, lp, kept = layer_ops.sample_tokens_penalized(logits, 0.0, key=(1, 0), penalties=pen)
    want = PC.greedy(x)
    assert torch.equal(tok[~skip, 0], want[~skip])
    assert (kept == (~torch.isnan(x) & (x > -math.inf)).sum(-1)).all()
    ref_lp = torch.log_softmax(x, -1)
    assert (lp.double() - ref_lp.gather(1, tok)[:, 0]).abs().max() < 1e-4
    # twice in a row: the same bits
    again = layer_ops.sample_tokens_penalized(logits, 0.0, key=(1, 0), penalties=pen)
    assert torch.equal(again[0], tok) and torch.equal(again[1], lp) and torch.equal(again[2], kept)
    # a hot draw: never a banned token, log-prob of the drawn token under the penalised distribution
    tok, lp, _ = layer_ops.sample_tokens_penalized(logits, 1.3, key=(9, 4), penalties=pen, top_p=0.95)
    assert (lp.double() - ref_lp.gather(1, tok)[:, 0]).abs().max() < 1e-4
    if pen.logit_bias is not None:
        banned = pen.logit_bias[0][pen.logit_bias[1] == -math.inf]
        assert banned.numel() and not torch.isin(tok, banned).any()
    # the same rows launched alone: the same tokens, counts and log-probs at temperature 0 (the noise is keyed by the row index)
    sub = torch.arange(rows, device=DEV)[rows // 3 :: max(rows // 5, 1)][:4]
    alone = Penalties(pen.repetition_penalty, pen.presence_penalty, pen.frequency_penalty, pen.logit_bias,
                      [(bits[sub // rpg].contiguous(), 1) for bits, rpg in pen.context],
                      None if pen.gen is None else pen.gen[sub].contiguous(), None if pen.gen is None else pen.gen_len[sub].contiguous())
    a = layer_ops.sample_tokens_penalized(logits[sub].contiguous(), 0.0, penalties=alone, top_k=50, top_p=0.9)
    b = layer_ops.sample_tokens_penalized(logits, 0.0, penalties=pen, top_k=50, top_p=0.9)
    assert all(torch.equal(u, v[sub]) for u, v in zip(a, b))


@pytest.mark.parametrize("name", ["bf16_128k_1024", "f16_odd_7", "f32_128k_7", "bf16_small_1024", "f32_wide_2", "bf16_32k_1024"])
def test_kept_counts_and_draws_against_the_definition(name):
    """Per case, as tests/test_sampling_filters_gpu.py does per parametrisation: exact counts on all but < 1 % of the (row, cut)
    pairs -- for the 7-row and 2-row cases (63 and 18 pairs) that is every pair."""
    allowed, total = _kept_case(name)
    print(f"{name}: {allowed} of {total} (row, cut) pairs differ from the exact float64 count")
    assert allowed < 0.01 * total


def _kept_case(name):
    logits, pen, _ = _dev(name)
    rows = torch.arange(logits.shape[0], device=DEV)[:: max(logits.shape[0] // 64, 1)][:64]
    x = _x(logits, pen, rows)
    allowed = 0
    for top_k, top_p, min_p in GRID:
        tok, _, kept = layer_ops.sample_tokens_penalized(logits, 1.5, key=(5, 0), penalties=pen, top_k=top_k, top_p=top_p, min_p=min_p)
        tok, kept = tok[rows], kept[rows].long()
        tp_lo = None if top_p is None else max(top_p - SLACK, 1e-6)
        tp_hi = None if top_p is None else min(top_p + SLACK, 1.0)
        mp_lo = None if min_p is None else min(min_p + SLACK, 1.0)
        mp_hi = None if min_p is None else max(min_p - SLACK, 0.0)
        lo, exact = sampling.kept_mask(x, top_k, tp_lo, mp_lo).sum(-1), sampling.kept_mask(x, top_k, top_p, min_p).sum(-1)
        loose = sampling.kept_mask(x, top_k, tp_hi, mp_hi)
        assert ((kept >= lo) & (kept <= loose.sum(-1))).all(), (top_k, top_p, min_p, kept, exact)
        assert loose.gather(1, tok).all()  # no draw outside the (loosened) kept set
        allowed += int((kept != exact).sum())
    return allowed, len(GRID) * rows.numel()


def test_draws_follow_the_penalised_softmax():
    g = torch.Generator(device=DEV).manual_seed(2)
    row = torch.randn(64, device=DEV, generator=g) * 1.5
    R = 16384
    x = row[None].repeat(R, 1)
    top = torch.topk(row, 6).indices
    ctx = [(layer_ops.token_bitmap(top[:2][None], None, 64), R)]
    gen = torch.stack([top[2], top[2], top[3], top[0]]).to(torch.int32)[None].repeat(R, 1).contiguous()
    pen = Penalties(1.6, 0.4, 0.3, sampling.normalize_logit_bias({int(top[4]): -math.inf, int(top[5]): 0.8, 7: -0.5}, DEV), ctx,
                    gen, torch.full((R,), 4, dtype=torch.int32, device=DEV))
    T, top_k, top_p = 0.8, 20, 0.8
    tok, _, kept = layer_ops.sample_tokens_penalized(x, T, key=(2024, 0), penalties=pen, top_k=top_k, top_p=top_p)
    xd = _x(x[:1], Penalties(pen.repetition_penalty, pen.presence_penalty, pen.frequency_penalty, pen.logit_bias,
                              [(ctx[0][0], 1)], gen[:1], pen.gen_len[:1]))
    keep = sampling.kept_mask(xd, top_k, top_p)[0]
    assert (kept == int(keep.sum())).all() and int(keep.sum()) > 2
    want = torch.softmax(torch.where(keep, xd[0] / T, torch.tensor(-math.inf, device=DEV, dtype=torch.float64)), -1)
    freq = torch.bincount(tok[:, 0], minlength=64).double() / R
    assert 0.5 * (freq - want).abs().sum() <= 0.02
    assert freq[int(top[4])] == 0


def test_every_token_banned_and_groups_and_append():
    n = 512
    g = torch.Generator(device=DEV).manual_seed(4)
    x = (torch.randn(1, n, device=DEV, generator=g) * 2).to(torch.bfloat16).repeat(8, 1)
    ban_all = sampling.normalize_logit_bias((torch.arange(n), torch.full((n,), -math.inf)), DEV)
    for T in (0.0, 1.0):
        tok, lp, kept = layer_ops.sample_tokens_penalized(x, T, penalties=Penalties(logit_bias=ban_all))
        assert (tok == 0).all() and (kept == 0).all() and torch.isnan(lp).all()
    # rows of different groups read their own group's bitmap
    best = int(x[0].float().argmax())
    ids = torch.tensor([[best, (best + 4) % n, (best + 5) % n], [(best + 1) % n, (best + 2) % n, (best + 3) % n]], device=DEV)
    pen = Penalties(50.0, context=[(layer_ops.token_bitmap(ids, None, n), 4)])
    tok = layer_ops.sample_tokens_penalized(x, 0.0, penalties=pen)[0][:, 0]
    assert (tok[:4] != best).all() and (tok[4:] == best).all()
    # append_out: the kernel keeps the list of generated tokens; at the stride the length still counts, nothing is written
    pen = Penalties(frequency_penalty=1000.0, gen=torch.full((8, 3), -1, dtype=torch.int32, device=DEV),
                    gen_len=torch.zeros(8, dtype=torch.int32, device=DEV), append=True)
    toks = [layer_ops.sample_tokens(x, 0.0, penalties=pen) for _ in range(4)]
    assert pen.gen_len.tolist() == [4] * 8 and torch.equal(pen.gen.long(), torch.cat(toks[:3], 1))
    assert torch.equal(x[0].float()[torch.cat(toks, 1)[0]], torch.topk(x[0].float(), 4).values)  # no repeats: the next best each time
    # Penalties.push (the torch route's append) writes what the kernel writes
    pen2 = Penalties(frequency_penalty=1000.0, gen=torch.full((8, 3), -1, dtype=torch.int32, device=DEV),
                     gen_len=torch.zeros(8, dtype=torch.int32, device=DEV))
    for t in toks:
        pen2.push(t)
    assert torch.equal(pen2.gen, pen.gen) and torch.equal(pen2.gen_len, pen.gen_len)


# ---- the model shell -------------------------------------------------------------------------------------------------------
def _model(dtype=torch.bfloat16, seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=DEV, seed=seed, std=0.05)


def _setup(model, batch=8):
    model.setup_caches(max_unique_batch_size=batch, max_unique_seq_length=48, max_shared_batch_sizes=[1, 2],
                       max_shared_seq_lengths=[256, 40])


def test_generate_neutral_arguments_change_nothing():
    model = _model()
    _setup(model)
    prompt = torch.randint(1, 512, (1, 40), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    for graph in (False, True):
        model.graph(graph)
        res = []
        for extra in (dict(), dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias={})):
            torch.manual_seed(77)
            res.append(model.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=8, temperature=0.9, top_p=0.9,
                                      return_logits=True, return_logprobs=True, **extra))
            offset = torch.cuda.default_generators[0].get_offset()
            res[-1] = res[-1] + (offset,)
        (o0, l0, p0, off0), (o1, l1, p1, off1) = res
        assert torch.equal(o0, o1) and torch.equal(p0, p1) and all(torch.equal(a, b) for a, b in zip(l0, l1)) and off0 == off1
    model.graph(False)


def test_generate_frequency_penalty_and_bans():
    model = _model()
    _setup(model)
    prompt = torch.randint(1, 512, (1, 40), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    kw = dict(input_ids=prompt, num_return_sequences=8, max_new_tokens=24, temperature=0.0)
    plain = model.generate(**kw)
    # fp32 logits of a 16-bit model stay far below 1e4 in magnitude: a generated token cannot come back
    out = model.generate(frequency_penalty=1e4, **kw)
    assert all(len(set(r)) == len(r) for r in out.tolist())
    # ban the greedy tokens of the unpenalised run: other tokens come, a banned id never (first token: the fan-out torch path)
    banned = plain.unique()
    for T in (0.0, 1.0):
        out = model.generate(logit_bias={int(t): -math.inf for t in banned}, **{**kw, "temperature": T})
        assert not torch.isin(out, banned).any()
    ids, vals = banned, torch.full((banned.numel(),), -math.inf)
    assert torch.equal(model.generate(logit_bias=(ids, vals), **kw), model.generate(logit_bias={int(t): -math.inf for t in banned}, **kw))
    with pytest.raises(ValueError):
        model.generate(repetition_penalty=0.0, **kw)
    with pytest.raises(ValueError):
        model.generate(logit_bias={512: 1.0}, **kw)


def test_generate_fused_and_torch_routes_agree_and_logprobs():
    model = _model()
    _setup(model)
    g = torch.Generator(device=DEV).manual_seed(10)
    shared = torch.randint(1, 512, (1, 40), device=DEV, generator=g)
    unique = torch.randint(1, 512, (8, 6), device=DEV, generator=g)
    lens = torch.tensor([6, 3, 4, 6, 1, 2, 5, 6], device=DEV)
    over = torch.randint(1, 40, (8, 12), device=DEV, generator=g)  # a small range: repeats
    pens = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15, logit_bias={3: -math.inf, 9: 1.5})
    kw = dict(input_ids=[shared, unique], seq_lens=[torch.tensor([40], device=DEV), lens], max_new_tokens=12, temperature=0.0,
              token_overrides=over, return_logits=True, return_logprobs=True, top_logprobs=3, **pens)
    res = {}
    for fused in (True, False):
        model.fused_sampling_penalties = fused
        res[fused] = model.generate(**kw)
    model.fused_sampling_penalties = True
    (o1, l1, p1, ti1, tl1), (o0, l0, p0, ti0, tl0) = res[True], res[False]
    assert all(torch.equal(a, b) for a, b in zip(l1, l0))  # the overrides feed both runs: identical logits
    ctx = [(layer_ops.token_bitmap(shared, None, 512), 8), (layer_ops.token_bitmap(unique, lens, 512), 1)]
    bias = sampling.normalize_logit_bias(pens["logit_bias"], DEV)
    skipped = 0
    for j, lg in enumerate(l1):
        x = sampling.penalize_logits(lg, 1.3, 0.4, 0.15, bias, ctx, over[:, :j].to(torch.int32),
                                     torch.full((8,), j, dtype=torch.int32, device=DEV))
        skip = PC.margin_rows(x)
        skipped += int(skip.sum())
        assert torch.equal(o1[~skip, j], o0[~skip, j]) and torch.equal(o1[~skip, j], PC.greedy(x)[~skip])
        want = torch.log_softmax(x, -1).gather(1, o1[:, j : j + 1])[:, 0]
        assert (p1[:, j].double() - want).abs().max() < 1e-4  # the PENALISED distribution
        # top_logprobs reports the model's raw distribution (hyd_token_logprobs on the unpenalised logits)
        raw = torch.log_softmax(lg.double(), -1)
        assert (tl1[:, j].double() - raw.gather(1, ti1[:, j])).abs().max() < 1e-4
    assert skipped <= 0.01 * o1.numel()
    assert not (o1 == 3).any() and ti1.shape == tl1.shape == (8, 12, 3)


def test_generate_extend_keeps_the_first_calls_prompt_in_the_context():
    model = _model()
    _setup(model)
    g = torch.Generator(device=DEV).manual_seed(11)
    p0 = torch.arange(0, 256, device=DEV)[None]  # the lower half of the vocabulary, kept as level 0 by the first call
    p1 = torch.randint(256, 512, (2, 30), device=DEV, generator=g)
    model.generate(input_ids=p0, num_return_sequences=2, max_new_tokens=2, temperature=0.0, shared_cache_op="extend")
    assert len(model.shared_bitmaps) == model.get_num_used_shared_caches() == 1
    kw = dict(input_ids=p1, num_return_sequences=4, max_new_tokens=10, temperature=0.0, shared_cache_op="preserve")
    plain = model.generate(**kw)
    out, logits = model.generate(repetition_penalty=1e4, return_logits=True, **kw)
    assert len(model.shared_bitmaps) == 1
    assert (plain < 256).any()  # (otherwise the next line shows nothing)
    # every positive logit of a context token is divided by 1e4: no token of EITHER call's prompt while another is positive
    for j, lg in enumerate(logits):
        ctx = [(model.shared_bitmaps[0], 8), (layer_ops.token_bitmap(p1, None, 512), 4)]
        gen = out[:, :j].to(torch.int32)
        x = sampling.penalize_logits(lg, 1e4, context=ctx, gen=gen, gen_len=torch.full((8,), j, dtype=torch.int32, device=DEV))
        skip = PC.margin_rows(x)
        assert torch.equal(out[~skip, j], PC.greedy(x)[~skip])
    assert (out >= 256).all()
    model.empty_shared_cache()
    assert model.shared_bitmaps == []
