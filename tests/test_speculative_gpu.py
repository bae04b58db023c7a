"""-m gpu: speculative decoding on the MI355X.  The causal-tail suffix kernels (both of them, through hyd_suffix_attn_causal_fwd and
hyd_decode_attn_fused with causal_tail = 1) against a float64 dense softmax, hyd_rope_append_multi against exact float64 arithmetic,
hyd_draft_lookup / hyd_draft_accept against their torch definitions (exactly), and generate(draft_tokens=) against plain decoding."""
import math

import numpy as np
import pytest
import torch

from hydragen_amd import speculative
from hydragen_amd.attention import hydragen_attention
from hydragen_amd.flash import flash_attention_seqlen
from hydragen_amd.speculative import Segment
from tests import glue_ref
from tests.gpu_util import TORCH_DT, assert_close, assert_close_l2
from tests.test_speculative import dense_causal_tail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the causal-tail kernels against the float64 reference --------------------------------------------------------------------
# Lengths at which a row's limit falls on, just before and just after a 32-key tile (the matrix-core kernel) and a 4- or 8-key wave
# instruction (the dot-product kernel); every one >= T, plus one retired row of length 0.
def _lengths(T, case):
    pool = [n for n in (T, T + 1, 31, 32, 33, 63, 64, 65, 129) if n >= T]
    return [pool[(case * 3 + j) % len(pool)] for j in range(3)] + [0]


_REF = {}


def _attn_case(dt, T, Hq, Hkv, D, S, case):
    """Inputs on the device and the float64 references (no level, one level, two levels), computed once per case."""
    key = (dt, T, Hq, Hkv, D, S, case)
    if key not in _REF:
        g = torch.Generator().manual_seed(1000 * T + 10 * Hq + Hkv + D + S + case)
        B = 4
        rnd = lambda *s: torch.randn(*s, generator=g).to(TORCH_DT[dt])  # noqa: E731  (unit-normal, zero mean: as every attention test)
        q, k, v = rnd(B, T, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
        levels = [(rnd(1, 40, Hkv, D), rnd(1, 40, Hkv, D)), (rnd(2, 24, Hkv, D), rnd(2, 24, Hkv, D))]
        lens = torch.tensor([min(n, S) for n in _lengths(T, case)], dtype=torch.int32)
        f64 = lambda t: t.double()  # noqa: E731
        want = [dense_causal_tail(f64(q), f64(k), f64(v), lens, [(f64(a), f64(b)) for a, b in levels[:n]]) for n in range(3)]
        _REF.clear()  # (one case at a time: the parametrisation below keeps a case's tests together)
        _REF[key] = (q.to(DEV), k.to(DEV), v.to(DEV), [(a.to(DEV), b.to(DEV)) for a, b in levels], lens.to(DEV), want)
    return _REF[key]


def _fused(q, k, v, levels, lens, causal):
    n = len(levels)
    return hydragen_attention(q, k, v, [a for a, _ in levels], [b for _, b in levels], [None] * n, [None] * n, [False] * n, lens, causal_tail=causal)


# (4, 4) with T = 2: units of 2 rows -> the one-unit-per-wave kernel; everything else has >= 3 rows -> the matrix-core kernel.
# (6, 2): g = 3, a 16-row chunk boundary falls inside a token at T = 8.  S = 132: few units, four waves per unit; S = 40: one wave per
# unit, 1 / 2 / 4 kv heads per workgroup.
CASES = [(dt, T, hq, hkv, D, S) for dt in ("f16", "bf16") for T in (2, 3, 5, 8) for hq, hkv in ((4, 4), (8, 2), (8, 1), (6, 2))
         for D in (64, 128) for S in (132, 40)]
# Head dim 256.  S = 132 (few units): the one-unit-per-wave kernel with four waves per unit -- 4/4 heads, T = 2 / 3: units of 2 / 3 rows,
# R = 2 / 4; 8/2 heads, T = 3: 12 rows, R = 8 in two chunks.  S = 40: 4/4 heads, T = 2: R = 2 with one wave per unit; units of >= 3 rows:
# the matrix-core kernel, one wave per unit, 2 (8/2 heads) and 1 (8/1) kv heads per workgroup.
CASES += [(dt, T, hq, hkv, 256, S) for dt in ("f16", "bf16")
          for T, hq, hkv, S in ((2, 4, 4, 132), (3, 4, 4, 132), (3, 8, 2, 132), (2, 4, 4, 40), (3, 8, 2, 40), (5, 8, 1, 40))]


@pytest.mark.parametrize("dt, T, Hq, Hkv, D, S", CASES)
def test_causal_tail_kernels_equal_the_dense_reference(dt, T, Hq, Hkv, D, S):
    case = CASES.index((dt, T, Hq, Hkv, D, S))
    q, k, v, levels, lens, want = _attn_case(dt, T, Hq, Hkv, D, S, case)
    live = (lens > 0).cpu()
    what = f"{dt} T={T} heads {Hq}/{Hkv} D={D} S={S} lens {lens.tolist()}"
    # the suffix pass alone (a retired row has no key at all: zeros)
    got, lse = flash_attention_seqlen(q, k, v, lens, causal_tail=True)
    torch.cuda.synchronize()
    assert_close(got.cpu().double()[live].numpy(), want[0][live].numpy(), dt, "suffix " + what)
    assert not got[~live.to(DEV)].any() and bool(torch.isinf(lse[~live.to(DEV)]).all())
    # ... and its LSE: log of the sum over the visible unique keys
    kk = k.double().cpu().repeat_interleave(Hq // Hkv, 2)
    s = torch.einsum("bthd,bshd->bths", q.double().cpu(), kk) / math.sqrt(D)
    lim = lens.cpu().long()[:, None] - (T - 1 - torch.arange(T))[None, :]
    s = s.masked_fill(torch.arange(S)[None, None, None, :] >= lim[:, :, None, None], float("-inf"))
    want_lse = torch.logsumexp(s, -1)
    assert float((lse.cpu().double()[live] - want_lse[live]).abs().max()) <= 2e-2, "lse " + what
    # the same call WITHOUT the flag is another function: a kernel that ignores the flag cannot pass
    plain, _ = flash_attention_seqlen(q, k, v, lens)
    with pytest.raises(AssertionError):
        assert_close(plain.cpu().double()[live].numpy(), want[0][live].numpy(), dt)
    # the whole operator with one and two shared levels (every row sees every shared key; the retired row only those).  Held to
    # assert_close_l2 -- the same maximum absolute error, and the relative L2 error for both dtypes -- as the suite's other tests of
    # merged partials on small tensors are (test_suffix_partials_gpu.py, test_token_row_gpu.py): assert_close's third figure, the
    # MEAN element-wise relative difference, is dominated by outputs near zero on tensors of a few thousand elements (gpu_util),
    # and the operator rounds each level's partial to 16 bits before the merge.  Measured on these 6144-element tensors, bf16: the
    # operator WITHOUT the flag against its own float64 reference reads 7.3e-3 .. 9.5e-3 of that figure's 1e-2, the causal calls
    # 7.2e-3 .. 1.1e-2 (4 of 130 cases above 1e-2), with max abs 2-5e-3 against bounds of 8-11e-3 and relative L2 2.0-2.7e-3
    # against 4e-3 in both forms.
    for n in (1, 2):
        got = _fused(q, k, v, levels[:n], lens, True)
        torch.cuda.synchronize()
        assert_close_l2(got.cpu().double().numpy(), want[n].numpy(), dt, f"fused, {n} level(s) " + what)
        assembled = speculative.assembled_causal_tail_attention(q, k, v, lens, [a for a, _ in levels[:n]], [b for _, b in levels[:n]])
        torch.cuda.synchronize()  # the definition the model shell falls back on, from the launches that existed before
        assert_close_l2(assembled.cpu().double().numpy(), want[n].numpy(), dt, f"assembled, {n} level(s) " + what)
    plain = _fused(q, k, v, levels[:1], lens, False)
    with pytest.raises(AssertionError):
        assert_close_l2(plain.cpu().double()[live].numpy(), want[1][live].numpy(), dt)


@pytest.mark.parametrize("nq", [1, 3])
def test_without_the_flag_the_operator_is_the_existing_suffix_pass_bit_for_bit(nq):
    """causal_tail = 0 changes nothing: hyd_decode_attn_fused without levels is hyd_suffix_attn_fwd on the same arguments, as before."""
    g = torch.Generator(device=DEV).manual_seed(nq)
    for dt, (Hq, Hkv), D in ((torch.bfloat16, (8, 2), 128), (torch.float16, (4, 4), 64)):
        q = torch.randn(5, nq, Hq, D, device=DEV, dtype=dt, generator=g)
        k, v = (torch.randn(5, 70, Hkv, D, device=DEV, dtype=dt, generator=g) for _ in range(2))
        lens = torch.tensor([70, 1, 33, 0, 64], device=DEV, dtype=torch.int32)
        a = hydragen_attention(q, k, v, [], [], [], [], [], lens)
        b, _ = flash_attention_seqlen(q, k, v, lens)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_causal_tail_is_never_silently_non_causal():
    q = torch.zeros(2, 3, 4, 64, device=DEV, dtype=torch.bfloat16)
    k = torch.zeros(2, 16, 4, 64, device=DEV, dtype=torch.bfloat16)
    lens = torch.tensor([16, 8], device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="2 to 8"):
        flash_attention_seqlen(q[:, :1], k, k, lens, causal_tail=True)
    with pytest.raises(NotImplementedError, match="causal_tail"):
        flash_attention_seqlen(q, k.to(torch.float8_e4m3fn), k.to(torch.float8_e4m3fn), lens, causal_tail=True)
    with pytest.raises(NotImplementedError, match="causal_tail"):
        flash_attention_seqlen(q[..., :48], k[..., :48], k[..., :48], lens, causal_tail=True)
    with pytest.raises(NotImplementedError, match="causal_tail"):
        hydragen_attention(q, k, k, [], [], [], [], [], None, causal_tail=True)


# ---- hyd_rope_append_multi against exact float64 arithmetic ---------------------------------------------------------------------
def _rope_append_multi_exact(dtype, T, D, fused=False, table_end=False):
    """fused: q / k / v are views into one [B, T, (Hq + 2 Hkv) D] projection buffer (token stride (Hq + 2 Hkv) D, heads contiguous).
    table_end: a fifth row whose later tokens' positions reach and pass max_pos -- they take the table's last row (the header:
    positions are clamped to it) and are written all the same."""
    from hydragen_amd.fused_decode import rope_append_multi

    B, Hq, Hkv, cache_len, G = 5 if table_end else 4, 8, 2, 12, glue_ref.GUARD
    cos, sin = glue_ref.exact_tables(D)
    q, k, v = (x.reshape(B, T, -1, D) for x in glue_ref.exact_inputs(B * T, Hq, Hkv, D))
    shared = np.array([3, 7, 5, 0], dtype=np.int64)
    # row 1: position shared_len - 1 (retired); row 2: its last tokens (1 of 2, 3 of 8) fall past the cache
    idx0 = np.array([0, -1, cache_len - T + min(3, T - 1), 2], dtype=np.int64)
    if table_end:  # row 4: first position max_pos - 2 at cache index 3 -- tokens 2 .. T - 1 are at max_pos and beyond
        shared, idx0 = np.append(shared, glue_ref.EXACT_MAX_POS - 5), np.append(idx0, 3)
    pos0 = shared + idx0
    pos = pos0[:, None] + np.arange(T)[None, :]
    assert pos[:4].max() < glue_ref.EXACT_MAX_POS and (not table_end or (pos[4, 1] == glue_ref.EXACT_MAX_POS - 1 and pos[4, 2] == glue_ref.EXACT_MAX_POS))
    rows = np.clip(pos, 0, glue_ref.EXACT_MAX_POS - 1).reshape(-1)
    want_q = glue_ref.to_dtype_exact(glue_ref.rope_ref64(q.reshape(B * T, Hq, D), cos[rows], sin[rows]), dtype).reshape(B, T, Hq, D)
    want_k = glue_ref.to_dtype_exact(glue_ref.rope_ref64(k.reshape(B * T, Hkv, D), cos[rows], sin[rows]), dtype).reshape(B, T, Hkv, D)
    tq, tk, tv = (glue_ref.to_dtype_exact(x, dtype) for x in (q, k, v))
    # caches with guard tokens behind every sequence and a guard sequence behind the batch, all sentinels
    kbuf = glue_ref.sentinel16((B + 1, cache_len + G, Hkv, D), dtype, 1)
    vbuf = glue_ref.sentinel16((B + 1, cache_len + G, Hkv, D), dtype, 2)
    dk, dv = kbuf.to(DEV), vbuf.to(DEV)
    dq, dkk, dvv = tq.to(DEV), tk.to(DEV), tv.to(DEV)
    if fused:
        buf = torch.cat([x.reshape(B, T, -1) for x in (dq, dkk, dvv)], -1)
        dq, dkk, dvv = (x.unflatten(-1, (-1, D)) for x in buf.split([Hq * D, Hkv * D, Hkv * D], -1))
        assert dq.stride(1) == (Hq + 2 * Hkv) * D and not dkk.is_contiguous() and dvv.data_ptr() == buf.data_ptr() + 2 * (Hq + Hkv) * D
    q_out, sl = rope_append_multi(dq, dkk, dvv, torch.from_numpy(cos).to(DEV), torch.from_numpy(sin).to(DEV),
                                  torch.from_numpy(pos0).to(DEV), torch.from_numpy(shared).to(DEV), dk[:B, :cache_len], dv[:B, :cache_len])
    torch.cuda.synchronize()
    bits = glue_ref.bits
    assert torch.equal(bits(q_out.cpu()), bits(want_q))
    assert sl.tolist() == [int(i + T) if i >= 0 else 0 for i in idx0]
    exp_k, exp_v = kbuf.clone(), vbuf.clone()
    for b in range(B):
        for i in range(T):
            j = idx0[b] + i
            if idx0[b] >= 0 and j < cache_len:
                exp_k[b, j], exp_v[b, j] = want_k[b, i], tv[b, i]
    assert torch.equal(bits(dk.cpu()), bits(exp_k)), "K: written rows hold the rotated keys, every other byte (guards, the retired row) is untouched"
    assert torch.equal(bits(dv.cpu()), bits(exp_v)), "V likewise"
    assert not torch.equal(bits(exp_k[2, cache_len - 1]), bits(kbuf[2, cache_len - 1])) and torch.equal(bits(exp_k[1]), bits(kbuf[1]))
    if table_end:  # the tokens past the table were rotated by its LAST row, not by their predecessor's and not skipped
        last = np.array([glue_ref.EXACT_MAX_POS - 1])
        for i in range(2, T):
            alone = glue_ref.to_dtype_exact(glue_ref.rope_ref64(k[4, i][None], cos[last], sin[last]), dtype)[0]
            assert torch.equal(bits(dk.cpu()[4, 3 + i]), bits(alone)) and not torch.equal(bits(alone), bits(tk[4, i]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T", [2, 8])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_rope_append_multi_exact(dtype, T, D):
    _rope_append_multi_exact(dtype, T, D)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T, D, fused, table_end", [(3, 128, True, False), (8, 256, True, True), (3, 64, False, True)])
def test_rope_append_multi_on_fused_views_and_at_the_end_of_the_tables(dtype, T, D, fused, table_end):
    _rope_append_multi_exact(dtype, T, D, fused, table_end)


# ---- hyd_draft_lookup and hyd_draft_accept: exactly their definitions ----------------------------------------------------------
def _to(segs, dev):
    return [Segment(s.ids.to(dev), None if s.lens is None else s.lens.to(dev)) for s in segs]


def test_draft_lookup_on_the_hand_written_cases():
    seqs = [[1, 2, 3, 9, 8, 7, 3, 5, 6, 1, 2, 3], [4, 5, 1, 1, 1, 4, 5, 2, 2, 2, 4, 5], [7, 8, 9], [5, 5], [3], [1, 2, 6, 1, 2], [1, 2, 1, 2], [2, 2]]
    width = max(map(len, seqs))
    ids = torch.tensor([s + [0] * (width - len(s)) for s in seqs])
    lens = torch.tensor([len(s) for s in seqs])
    for k in (1, 3, 7):
        for ng in ((1, 3), (2, 2), (1, 1), (2, 8)):
            seg = [Segment(ids, lens)]
            want = speculative.prompt_lookup_reference(seg, len(seqs), k, ng)
            got = speculative.draft_lookup(_to(seg, DEV), len(seqs), k, ng)
            assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (k, ng)
    empty = [Segment(torch.zeros((1, 0), dtype=torch.int64)), Segment(torch.tensor([[3, 3, 3]]), torch.tensor([0]))]
    got = speculative.draft_lookup(_to(empty, DEV), 2, 2)
    assert got[0].tolist() == [[0, 0], [0, 0]] and got[1].tolist() == [0, 0]


@pytest.mark.parametrize("K", [1, 4, 7])
def test_draft_lookup_random_small_vocabulary(K):
    """16 token ids, so n-grams repeat: two levels (one sequence; four, ragged), ragged prompts, ragged generated tails; B = 8."""
    g = torch.Generator().manual_seed(K)
    B, total = 8, 0
    for trial in range(6):
        rnd = lambda r, w: torch.randint(0, 16, (r, w), generator=g)  # noqa: E731
        segs = [Segment(rnd(1, 37)), Segment(rnd(4, 21), torch.randint(0, 22, (4,), generator=g)),
                Segment(rnd(8, 9), torch.randint(0, 10, (8,), generator=g).int()), Segment(rnd(8, 70), torch.randint(0, 71, (8,), generator=g).int())]
        ng = [(1, 3), (2, 4), (1, 1), (3, 3), (1, 8), (2, 2)][trial]
        want = speculative.prompt_lookup_reference(segs, B, K, ng)
        wide = torch.full((B, K + 1), -5, dtype=torch.int64, device=DEV)  # the drafts go straight into columns 1.. of the next input
        got = speculative.draft_lookup(_to(segs, DEV), B, K, ng, out=wide[:, 1:])
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (trial, ng)
        assert torch.equal(wide[:, 1:].cpu(), want[0]) and bool((wide[:, 0] == -5).all())
        total += int(want[1].sum())
    assert total > 0  # (some trial proposed something)


@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("rows", [6, 130])
def test_draft_accept_equals_the_definition_over_a_generation(K, rows):
    """Random drafts that agree with the draws about two times in three, EOS ids that occur, several steps to the end: the device state
    and the hand-backs equal accept_reference's after every step."""
    g = torch.Generator().manual_seed(10 * K + rows)
    T, mx, pad, eos = K + 1, 19, 15, (3, 11)
    start = torch.arange(rows) * 5 + 40
    shared = torch.arange(rows) % 4 + 30
    for retire, with_lp in ((True, True), (False, False)):
        cpu = speculative.new_state(rows, mx, pad, None, with_lp)
        dev = speculative.new_state(rows, mx, pad, DEV, with_lp)
        live = torch.zeros((mx,), dtype=torch.int32, device=DEV)
        for step in range(mx):
            t = 1 if step == 0 else T
            sampled = torch.randint(0, 14, (rows, t), generator=g)
            sampled[torch.rand(rows, t, generator=g) < 0.03] = 11
            fed = torch.randint(0, 14, (rows, t), generator=g)
            agree = torch.rand(rows, t, generator=g) < 0.66
            fed[:, 1:] = torch.where(agree[:, 1:], sampled[:, :-1], fed[:, 1:])
            lp = -torch.rand(rows, t, generator=g) if with_lp else None
            want = speculative.accept_reference(fed, sampled, *cpu[:4], start, shared, eos, pad, mx, retire, lp, cpu[4])
            got = speculative.draft_accept(fed.to(DEV), sampled.to(DEV), *dev[:4], live[step : step + 1], start.to(DEV), shared.to(DEV), eos, pad, mx,
                                           retire, None if lp is None else lp.to(DEV), dev[4])
            for a, b, name in zip(got, want[:3], ("feed", "next_pos", "accepted")):
                assert torch.equal(a.cpu(), b), (name, step)
            assert int(live[step]) == want[3]
            for a, b, name in zip(dev, cpu, ("out", "length", "reason", "stop_index", "logprobs")):
                assert (a is None and b is None) or torch.equal(a.cpu(), b), (name, step)
        if rows > 64:  # (enough rows that both ends occur: some run to max_new_tokens, some stop at an EOS id)
            assert int(cpu[1].max()) == mx and int((cpu[2] == 1).sum()) > 0


# ---- end to end: generate(draft_tokens=) against plain decoding ---------------------------------------------------------------
# The largest |plain decode logits - float64 reference model| over THIS test's models and prompts, measured on the commit before
# the feature (profiles/speculative.md records the run), and twice that as the top-2 gap below which a row is compared no further:
# a two-sided error on two logits.
LOGIT_ERR = 0.008  # measured 0.00394 (4/4 heads) and 0.00795 (8/2): the larger, rounded up
GAP = 2 * LOGIT_ERR
NEW, PROMPT = 24, 48
# fp16 models (hidden = heads x 64: 256 for 4/4 heads, 512 for 8/2).  Seed of the weights and the prompts per head geometry, searched
# on the CPU with the float64 model below (seeds 0 .. 399): the ones whose greedy decode keeps the largest smallest top-2 gap --
# 0.0336 (4/4) and 0.0531 (8/2), above GAP, so that no row is cut short.  A bf16 model is out of reach for this comparison: its
# measured logit error is 0.039 / 0.065, and no seed in 400 keeps every top-2 gap of 48 decisions above 0.13.
SEEDS = {(4, 4): 115, (8, 2): 81}


def cpu_model(heads, kv_heads, seed):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=heads * 64, intermediate_size=512, num_hidden_layers=2, num_attention_heads=heads,
                      num_key_value_heads=kv_heads, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.float16, device="cpu", seed=seed, std=0.05)


def cpu_prompts(seed):
    return torch.randint(1, 512, (2, PROMPT), generator=torch.Generator().manual_seed(seed))


@torch.no_grad()
def ref_logits64(model, ids):
    """float64 causal transformer over full sequences ids [b, n] with the model's weights, on the CPU (the glue references'
    definitions: RMSNorm with fp32-valued eps, rotate-half RoPE on the model's own fp32 tables, SwiGLU)."""
    from hydragen_amd.llama import rotate_half

    cfg = model.config
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    D = cfg.hidden_size // H
    f = lambda t: t.detach().cpu().double()  # noqa: E731
    ids = ids.cpu()
    b, n = ids.shape
    h = f(model.model.embed_tokens.weight)[ids]
    cos = f(model.model.rotary_emb.cos_cached)[:n][None, :, None, :]
    sin = f(model.model.rotary_emb.sin_cached)[:n][None, :, None, :]
    eps = float(np.float32(cfg.rms_norm_eps))
    norm = lambda x, w: f(w) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))  # noqa: E731
    for layer in model.model.layers:
        a, m = layer.self_attn, layer.mlp
        x = norm(h, layer.input_layernorm.weight)
        q = (x @ f(a.q_proj.weight).T).view(b, n, H, D)
        k = (x @ f(a.k_proj.weight).T).view(b, n, Hkv, D)
        v = (x @ f(a.v_proj.weight).T).view(b, n, Hkv, D)
        q, k = q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin
        k, v = k.repeat_interleave(H // Hkv, 2), v.repeat_interleave(H // Hkv, 2)
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5
        s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("-inf"))
        h = h + torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(b, n, H * D) @ f(a.o_proj.weight).T
        x = norm(h, layer.post_attention_layernorm.weight)
        h = h + (torch.nn.functional.silu(x @ f(m.gate_proj.weight).T) * (x @ f(m.up_proj.weight).T)) @ f(m.down_proj.weight).T
    return norm(h, model.model.norm.weight) @ f(model.lm_head.weight).T


_E2E = {}


def e2e(heads, kv_heads):
    """The model, its prompts, plain decoding's tokens G and per-step logits, computed once per head geometry."""
    if (heads, kv_heads) not in _E2E:
        from tests.test_model_gpu import make_model

        seed = SEEDS[(heads, kv_heads)]
        model = make_model(torch.float16, head_dim=64, kv_heads=kv_heads, layers=2, heads=heads)
        with torch.no_grad():  # the weights of the CPU model the seed was searched with (generators differ between devices)
            for p, c in zip(model.parameters(), cpu_model(heads, kv_heads, seed).parameters()):
                p.copy_(c)
        model.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[PROMPT])
        prompts = cpu_prompts(seed).to(DEV)
        G, logits = model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, return_logits=True)
        logits = torch.stack(list(logits), 1) if not isinstance(logits, torch.Tensor) else logits
        top2 = logits.float().topk(2, -1).values
        _E2E[(heads, kv_heads)] = (model, prompts, G.cpu(), logits.float().cpu(), (top2[..., 0] - top2[..., 1]).cpu())
    return _E2E[(heads, kv_heads)]


def compared(gap):
    """Per row, how many leading positions are compared: up to the first one whose top-2 gap is below GAP."""
    below = gap < GAP
    return torch.where(below.any(1), below.int().argmax(1), torch.full((gap.shape[0],), gap.shape[1]))


def spec(model, prompts, **kw):
    return model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, return_draft_stats=True, **kw)


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
def test_plain_decode_stays_within_the_measured_logit_error(heads, kv_heads):
    """The condition of the comparisons below: plain decoding itself is within LOGIT_ERR of the float64 model on this seed, and at
    most 1 row in 6 is cut short by a top-2 gap below GAP."""
    model, prompts, G, logits, gap = e2e(heads, kv_heads)
    full = torch.cat([prompts.cpu().repeat_interleave(3, 0), G], 1)
    want = ref_logits64(model, full)[:, PROMPT - 1 : PROMPT - 1 + NEW]
    err = float((logits.double() - want).abs().max())
    n = compared(gap)
    print(f"heads {heads}/{kv_heads}: max |plain decode logits - float64 model| = {err:.4f}, smallest top-2 gap {float(gap.min()):.4f}, compared {n.tolist()}")
    assert err <= LOGIT_ERR
    assert int((n < NEW).sum()) <= 1


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_generate_with_drafts_returns_plain_decoding(heads, kv_heads, K):
    model, prompts, G, _, gap = e2e(heads, kv_heads)
    n = compared(gap)
    uncut = n == NEW
    T = K + 1
    model.stop_poll_steps = 1
    try:
        runs = {
            "perfect": spec(model, prompts, draft_tokens=K, draft=G.to(DEV)),
            "all wrong": spec(model, prompts, draft_tokens=K, draft=((G + 1) % 512).to(DEV)),
            "prompt lookup": spec(model, prompts, draft_tokens=K),
        }
    finally:
        del model.stop_poll_steps
    for name, (out, stats) in runs.items():
        out = out.cpu()
        assert out.shape == (6, NEW), name
        for b in range(6):
            assert torch.equal(out[b, : n[b]], G[b, : n[b]]), (name, b, out[b].tolist(), G[b].tolist())
        assert bool((stats.accepted <= stats.proposed).all()) and stats.steps <= NEW - 1, name
    _, s = runs["perfect"]
    assert torch.equal(s.accepted.cpu()[uncut], s.proposed.cpu()[uncut]) and bool((s.proposed.cpu()[uncut] == NEW - 1 - math.ceil((NEW - 1) / T)).all())
    if bool(uncut.all()):
        assert s.steps <= math.ceil((NEW - 1) / T) + 2, s.steps  # + the polling slack: a poll is read one step after it was started
    _, s = runs["all wrong"]
    assert int(s.accepted.cpu()[uncut].sum()) == 0 and (not bool(uncut.all()) or s.steps == NEW - 1)


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
def test_generate_without_the_fused_preamble_takes_the_assembled_attention(heads, kv_heads):
    """use_fused_decode off: the torch RoPE + scatter, then speculative.assembled_causal_tail_attention on the HIP operators (finished
    rows are not retired on this path).  Same tokens."""
    model, prompts, G, _, gap = e2e(heads, kv_heads)
    n = compared(gap)
    for layer in model.model.layers:
        layer.self_attn.use_fused_decode = False
    try:
        out, stats = spec(model, prompts, draft_tokens=3, draft=G.to(DEV))
        looked, _ = spec(model, prompts, draft_tokens=2)
    finally:
        for layer in model.model.layers:
            layer.self_attn.use_fused_decode = True
    for b in range(6):
        assert torch.equal(out.cpu()[b, : n[b]], G[b, : n[b]]) and torch.equal(looked.cpu()[b, : n[b]], G[b, : n[b]]), b
    assert int(stats.accepted.sum()) > 0


def test_graph_decode_on_and_off_return_the_same_tokens():
    model, prompts, G, _, gap = e2e(4, 4)
    n = compared(gap)
    eager, _ = spec(model, prompts, draft_tokens=3, draft=G.to(DEV))
    model.graph(True)
    try:
        graphed, st = spec(model, prompts, draft_tokens=3, draft=G.to(DEV))
    finally:
        model.graph(False)
    for b in range(6):
        assert torch.equal(eager[b, : n[b]], graphed[b, : n[b]])
    assert int(st.accepted.sum()) > 0


def test_eos_list_matches_the_truncation_of_plain_decoding():
    from hydragen_amd import stopping

    model, prompts, G, _, gap = e2e(8, 2)
    assert bool((compared(gap) == NEW).all()), "needs a seed on which no row is cut"
    eos = int(G[0, NEW // 2])  # an id G contains: row 0 (and its two copies) stop there at the latest
    sp = stopping.check_stop([eos], None, 7, False, 512)
    w_out, w_len, w_reason, w_index = stopping.truncate_reference(G, sp)
    out, lp, fin, stats = model.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, draft_tokens=3, draft=G.to(DEV),
                                         eos_token_id=[eos], pad_token_id=7, return_finish=True, return_logprobs=True, return_draft_stats=True)
    width = int(w_len.max())
    assert torch.equal(out.cpu(), w_out[:, :width])
    assert torch.equal(fin.lengths.cpu(), w_len) and torch.equal(fin.reasons.cpu(), w_reason) and torch.equal(fin.stop_index.cpu(), w_index)
    past = torch.arange(width)[None, :] >= w_len[:, None]
    assert lp.shape == out.shape and bool((lp.cpu()[past] == 0).all()) and bool((lp.cpu()[~past] <= 0).all())
