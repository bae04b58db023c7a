"""-m gpu: hyd_token_logprobs (csrc/token_logprob.hip) against the float64 definition (hydragen_amd/scoring.py) and against the
sampler's log-prob, its determinism, and the model shell's score() / generate(top_logprobs=) against independent paths.
The rows of `_rows` take the top-N select's one-gather histogram path almost everywhere; the rows built for its key and index
levels, its distance bin 255 and its full candidate buffer are tests/scoring_stress_cases.py, run by
tests/test_scoring_stress_gpu.py (tests/test_scoring_stress.py records which path each row of `_rows` takes)."""
import math

import pytest
import torch

from hydragen_amd import layer_ops, scoring
from hydragen_amd.llama import SharedCacheOp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
# Per-token log-prob agreement between score() and the independent bf16 paths of the same model (teacher-forced decode, the
# no-sharing prefill, a flat prompt).  They run different attention kernels and GEMM shapes over bf16 activations; the measured
# spread on this model is printed by the tests (max |diff| 1.6e-2 against each of the three, 1.9e-2 for the three-level
# hierarchy against a flat prompt, profiles/scoring.md); the bound is 3x that.
TOL = 6e-2
# fp8 unique caches against the bf16 caches where the prefill reads them back (disable_hydragen): measured 1.45e-1, bound 2x that
TOL_FP8 = 0.3


def _rows(rows, n, dtype, seed, pad=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(rows, n + pad, device=DEV, generator=g) * 3).to(dtype)
    if rows >= 8 and n >= 8:
        x[1, : n // 2] = 0.0                                              # ties at the max across half a row
        x[2] = torch.randint(0, 4, (n + pad,), device=DEV, generator=g).to(dtype)  # ~n/4 ties at the N-th value
        x[3] = (torch.randn(n + pad, device=DEV, generator=g) * 0.01).to(dtype)    # everything inside one 1/8 bin
        x[4, ::3] = float("nan")
        x[5, ::2] = float("-inf")
        x[6] = float("-inf")                                              # no valid logit
        x[7, 1:] = float("-inf")                                          # one valid logit
    return x[:, :n]


def _targets(x, seed):
    R, n = x.shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randint(0, n, (R,), device=DEV, generator=g)
    t[::5] = x.float().nan_to_num(nan=-math.inf).argmax(-1)[::5]  # greedy rows
    if R > 9:
        t[8], t[9] = -1, n  # padding
    return t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V, pad", [(1, 0), (7, 0), (32000, 0), (32000, 24), (128256, 0), (128253, 8)])
def test_kernel_against_float64(dtype, V, pad):
    x = _rows(48, V, dtype, seed=V + pad, pad=pad)
    t = _targets(x, seed=V)
    for N in (0, 1, 5, 20):
        lp, greedy, ids, tlp = layer_ops.token_logprobs(x, t, N)
        rlp, rgreedy, rids, rtlp = scoring.token_logprobs_reference(x.cpu(), t.cpu(), N)
        assert lp.shape == (48,) and greedy.dtype == torch.bool and ids.shape == tlp.shape == (48, N)
        assert torch.equal(greedy.cpu(), rgreedy)
        assert torch.equal(ids.cpu(), rids)
        a, b = lp.cpu().double(), rlp.double()
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a == -math.inf, b == -math.inf)
        fin = torch.isfinite(b)
        assert (a[fin] - b[fin]).abs().max() < 1e-5
        a, b = tlp.cpu().double(), rtlp.double()
        assert torch.equal(a == -math.inf, b == -math.inf)
        fin = torch.isfinite(b)
        if fin.any():
            assert (a[fin] - b[fin]).abs().max() < 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprob_equals_the_samplers_bit_for_bit(dtype):
    x = _rows(256, 32000, dtype, seed=3)
    for T in (0.0, 1.0):
        tok, slp, _ = layer_ops.sample_tokens_filtered(x, T, key=(11, 4), top_p=0.9)
        lp, greedy, _, _ = layer_ops.token_logprobs(x, tok[:, 0], 3)
        ok = ~slp.isnan()
        assert torch.equal(lp[ok], slp[ok]) and torch.equal(lp.isnan(), slp.isnan())
        if T == 0.0:
            assert greedy[ok].all()


def _same(a, b):
    """Bitwise equal, NaN where the other has NaN."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a[~a.isnan()], b[~b.isnan()])


def test_rows_do_not_depend_on_the_launch():
    x = _rows(300, 128256, torch.bfloat16, seed=5)
    t = _targets(x, seed=5)
    full = layer_ops.token_logprobs(x, t, 20)
    again = layer_ops.token_logprobs(x, t, 20)
    for a, b in zip(full, again):
        assert _same(a, b)
    for i in (0, 1, 2, 3, 8, 150, 299):
        one = layer_ops.token_logprobs(x[i : i + 1], t[i : i + 1], 20)
        for a, b in zip(full, one):
            assert _same(a[i : i + 1], b)
    parts = [layer_ops.token_logprobs(x[s : s + 37], t[s : s + 37], 20) for s in range(0, 300, 37)]
    for k in range(4):
        assert _same(full[k], torch.cat([p[k] for p in parts]))
    # N = 0 and N > 0 give the same log-probs and flags
    n0 = layer_ops.token_logprobs(x, t, 0)
    assert _same(n0[0], full[0]) and _same(n0[1], full[1])


# ---- model shell ---------------------------------------------------------------------------------------------------------
VOCAB = 512


def _model(seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=VOCAB, max_position_embeddings=1024, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=seed, std=0.05)


@pytest.fixture(scope="module")
def model():
    m = _model()
    m.setup_caches(max_unique_batch_size=64, max_unique_seq_length=64, max_shared_batch_sizes=[1, 8],
                   max_shared_seq_lengths=[32, 16])
    return m


def _case(B=6, P=24, Lu=10, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    prefix = torch.randint(1, VOCAB, (1, P), device=DEV, generator=g)
    uids = torch.randint(1, VOCAB, (B, Lu), device=DEV, generator=g)
    ul = torch.randint(2, Lu + 1, (B,), device=DEV, generator=g)
    ul[0] = Lu
    tl = torch.minimum(torch.randint(1, Lu, (B,), device=DEV, generator=g), ul - 1)
    return prefix, uids, ul, tl


def _teacher_forced(model, prefix, uids, ul, tl):
    """log softmax in float64 of generate(token_overrides=..., return_logits=True) along the targets: [B, T]."""
    B = uids.shape[0]
    T = int(tl.max())
    ctx_len = ul - tl
    ctx = torch.zeros_like(uids)
    over = torch.zeros((B, T), dtype=torch.long, device=DEV)
    for b in range(B):
        c, t = int(ctx_len[b]), int(tl[b])
        ctx[b, :c] = uids[b, :c]
        over[b, :t] = uids[b, c : c + t]
    out, logits = model.generate(input_ids=[prefix, ctx[:, : int(ctx_len.max())]], seq_lens=[torch.tensor([prefix.shape[1]],
                                 device=DEV), ctx_len], max_new_tokens=T, temperature=0.0, token_overrides=over, return_logits=True)
    lps = torch.stack([torch.log_softmax(lg.double(), -1).gather(1, over[:, j : j + 1])[:, 0] for j, lg in enumerate(logits[:T])], 1)
    return lps, logits[:T]


def _live(tl, T):
    return torch.arange(T, device=DEV)[None, :] < tl[:, None]


def _flat(prefix, uids, ul):
    B, P = uids.shape[0], prefix.shape[1]
    flat = torch.cat([prefix.expand(B, -1), uids], 1)
    return flat, P + ul


def test_score_against_three_independent_paths(model):
    prefix, uids, ul, tl = _case()
    plen = torch.tensor([prefix.shape[1]], device=DEV)
    res = model.score([prefix, uids], tl, seq_lens=[plen, ul])
    T = int(tl.max())
    live = _live(tl, T)
    assert res.logprobs.shape == res.token_greedy.shape == (6, T) and res.sum.dtype == torch.float64
    assert res.logprobs[~live].isnan().all() and torch.isfinite(res.logprobs[live]).all()
    assert torch.allclose(res.sum, torch.where(live, res.logprobs.double(), 0.0).sum(1))
    tf, _ = _teacher_forced(model, prefix, uids, ul, tl)
    base = model.score([prefix, uids], tl, seq_lens=[plen, ul], disable_hydragen=True)
    flat, flen = _flat(prefix, uids, ul)
    fl = model.score(flat, tl, seq_lens=flen)
    for name, other in (("teacher-forced", tf), ("disable_hydragen", base.logprobs), ("flat", fl.logprobs)):
        d = (res.logprobs.double() - other.double())[live].abs().max().item()
        print(f"score() vs {name}: max |diff| {d:.2e}")
        assert d < TOL, name


def test_three_level_hierarchy_scores_the_first_token_from_shared_logits(model):
    g = torch.Generator(device=DEV).manual_seed(4)
    few = torch.randint(1, VOCAB, (1, 20), device=DEV, generator=g)
    Q, C = 3, 4
    qs = torch.randint(1, VOCAB, (Q, 8), device=DEV, generator=g)
    qlen = torch.tensor([8, 5, 6], device=DEV)
    ch = torch.randint(1, VOCAB, (Q * C, 5), device=DEV, generator=g)
    clen = torch.randint(1, 6, (Q * C,), device=DEV, generator=g)
    res = model.score([few, qs, ch], clen, seq_lens=[torch.tensor([20], device=DEV), qlen, clen], top_logprobs=4)
    assert res.top_ids.shape == (Q * C, int(clen.max()), 4)
    assert model.get_num_used_shared_caches() == 0
    # flat: each choice's full string as one unique prompt
    rows, lens = [], []
    for b in range(Q * C):
        q = b // C
        rows.append(torch.cat([few[0], qs[q, : int(qlen[q])], ch[b]]))
        lens.append(20 + int(qlen[q]) + int(clen[b]))
    W = max(r.numel() for r in rows)
    flat = torch.stack([torch.cat([r, r.new_zeros(W - r.numel())]) for r in rows])
    fl = model.score(flat, clen, seq_lens=torch.tensor(lens, device=DEV), top_logprobs=4)
    live = _live(clen, int(clen.max()))
    d = (res.logprobs.double() - fl.logprobs.double())[live].abs().max().item()
    print(f"three-level vs flat: max |diff| {d:.2e}")
    assert d < TOL
    assert torch.isfinite(res.logprobs[:, 0]).all()  # every first target came from the question's logits


def test_results_do_not_depend_on_the_chunk_size(model):
    prefix, uids, ul, tl = _case(B=64, Lu=12, seed=7)
    plen = torch.tensor([prefix.shape[1]], device=DEV)
    tl = torch.minimum(ul - 1, torch.full_like(tl, 11))  # ~ 400 scored rows: several GEMM blocks
    big = model.score([prefix, uids], tl, seq_lens=[plen, ul], top_logprobs=5)
    old = model.score_chunk_bytes
    try:
        for rows in (1, 300):
            model.score_chunk_bytes = rows * VOCAB * 2
            small = model.score([prefix, uids], tl, seq_lens=[plen, ul], top_logprobs=5)
            for f in ("logprobs", "token_greedy", "sum", "is_greedy", "top_ids", "top_logprobs"):
                a, b = getattr(big, f), getattr(small, f)
                assert _same(a, b), f
    finally:
        model.score_chunk_bytes = old


def test_top_logprobs_consistent_with_the_teacher_forced_logits(model):
    prefix, uids, ul, tl = _case(seed=9)
    plen = torch.tensor([prefix.shape[1]], device=DEV)
    res = model.score([prefix, uids], tl, seq_lens=[plen, ul], top_logprobs=5)
    _, logits = _teacher_forced(model, prefix, uids, ul, tl)
    for j, lg in enumerate(logits):
        _, _, rids, rtlp = scoring.token_logprobs_reference(lg.cpu(), torch.zeros(lg.shape[0], dtype=torch.long), 5)
        for b in range(uids.shape[0]):
            if j >= int(tl[b]):
                assert (res.top_ids[b, j] == -1).all() and (res.top_logprobs[b, j] == -math.inf).all()
                continue
            got = res.top_logprobs[b, j].cpu().double()
            assert (got - rtlp[b].double()).abs().max() < TOL
            assert (got[:-1] >= got[1:]).all()
            gaps = torch.cat([torch.tensor([math.inf]), (rtlp[b, :-1] - rtlp[b, 1:]).double(), torch.tensor([math.inf])])
            clear = (gaps[:-1] > 2 * TOL) & (gaps[1:] > 2 * TOL)
            assert torch.equal(res.top_ids[b, j].cpu()[clear], rids[b][clear])


def test_preserve_leaves_the_cache_state_as_it_was(model):
    prefix, uids, ul, tl = _case(seed=11)
    plen = torch.tensor([prefix.shape[1]], device=DEV)

    def gen():
        torch.manual_seed(5)
        return model.generate(input_ids=[prefix, uids], seq_lens=[plen, ul], max_new_tokens=6, temperature=1.0)

    before = gen()
    model.score([prefix, uids], tl, seq_lens=[plen, ul], shared_cache_op=SharedCacheOp.PRESERVE)
    assert model.get_num_used_shared_caches() == 0
    assert torch.equal(before, gen())


def test_greedy_continuations_are_greedy(model):
    prefix, uids, ul, _ = _case(seed=13)
    plen = torch.tensor([prefix.shape[1]], device=DEV)
    T = 6
    cont, logits = model.generate(input_ids=[prefix, uids], seq_lens=[plen, ul], max_new_tokens=T, temperature=0.0,
                                  return_logits=True)
    B, Lu = uids.shape
    full = torch.cat([uids, torch.zeros((B, T), dtype=uids.dtype, device=DEV)], 1)
    for b in range(B):
        full[b, int(ul[b]) : int(ul[b]) + T] = cont[b]
    res = model.score([prefix, full], torch.full((B,), T, device=DEV), seq_lens=[plen, ul + T])
    top2 = torch.stack([lg.topk(2, -1).values for lg in logits], 1)  # [B, T, 2]
    close = (top2[..., 0] - top2[..., 1]) < TOL
    print(f"greedy continuations: {int(close.sum())} of {close.numel()} positions within {TOL} of a tie")
    assert (res.token_greedy | close).all()
    assert torch.equal(res.is_greedy, (res.token_greedy).all(1))


def test_fp8_unique_caches_agree_with_bf16():
    m = _model(seed=2)
    prefix, uids, ul, tl = _case(seed=15)
    plen = torch.tensor([prefix.shape[1]], device=DEV)
    out = {}
    for kvd in (None, torch.float8_e4m3fn):
        m.setup_caches(max_unique_batch_size=8, max_unique_seq_length=48, max_shared_batch_sizes=[1],
                       max_shared_seq_lengths=[32], kv_cache_dtype=kvd)
        for base in (False, True):
            out[kvd, base] = m.score([prefix, uids], tl, seq_lens=[plen, ul], disable_hydragen=base)
    live = _live(tl, int(tl.max()))
    for base in (False, True):
        d = (out[None, base].logprobs.double() - out[torch.float8_e4m3fn, base].logprobs.double())[live].abs().max().item()
        print(f"fp8 vs bf16 unique caches, disable_hydragen={base}: max |diff| {d:.2e}")
        assert d < TOL_FP8
    # the shared-prefix prefill attends over this call's own 16-bit K/V and only writes the cache: identical results
    assert _same(out[None, False].logprobs, out[torch.float8_e4m3fn, False].logprobs)


def test_generate_top_logprobs():
    m = _model(seed=3)
    g = torch.Generator(device=DEV).manual_seed(17)
    prompt = torch.randint(1, VOCAB, (1, 24), device=DEV, generator=g)
    m.setup_caches(max_unique_batch_size=8, max_unique_seq_length=32, max_shared_batch_sizes=[1], max_shared_seq_lengths=[24])
    res = {}
    for graph in (False, True):
        m.graph(graph)
        torch.manual_seed(21)
        res[graph] = m.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=9, temperature=1.0, top_k=50,
                                return_logprobs=True, return_logits=True, top_logprobs=5)
    m.graph(False)
    out, logits, lp, ids, tlp = res[False]
    assert ids.shape == tlp.shape == (8, 9, 5) and ids.dtype == torch.int64 and tlp.dtype == torch.float32
    for k in (0, 2, 3, 4):  # tokens, log-probs, top ids, top log-probs
        assert torch.equal(res[False][k], res[True][k])
    for j in range(9):
        assert torch.equal(ids[:, j, 0], logits[j].argmax(-1))
        want = torch.log_softmax(logits[j].double(), -1).gather(1, ids[:, j])
        assert (tlp[:, j].double() - want).abs().max() < 1e-4
    # the sampled token's log-prob is the sampler's, with or without top_logprobs
    torch.manual_seed(21)
    out2, lp2 = m.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=9, temperature=1.0, top_k=50,
                           return_logprobs=True)
    torch.manual_seed(21)
    out3, lp3, ids3, _ = m.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=9, temperature=1.0, top_k=50,
                                    return_logprobs=True, top_logprobs=5)
    assert torch.equal(out2, out3) and torch.equal(lp2, lp3)
    # EOS stops keep the columns aligned
    torch.manual_seed(21)
    o, l, i, t = m.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=9, temperature=1.0, top_k=50,
                            return_logprobs=True, top_logprobs=2, eos_token_id=int(out2[0, 2]))
    assert o.shape == l.shape and i.shape == t.shape == o.shape + (2,)
