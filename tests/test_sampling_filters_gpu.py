"""-m gpu: hyd_sample_tokens_filtered (csrc/sample_filter.hip) against the float64 definition of the cuts
(hydragen_amd/sampling.py): tokens without cuts equal hyd_sample_tokens', kept counts, draws inside the kept set, the drawn
distribution, edge rows, log-probs, and the model shell's generate(top_k / top_p / min_p / return_logprobs)."""
import math

import pytest
import torch

from hydragen_amd import layer_ops, sampling

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
SLACK = 1e-5  # probability mass a row's boundary may sit from its threshold and still differ from float64


def _logits(rows, n, dtype, seed, scale=3.0, stride_pad=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, n + stride_pad, device=DEV, generator=g) * scale
    return x.to(dtype)[:, :n]  # stride_pad > 0: a strided row view


def _bounds(x, top_k, top_p, min_p):
    """Kept counts of the float64 definition with every threshold tightened / loosened by SLACK."""
    def cnt(tp, mp):
        return sampling.kept_mask(x, top_k, tp, mp).sum(-1)
    tp_lo = None if top_p is None else max(top_p - SLACK, 1e-6)
    tp_hi = None if top_p is None else min(top_p + SLACK, 1.0)
    mp_lo = None if min_p is None else min(min_p + SLACK, 1.0)
    mp_hi = None if min_p is None else max(min_p - SLACK, 0.0)
    return cnt(tp_lo, mp_lo), cnt(top_p, min_p), cnt(tp_hi, mp_hi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [0.0, 0.7, 1.0])
def test_no_cut_equals_the_plain_sampler(dtype, T):
    x = _logits(257, 32000, dtype, seed=1)
    want = layer_ops.sample_tokens(x, T, key=(77, 12))
    tok, lp, kept = layer_ops.sample_tokens_filtered(x, T, key=(77, 12))
    assert torch.equal(tok, want)
    assert (kept == 32000).all()
    got, lp2 = layer_ops.sample_tokens(x, T, key=(77, 12), return_logprobs=True)
    assert torch.equal(got, want) and torch.equal(lp2[:, 0], lp)


GRID = [(20, None, None), (1, None, None), (None, 0.9, None), (None, 0.5, None), (None, None, 0.05), (50, 0.95, None),
        (None, 0.95, 0.01), (40, 0.8, 0.1), (1000, 0.99, None)]


@pytest.mark.parametrize("V, pad", [(1000, 0), (32000, 0), (31997, 0), (32000, 24), (128256, 0), (128253, 8)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_kept_counts_equal_the_float64_definition(V, pad, dtype):
    x = _logits(96, V, dtype, seed=V + pad, stride_pad=pad)
    xd = x.double()
    allowed = 0
    for top_k, top_p, min_p in GRID:
        _, _, kept = layer_ops.sample_tokens_filtered(x, 1.0, key=(5, 0), top_k=top_k, top_p=top_p, min_p=min_p)
        lo, exact, hi = _bounds(xd, top_k, top_p, min_p)
        kept = kept.long()
        assert ((kept >= lo) & (kept <= hi)).all(), (top_k, top_p, min_p, kept, exact)
        allowed += int((kept != exact).sum())
        if top_k and not top_p and not min_p:
            assert torch.equal(kept, exact)  # keys are exact: top-k alone has no rounding
    assert allowed < 0.01 * len(GRID) * x.shape[0]


def test_no_draw_outside_the_kept_set():
    x = _logits(4096, 4000, torch.bfloat16, seed=11, scale=2.0)
    for top_k, top_p, min_p in [(30, None, None), (None, 0.9, None), (None, None, 0.1), (100, 0.95, 0.02)]:
        tok, _, kept = layer_ops.sample_tokens_filtered(x, 1.5, top_k=top_k, top_p=top_p, min_p=min_p)
        loose = sampling.kept_mask(x.double(), top_k, None if top_p is None else min(top_p + SLACK, 1.0),
                                   None if min_p is None else min_p - SLACK)
        assert loose.gather(1, tok).all()


def test_draws_follow_the_renormalised_softmax():
    g = torch.Generator(device=DEV).manual_seed(2)
    row = torch.randn(64, device=DEV, generator=g) * 1.5
    x = row[None].repeat(16384, 1)
    T, top_k, top_p = 0.8, 20, 0.8
    tok, _, kept = layer_ops.sample_tokens_filtered(x, T, key=(2024, 0), top_k=top_k, top_p=top_p)
    keep = sampling.kept_mask(row[None].double(), top_k, top_p)[0]
    assert (kept == int(keep.sum())).all() and int(keep.sum()) > 2
    want = torch.softmax(torch.where(keep, row.double() / T, torch.tensor(-math.inf, device=DEV, dtype=torch.float64)), -1)
    freq = torch.bincount(tok[:, 0], minlength=64).double() / tok.shape[0]
    assert 0.5 * (freq - want).abs().sum() <= 0.02


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_rows(dtype):
    x = _logits(64, 5000, dtype, seed=9)
    # T = 0 with cuts: the argmax (the max always survives; lowest index on ties)
    tok, _, _ = layer_ops.sample_tokens_filtered(x, 0.0, top_k=10, top_p=0.5, min_p=0.2)
    assert torch.equal(tok[:, 0], x.float().argmax(-1))
    tie = torch.zeros(1, 64, device=DEV, dtype=dtype)
    tie[0, [7, 9]] = 3.0
    assert layer_ops.sample_tokens_filtered(tie, 0.0, top_k=2)[0].item() == 7
    # -inf entries are never drawn, NaN neither; an all -inf row gives token 0 and keeps nothing
    y = x.clone()
    g = torch.Generator(device=DEV).manual_seed(4)
    y[torch.rand(y.shape, device=DEV, generator=g) < 0.5] = -math.inf
    y[:, 0] = float("nan")
    y[5] = -math.inf
    for cuts in (dict(), dict(top_k=50), dict(top_p=0.9), dict(min_p=0.01)):
        tok, lp, kept = layer_ops.sample_tokens_filtered(y, 1.0, **cuts)
        drawn = y.float().gather(1, tok)[:, 0]
        others = torch.arange(64, device=DEV) != 5
        assert torch.isfinite(drawn[others]).all()
        assert tok[5].item() == 0 and kept[5].item() == 0 and torch.isnan(lp[5])
    # a repeated key gives the same tokens, kept counts and log-probs bit for bit
    a = layer_ops.sample_tokens_filtered(x, 0.9, key=(3, 40), top_k=100, top_p=0.9, min_p=0.01)
    b = layer_ops.sample_tokens_filtered(x, 0.9, key=(3, 40), top_k=100, top_p=0.9, min_p=0.01)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logprobs_equal_log_softmax(dtype):
    x = _logits(128, 128256, dtype, seed=21, scale=4.0)
    tok, lp, _ = layer_ops.sample_tokens_filtered(x, 1.0, top_p=0.95)
    want = torch.log_softmax(x.double(), -1).gather(1, tok)[:, 0]
    assert (lp.double() - want).abs().max() < 1e-4


def _model(dtype=torch.bfloat16, seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=DEV, seed=seed, std=0.05)


def test_generate_top_p_tokens_unchanged_by_the_fused_path():
    model = _model()
    g = torch.Generator(device=DEV).manual_seed(8)
    prompt = torch.randint(1, 512, (1, 40), device=DEV, generator=g)
    model.setup_caches(max_unique_batch_size=16, max_unique_seq_length=32, max_shared_batch_sizes=[1],
                       max_shared_seq_lengths=[40])
    outs = {}
    for fused in (True, False):
        model.fused_sampling_filters = fused
        torch.manual_seed(1234)
        outs[fused] = model.generate(input_ids=prompt, num_return_sequences=16, max_new_tokens=12, temperature=0.7, top_p=0.9)
    model.fused_sampling_filters = True
    assert torch.equal(outs[True], outs[False])


def test_generate_with_cuts_and_logprobs_graph_on_and_off():
    model = _model()
    g = torch.Generator(device=DEV).manual_seed(9)
    prompt = torch.randint(1, 512, (1, 40), device=DEV, generator=g)
    model.setup_caches(max_unique_batch_size=8, max_unique_seq_length=32, max_shared_batch_sizes=[1],
                       max_shared_seq_lengths=[40])
    res = {}
    for graph in (False, True):
        model.graph(graph)
        torch.manual_seed(99)
        res[graph] = model.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=10, temperature=1.0, top_k=40,
                                    min_p=0.05, return_logprobs=True, return_logits=True)
    for graph, (out, logits, lp) in res.items():
        assert out.shape == lp.shape == (8, 10) and lp.dtype == torch.float32
        for j, lg in enumerate(logits):
            want = torch.log_softmax(lg.double(), -1).gather(1, out[:, j : j + 1])[:, 0]
            assert (lp[:, j].double() - want).abs().max() < 1e-4
            assert sampling.kept_mask(lg.double(), 40, None, 0.05 - SLACK).gather(1, out[:, j : j + 1]).all()
    (o0, l0, p0), (o1, l1, p1) = res[False], res[True]
    assert torch.equal(o0, o1) and torch.equal(p0, p1)
    # return_logprobs alone: (out, logprobs); EOS stops keep the columns aligned
    model.graph(False)
    out, lp = model.generate(input_ids=prompt, num_return_sequences=8, max_new_tokens=6, temperature=1.0, top_k=5,
                             return_logprobs=True, eos_token_id=int(o0[0, 2]))
    assert out.shape == lp.shape
