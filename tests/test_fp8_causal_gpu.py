"""-m gpu: speculative decoding on fp8 (e4m3fn) unique K/V caches.
  * the causal-tail form of the fp8 matrix-core suffix kernel (csrc/suffix_attn_gqa_fp8_causal.hip): `out` and `lse` BIT-IDENTICAL to
    the 16-bit causal matrix-core kernel on dequantize_kv of the caches, with flash.dequantize_kv patched to raise during every fp8 call;
  * the multi-token preamble on fp8 caches (hyd_rope_append_multi_kvq): the bytes of T one-token calls, exactly;
  * generate(draft_tokens=) on fp8 caches, end to end."""
import numpy as np
import pytest
import torch

from hydragen_amd import flash as F
from hydragen_amd.attention import hydragen_attention
from hydragen_amd.constraint import TokenDFA
from hydragen_amd.flash import flash_attention_seqlen
from hydragen_amd.fused_decode import rope_append_decode, rope_append_multi
from hydragen_amd.kv_quant import FP8_DTYPE, dequantize_kv, quantize_kv
from tests.gpu_util import TORCH_DT
from tests.test_constrained_drafts import forced_steps
from tests.test_speculative_gpu import _lengths

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 4


def _no_fallback(monkeypatch):
    """flash / attention and the model's multi-token step (its assembled route) may not dequantize: a fallback fails instead of passing."""
    import hydragen_amd.llama as L

    def raiser(*a, **k):
        raise AssertionError("dequantize_kv reached: the fp8 causal call fell back to a 16-bit path")

    monkeypatch.setattr(F, "dequantize_kv", raiser)
    monkeypatch.setattr(L, "dequantize_kv", raiser)


# ---- the kernel, bit for bit --------------------------------------------------------------------------------------------------------
# S = 132: few units, four waves per unit; S = 40: one wave per unit with 1 / 2 / 4 kv heads per workgroup.  (4, 4) with T = 2: units of
# 2 rows; (6, 2) with T = 8: a 16-row chunk boundary inside a token.  Head dim 256: S = 40 only (few units are not eligible).
CASES = [(dt, T, hq, hkv, D, S) for dt in ("f16", "bf16") for T in (2, 3, 5, 8) for hq, hkv in ((4, 4), (8, 2), (8, 1), (6, 2))
         for D in (64, 128) for S in (132, 40)]
CASES += [(dt, T, hq, hkv, 256, 40) for dt in ("f16", "bf16") for T, hq, hkv in ((3, 8, 2), (5, 8, 1), (3, 4, 4))]
SCALES = ("pow2", "arbitrary", None)


def _scales(rng, Hkv, kind):
    if kind is None:  # all ones, given as tensors (the causal call takes fp8 caches only with both)
        return torch.ones(Hkv, device=DEV), torch.ones(Hkv, device=DEV)
    if kind == "pow2":  # mixed powers of two per head: a head / scale mix-up fails, every product is exact
        mk = lambda: torch.from_numpy((2.0 ** rng.integers(-3, 4, Hkv)).astype(np.float32)).to(DEV)  # noqa: E731
    else:  # products that do not fit the 16-bit formats: the rounding of the widening itself
        mk = lambda: torch.from_numpy((0.1 + rng.random(Hkv)).astype(np.float32)).to(DEV)  # noqa: E731
    return mk(), mk()


def _problem(rng, dt, T, Hq, Hkv, D, S, kind, lens):
    g = torch.Generator(device=DEV).manual_seed(int(rng.integers(1 << 31)))
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV).to(TORCH_DT[dt])  # noqa: E731
    q, k, v = rnd(B, T, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
    ks, vs = _scales(rng, Hkv, kind)
    k8, v8 = quantize_kv(k, ks), quantize_kv(v, vs)
    sl = torch.tensor([min(n, S) for n in lens], dtype=torch.int32, device=DEV)
    past = torch.arange(S, device=DEV)[None, :] >= sl.long()[:, None]
    for x8 in (k8, v8):  # rows at and past each sequence's length hold the fp8 NaN byte
        x8.view(torch.uint8)[past] = 0x7F
    return q, k8, v8, ks, vs, sl


def _reference_16bit(q, kd, vd, sl):
    """The 16-bit causal call on the dequantized caches.  Units of >= 3 rows: flash_attention_seqlen(causal_tail=True) runs the 16-bit
    causal matrix-core kernel, the kernel of the contract.  Units of 2 rows ((4, 4) heads, T = 2) go to the one-unit-per-wave kernel
    there, another summation order; the matrix-core kernel takes the same rows as the LAST two tokens of a three-token call (token i of
    T + 1 tokens and token i - 1 of T tokens have the same key limit, a query row's arithmetic does not depend on the rows beside it, and
    the launch plan -- units, chunks, keys -- is the same), so the reference is that call with a zero token in front, cut off again."""
    T, g = q.shape[1], q.shape[2] // kd.shape[2]
    if T * g >= 3:
        return flash_attention_seqlen(q, kd, vd, sl, causal_tail=True)
    out, lse = flash_attention_seqlen(torch.cat([torch.zeros_like(q[:, :1]), q], 1), kd, vd, sl, causal_tail=True)
    return out[:, 1:].contiguous(), lse[:, 1:].contiguous()


def _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl, what):
    o16, l16 = _reference_16bit(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), sl)
    with monkeypatch.context() as m:
        _no_fallback(m)
        o8, l8 = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs, causal_tail=True)
    torch.cuda.synchronize()
    assert not torch.isnan(o8).any(), what
    assert torch.equal(o8, o16), (what, int((o8 != o16).sum()))
    assert torch.equal(l8, l16), (what, int((l8 != l16).sum()))
    return o8, l8


@pytest.mark.parametrize("dt, T, Hq, Hkv, D, S", CASES)
def test_fp8_causal_kernel_is_bit_identical_to_the_16bit_causal_kernel(monkeypatch, dt, T, Hq, Hkv, D, S):
    case = CASES.index((dt, T, Hq, Hkv, D, S))
    drawn = _lengths(T, case)  # T, T + 1, 31 .. 33, 63 .. 65, 129 by turns, and a retired row of 0
    for i, kind in enumerate(SCALES):
        # the four rows as drawn, and with the retired row replaced by one shorter than T (its first tokens see no key at all)
        for lens in (drawn, drawn[:3] + [T - 1 - (i % (T - 1)) if T > 2 else 1]):
            rng = np.random.default_rng(1000 * case + 10 * i + len(lens) + lens[3])
            q, k8, v8, ks, vs, sl = _problem(rng, dt, T, Hq, Hkv, D, S, kind, lens)
            what = f"{dt} T={T} heads {Hq}/{Hkv} D={D} S={S} scales={kind} lens {sl.tolist()}"
            o8, l8 = _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl, what)
            short = sl.cpu() < T
            for b in torch.nonzero(short).flatten().tolist():  # token i of a row of length n < T sees n - (T - 1 - i) <= 0 keys: zeros, lse -inf
                blind = T - int(sl[b])
                assert not o8[b, :blind].any() and bool(torch.isinf(l8[b, :blind]).all()), what
                assert int(sl[b]) == 0 or bool(torch.isfinite(l8[b, blind:]).all()), what
    # the same fp8 call WITHOUT the per-row limit is another function: a kernel that ignores it cannot pass
    if T * (Hq // Hkv) >= 3:
        plain, _ = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs)
        live = sl >= T
        assert not torch.equal(plain[live], o8[live])


LEVEL_SHAPES = [("f16", 3, 8, 2, 128, 40), ("bf16", 8, 6, 2, 64, 132)]


@pytest.mark.parametrize("dt, T, Hq, Hkv, D, S", LEVEL_SHAPES)
def test_whole_operator_with_levels_is_bit_identical_on_fp8_and_dequantized_caches(monkeypatch, dt, T, Hq, Hkv, D, S):
    """hydragen_attention(causal_tail=True) with one and with two shared levels: the level passes are the same launches, the suffix
    pass merges their partials in its epilogue -- equal bit for bit to the same call on the dequantized caches."""
    rng = np.random.default_rng(T * 100 + D)
    q, k8, v8, ks, vs, sl = _problem(rng, dt, T, Hq, Hkv, D, S, "arbitrary", _lengths(T, 1)[:3] + [1])
    g = torch.Generator(device=DEV).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV).to(TORCH_DT[dt])  # noqa: E731
    levels = [(rnd(1, 40, Hkv, D), rnd(1, 40, Hkv, D)), (rnd(2, 300, Hkv, D), rnd(2, 300, Hkv, D))]  # (300 keys: a level the prefix kernel runs)
    kd, vd = dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype)
    for n in (1, 2):
        lk, lv = [a for a, _ in levels[:n]], [b for _, b in levels[:n]]
        want = hydragen_attention(q, kd, vd, lk, lv, [None] * n, [None] * n, [False] * n, sl, causal_tail=True)
        with monkeypatch.context() as m:
            _no_fallback(m)
            got = hydragen_attention(q, k8, v8, lk, lv, [None] * n, [None] * n, [False] * n, sl, k_scale=ks, v_scale=vs, causal_tail=True)
        torch.cuda.synchronize()
        assert not torch.isnan(got).any() and torch.equal(got, want), (n, int((got != want).sum()))


def test_fp8_causal_call_under_a_captured_graph_equals_eager(monkeypatch):
    rng = np.random.default_rng(77)
    q, k8, v8, ks, vs, sl = _problem(rng, "bf16", 5, 8, 2, 128, 132, "pow2", [129, 64, 33, 3])
    eager, eager_lse = _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl, "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs, causal_tail=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs, causal_tail=True)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(lse, eager_lse)
    # the scales and the lengths are read at run time: a replay sees the values of its own moment (shorter lengths: the rows behind
    # the first ones hold the NaN byte)
    sl.copy_(torch.tensor([70, 60, 33, 2], device=DEV, dtype=torch.int32))
    ks.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    want, want_lse = _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl, "after the update")
    assert torch.equal(out, want) and torch.equal(lse, want_lse) and not torch.equal(out, eager)


def test_fp8_causal_calls_that_no_kernel_takes_raise():
    """Never dequantized into, or run as, a non-causal call."""
    rng = np.random.default_rng(3)
    q, k8, v8, ks, vs, sl = _problem(rng, "bf16", 2, 4, 4, 256, 132, "pow2", [129, 64, 33, 3])  # head dim 256 with few units
    with pytest.raises(NotImplementedError, match="causal"):
        flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs, causal_tail=True)
    with pytest.raises(NotImplementedError, match="causal"):
        hydragen_attention(q, k8, v8, [], [], [], [], [], sl, k_scale=ks, v_scale=vs, causal_tail=True)
    q, k8, v8, ks, vs, sl = _problem(rng, "bf16", 3, 8, 2, 128, 40, "pow2", [40, 33, 3, 0])
    with pytest.raises(NotImplementedError, match="causal_tail"):
        hydragen_attention(q, k8, v8, [], [], [], [], [], None, k_scale=ks, v_scale=vs, causal_tail=True)
    for kw in (dict(), dict(k_scale=ks), dict(v_scale=vs)):  # without both scale tensors: the refusal the call has always had
        with pytest.raises(NotImplementedError, match="causal_tail"):
            flash_attention_seqlen(q, k8, v8, sl, causal_tail=True, **kw)


# ---- the preamble, exactly ---------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def _rope_tables(D, n):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    ang = torch.cat([ang, ang], -1)
    return ang.cos().float().to(DEV), ang.sin().float().to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "qk-norm"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("T", [2, 8])
def test_rope_append_multi_on_fp8_caches_writes_the_bytes_of_one_token_calls(dtype, norm, D, T):
    Bp, Hq, Hkv, cache_len, max_pos = 5, 8, 2, 12, 64
    g = torch.Generator(device=DEV).manual_seed(100 * T + D + norm)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)  # noqa: E731
    q, k, v = rnd(Bp, T, Hq, D).to(dtype), (3 * rnd(Bp, T, Hkv, D)).to(dtype), (3 * rnd(Bp, T, Hkv, D)).to(dtype)
    v[0, 1, 1, 5] = float("nan")  # one NaN input: it stays NaN (0x7F), alone
    # head 0: a scale that sends |x / scale| beyond 448 (the clamp); head 1: an arbitrary one
    ks = torch.tensor([2.0 ** -9, 0.37], device=DEV)
    vs = torch.tensor([0.61, 2.0 ** -8], device=DEV)
    shared = torch.tensor([3, 7, 5, 0, 9], device=DEV)
    # row 1: position shared_len - 1 (retired); row 2: its last tokens (1 of 2, 3 of 8) reach cache_len; row 4: the last index it may write
    idx0 = torch.tensor([0, -1, cache_len - T + min(3, T - 1), 2, cache_len - T], device=DEV)
    pos0 = shared + idx0
    cos, sin = _rope_tables(D, max_pos)
    gains = dict(q_norm=(1 + 0.3 * rnd(D)).to(dtype), k_norm=(1 - 0.3 * rnd(D)).to(dtype), norm_eps=1e-6) if norm else {}

    def caches(dt):
        fill = torch.full((Bp + 1, cache_len + 2, Hkv, D), SENTINEL, dtype=torch.uint8, device=DEV)  # (guard rows and a guard sequence)
        if dt == FP8_DTYPE:
            return fill.view(FP8_DTYPE), fill.clone().view(FP8_DTYPE)
        wide = torch.full((Bp + 1, cache_len + 2, Hkv, D), 7.0, dtype=dt, device=DEV)
        return wide, wide.clone()

    k8, v8 = caches(FP8_DTYPE)
    q_out, sl = rope_append_multi(q, k, v, cos, sin, pos0, shared, k8[:Bp, :cache_len], v8[:Bp, :cache_len], **gains, k_scale=ks, v_scale=vs)
    # (1) the 16-bit multi-token call on the same inputs: q_out and seq_lens are its bits, the cache bytes quantize_kv of its rows
    k16, v16 = caches(dtype)
    q_16, sl_16 = rope_append_multi(q, k, v, cos, sin, pos0, shared, k16[:Bp, :cache_len], v16[:Bp, :cache_len], **gains)
    torch.cuda.synchronize()
    assert torch.equal(q_out.view(torch.int16), q_16.view(torch.int16)) and torch.equal(sl, sl_16)
    assert sl.tolist() == [T, 0, int(idx0[2]) + T, 2 + T, cache_len]
    written = torch.zeros((Bp + 1, cache_len + 2), dtype=torch.bool, device=DEV)
    for b in range(Bp):
        for i in range(T):
            j = int(idx0[b]) + i
            if int(idx0[b]) >= 0 and j < cache_len:
                written[b, j] = True
    assert int(written[2].sum()) == T - min(3, T - 1) and not written[1].any() and bool(written[4, cache_len - 1])
    # (a NaN is a NaN code exactly where quantize_kv has one; the sign bit of that code is not part of the definition -- the rule of
    # tests/test_fp8_kv_gpu.py for the one-token kernel -- so both NaN codes compare as 0x7F; every other byte bit for bit)
    one_nan = lambda b: torch.where((b & 0x7F) == 0x7F, torch.full_like(b, 0x7F), b)  # noqa: E731
    for x8, x16, sc, name in ((k8, k16, ks, "K"), (v8, v16, vs, "V")):
        got = x8.view(torch.uint8)
        want = torch.where(written[:, :, None, None], quantize_kv(x16, sc).view(torch.uint8), torch.full_like(got, SENTINEL))
        assert torch.equal(one_nan(got), one_nan(want)), f"{name}: written rows hold quantize_kv of the 16-bit rows, every other byte keeps the sentinel"
        assert bool((x16[~written] == 7.0).all())
    assert int(((v8.view(torch.uint8)[0, 1] & 0x7F) == 0x7F).sum()) == 1 and int(v8.view(torch.uint8)[0, 1, 1, 5]) & 0x7F == 0x7F
    assert int(((k8.view(torch.uint8)[written] & 0x7F) == 0x7F).sum()) == 0
    assert int(((k8.view(torch.uint8)[written][:, 0] & 0x7F) == 0x7E).sum()) > 0, "no value reached the clamp: +-448 is code 0x7E / 0xFE"
    # (2) T successive one-token calls at positions pos + i on the same q / k / v (the retired row left out: one-token calls know no
    # retired row and would write its later tokens)
    live = [0, 2, 3, 4]
    k1, v1 = caches(FP8_DTYPE)
    for i in range(T):
        sub = lambda x: x[live, i : i + 1].contiguous()  # noqa: E731
        rows_k = torch.full((len(live), cache_len, Hkv, D), SENTINEL, dtype=torch.uint8, device=DEV).view(FP8_DTYPE)
        rows_v = rows_k.clone()
        rows_k.view(torch.uint8).copy_(k1.view(torch.uint8)[live, :cache_len])
        rows_v.view(torch.uint8).copy_(v1.view(torch.uint8)[live, :cache_len])
        q1, _ = rope_append_decode(sub(q), sub(k), sub(v), cos, sin, (pos0[live] + i)[:, None], shared[live], rows_k, rows_v, **gains,
                                   k_scale=ks, v_scale=vs)
        k1.view(torch.uint8)[live, :cache_len] = rows_k.view(torch.uint8)
        v1.view(torch.uint8)[live, :cache_len] = rows_v.view(torch.uint8)
        assert torch.equal(q1[:, 0].view(torch.int16), q_out[live, i].view(torch.int16)), i
    torch.cuda.synchronize()
    assert torch.equal(k8.view(torch.uint8), k1.view(torch.uint8)) and torch.equal(v8.view(torch.uint8), v1.view(torch.uint8))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
# Weights-independent and exact: the fully forced choice below, eager and graph, temperature 0 and 1, calibrated scales, and through
# the assembled route.  A comparison of drafted against PLAIN fp8 decoding token by token (as tests/test_speculative_gpu.py compares
# 16-bit caches) is NOT here, because its condition cannot be met (profiles/speculative_fp8.md has the runs):
#   LOGIT_ERR_FP8 = 0.035: the largest |plain fp8-cache decode logits - float64 model with the fp8 round trip (tests/fp8_spec_ref.py)|
#     over the models and prompts of tests/test_speculative_gpu.py, measured on the commit before the feature: 0.01175 (4/4 heads,
#     seed 115) and 0.03422 (8/2, seed 81), the larger rounded up (16-bit caches, same runs: 0.00394 / 0.00795).  An fp16 last-bit
#     difference in a rotated k moves an e4m3 code, a sixteenth of the value, which the float64 model does not see.
#   GAP_FP8 = 2 x LOGIT_ERR_FP8 = 0.07.
#   Seeds 0 .. 399 of weights and prompts, searched on the CPU with that float64 model for the largest smallest top-2 gap of the
#     48 greedy decisions: std 0.05: 0.0354 (4/4, seed 382) and 0.0588 (8/2, seed 212) -- no seed keeps every gap above 0.07, and a gap
#     below it cuts a prompt's three rows, 3 rows in 6; std 0.1: 0.0613 (4/4, seed 135) and 0.1533 (8/2, seed 347), but plain fp8
#     decoding of those models is 0.154 / 0.245 off the float64 model (seeds 71 / 117: 0.066 / 0.593), beyond LOGIT_ERR_FP8.
EOS = 511
NEW, PROMPT = 24, 48
_MODELS = {}


def fp8_model(heads, kv_heads, seed, kv_scales="unit"):
    """The 2-layer fp16 model of tests/test_speculative_gpu.py with the CPU model's weights and fp8 unique caches."""
    key = (heads, kv_heads, seed, kv_scales)
    if key not in _MODELS:
        from tests.test_model_gpu import make_model
        from tests.test_speculative_gpu import cpu_model, cpu_prompts

        model = make_model(torch.float16, head_dim=64, kv_heads=kv_heads, layers=2, heads=heads)
        with torch.no_grad():
            for p, c in zip(model.parameters(), cpu_model(heads, kv_heads, seed).parameters()):
                p.copy_(c)
        model.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[PROMPT],
                           kv_cache_dtype=FP8_DTYPE, kv_scales=kv_scales)
        _MODELS[key] = (model, cpu_prompts(seed).to(DEV))
    return _MODELS[key]


def _forced(model, prompts, K, temperature, **kw):
    choice = [(37 * i + 11) % 500 + 1 for i in range(20)]
    dfa = TokenDFA.from_choices([choice], 512, eos=[EOS]).to(DEV)
    total = len(choice) + 1
    model.stop_poll_steps = 1
    try:
        out, fin, state, stats = model.generate([prompts], num_return_sequences=3, max_new_tokens=total, temperature=temperature,
                                                eos_token_id=[EOS], constraint=dfa, draft_tokens=K, draft="constraint",
                                                return_constraint_state=True, return_finish=True, return_draft_stats=True, **kw)
    finally:
        del model.stop_poll_steps
    assert out.tolist() == [choice + [EOS]] * 6 and fin.lengths.tolist() == [total] * 6 and fin.reasons.tolist() == [1] * 6
    assert dfa.choice_of(state).tolist() == [0] * 6
    assert stats.steps == forced_steps(total, K), stats.steps
    emitting = stats.steps - 1
    assert stats.accepted.tolist() == stats.proposed.tolist() == stats.forced.tolist() == [total - 1 - emitting] * 6


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
def test_a_fully_forced_choice_is_accepted_whole_on_fp8_caches(monkeypatch, heads, kv_heads, K, temperature, graph):
    """Weights-independent and exact: one choice of 20 tokens + EOS, every state forced -- the output is the choice whatever the cache
    rounds, every draft is accepted, and the step count is the closed form of tests/test_constrained_drafts_gpu.py.  (4, 4) heads with
    K = 3 / 7 feed 4- / 8-row units, (8, 2) heads 16- / 32-row ones: the fp8 causal kernel takes all of them, nothing is dequantized."""
    model, prompts = fp8_model(heads, kv_heads, 115)
    torch.manual_seed(K)
    model.graph(graph)
    try:
        with monkeypatch.context() as m:
            _no_fallback(m)
            _forced(model, prompts, K, temperature)
    finally:
        model.graph(False)


def test_a_fully_forced_choice_with_calibrated_scales():
    """kv_scales="calibrate": the speculative loop's first write to the unique cache closes the scale window where the plain loop's does
    -- the scales are written once from the prompts' K / V, differ from 1, and the decode leaves them as they are."""
    model, prompts = fp8_model(8, 2, 81, kv_scales="calibrate")
    caches = [layer.self_attn.kv_cache for layer in model.model.layers]
    _forced(model, prompts, 3, 0.0)
    after = [(c.k_scale.clone(), c.v_scale.clone()) for c in caches]
    assert all(bool((k != 1).any()) and bool((v != 1).any()) for k, v in after)
    assert all(not c._scale_window for c in caches)
    # a second call on the same hierarchy's prompts calibrates to the same scales before its first write, and no step moves them:
    # plain decoding (no drafts) ends with the same values
    model.generate([prompts], num_return_sequences=3, max_new_tokens=8, temperature=0)
    plain = [(c.k_scale.clone(), c.v_scale.clone()) for c in caches]
    _forced(model, prompts, 7, 1.0)
    for c, (k0, v0), (k1, v1) in zip(caches, after, plain):
        assert torch.equal(c.k_scale, k0) and torch.equal(c.v_scale, v0) and torch.equal(k1, k0) and torch.equal(v1, v0)


def test_a_fully_forced_choice_through_the_assembled_route(monkeypatch):
    """use_fused_decode = False on fp8 caches: the torch RoPE + quantizing scatter, then speculative.assembled_causal_tail_attention on
    dequantize_kv of the cache rows (functional, not fast) -- and the same answer."""
    model, prompts = fp8_model(4, 4, 115)
    calls = []
    real = dequantize_kv
    import hydragen_amd.llama as L

    monkeypatch.setattr(L, "dequantize_kv", lambda *a, **k: calls.append(1) or real(*a, **k))
    for layer in model.model.layers:
        layer.self_attn.use_fused_decode = False
    try:
        _forced(model, prompts, 3, 0.0)
    finally:
        for layer in model.model.layers:
            layer.self_attn.use_fused_decode = True
    assert len(calls) >= 2 * 2 * 5  # two tensors, two layers, every multi-token step
