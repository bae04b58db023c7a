"""-m gpu: fp8 (e4m3fn) unique K/V caches on grouped-query heads -- the fp8 matrix-core suffix kernel (csrc/suffix_attn_gqa_fp8.hip).
Its contract: `out` and `lse` are BIT-IDENTICAL to the 16-bit grouped-query kernel run on dequantize_kv(k8, k_scale, q dtype) /
dequantize_kv(v8, v_scale, q dtype).  Every fp8 call here runs with flash.dequantize_kv patched to raise, so a silent fallback to the
16-bit path fails the test instead of passing it."""
import ctypes as C

import numpy as np
import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd import attention as A
from hydragen_amd import flash as F
from hydragen_amd import placement
from hydragen_amd.attention import hydragen_attention_nopad
from hydragen_amd.flash import flash_attention_seqlen, longest_first, seq_order
from hydragen_amd.kv_quant import FP8_DTYPE, dequantize_kv
from oracle import hydragen_oracle as O
from tests.gpu_util import TORCH_DT, assert_close_l2
from tests.test_fp8_kv_gpu import FP8_LOGITS_REL_L2, _caches, _hier, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, Hq, Hkv, nq, D, S)
SHAPES = {
    "4-heads-per-workgroup": (128, 32, 8, 1, 128, 96),
    "D64-two-tile-sets": (256, 8, 2, 1, 64, 96),
    "D256": (2048, 8, 1, 1, 256, 40),
    "1-head-per-workgroup": (1024, 8, 1, 1, 128, 70),
    "four-waves-per-unit": (4, 8, 2, 1, 128, 160),
    "3-row-units": (64, 12, 4, 1, 128, 50),
    "two-16-row-chunks": (64, 20, 1, 1, 128, 50),
    "nq2": (64, 8, 2, 2, 128, 50),
}


def _no_fallback(monkeypatch):
    def raiser(*a, **k):
        raise AssertionError("dequantize_kv reached: the fp8 call fell back to the 16-bit path")

    monkeypatch.setattr(F, "dequantize_kv", raiser)


def _lens(rng, B, S, dtype=np.int32):
    sl = rng.integers(0, S + 1, B).astype(dtype)
    edge = [x for x in (0, 1, 31, 32, 33, 64, 65, S) if x <= S]
    sl[: min(B, len(edge))] = edge[:B]
    if B < len(edge):
        sl[-1] = S
    return sl


def _poison(x8, sl):
    """rows at and past each sequence's length hold the fp8 NaN byte"""
    S = x8.shape[1]
    past = torch.arange(S, device=DEV)[None, :] >= torch.as_tensor(sl.astype(np.int64), device=DEV)[:, None]
    x8.view(torch.uint8)[past] = 0x7F
    return x8


def _problem(rng, shape, dt, scales="caches", len_dtype=np.int32):
    B, Hq, Hkv, nq, D, S = shape
    k8, v8, ks, vs = _caches(rng, B, S, Hkv, D, dt, scales=scales == "caches")
    if scales == "arbitrary":  # products that do not fit the 16-bit formats: the rounding of the widening itself
        ks = torch.from_numpy((0.1 + rng.random(Hkv)).astype(np.float32)).to(DEV)
        vs = torch.from_numpy((0.1 + rng.random(Hkv)).astype(np.float32)).to(DEV)
    q = torch.from_numpy(rng.standard_normal((B, nq, Hq, D)).astype(np.float32)).to(DEV, TORCH_DT[dt])
    sl = _lens(rng, B, S, len_dtype)
    return q, _poison(k8, sl), _poison(v8, sl), ks, vs, sl


def _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl_t, what):
    kd, vd = dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype)
    o16, l16 = flash_attention_seqlen(q, kd, vd, sl_t)
    with monkeypatch.context() as m:
        _no_fallback(m)
        o8, l8 = flash_attention_seqlen(q, k8, v8, sl_t, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert not torch.isnan(o8).any(), what
    assert torch.equal(o8, o16), (what, int((o8 != o16).sum()))
    assert torch.equal(l8, l16), (what, int((l8 != l16).sum()))
    return o8, l8


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp8_gqa_is_bit_identical_to_16bit_kernel_on_dequantized_caches(monkeypatch, name, dt):
    for i, scales in enumerate(("caches", "arbitrary", None)):
        rng = np.random.default_rng(len(name) * 7 + i)
        q, k8, v8, ks, vs, sl = _problem(rng, SHAPES[name], dt, scales)
        _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, torch.from_numpy(sl).to(DEV), f"{name} {dt} scales={scales}")


def test_fp8_gqa_int64_lengths(monkeypatch):
    rng = np.random.default_rng(64)
    q, k8, v8, ks, vs, sl = _problem(rng, SHAPES["4-heads-per-workgroup"], "bf16", "arbitrary", np.int64)
    _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, torch.from_numpy(sl).to(DEV), "int64 lengths")


def test_fp8_gqa_on_a_kv_arena(monkeypatch):
    """the model's layout: a sequence's V rows behind its K rows in one allocation (placement.kv_arena), strides in bytes"""
    rng = np.random.default_rng(65)
    shape = SHAPES["3-row-units"]
    B, Hq, Hkv, nq, D, S = shape
    q, k8, v8, ks, vs, sl = _problem(rng, shape, "f16", "arbitrary")
    arena = placement.kv_arena((B, S, Hkv, D), FP8_DTYPE, DEV)
    arena[0].view(torch.uint8).copy_(k8.view(torch.uint8))
    arena[1].view(torch.uint8).copy_(v8.view(torch.uint8))
    assert arena[0].stride(0) == 2 * S * Hkv * D
    o, _ = _assert_bit_identical(monkeypatch, q, arena[0], arena[1], ks, vs, torch.from_numpy(sl).to(DEV), "kv_arena")
    o2, _ = flash_attention_seqlen(q, k8, v8, torch.from_numpy(sl).to(DEV), k_scale=ks, v_scale=vs)
    assert torch.equal(o, o2)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(SHAPES)[:3])
def test_fp8_gqa_matches_oracle_on_dequantized_caches(monkeypatch, name, dt):
    rng = np.random.default_rng(len(name))
    q, k8, v8, ks, vs, sl = _problem(rng, SHAPES[name], dt, "arbitrary")
    B = q.shape[0]
    with monkeypatch.context() as m:
        _no_fallback(m)
        out, lse = flash_attention_seqlen(q, k8, v8, torch.from_numpy(sl).to(DEV), k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    idx = np.unique(np.concatenate([np.arange(8), rng.integers(0, B, 6)]))
    # the oracle reads what the kernel's MFMAs read: the caches as dequantize_kv widens them to the q dtype (poisoned rows are past
    # the lengths: zeroed for numpy, which would multiply them by zero weights)
    kn = dequantize_kv(_rows(k8, idx), ks, q.dtype).float().nan_to_num(0.0).cpu().numpy()
    vn = dequantize_kv(_rows(v8, idx), vs, q.dtype).float().nan_to_num(0.0).cpu().numpy()
    want, wlse = O.flash_attention_seqlen(q.float().cpu().numpy()[idx], kn, vn, sl[idx])
    has = sl[idx] > 0
    assert_close_l2(out.float().cpu().numpy()[idx][has], want[has], dt, f"fp8 gqa {name} {dt}")
    gl = lse.cpu().numpy()[idx]
    assert np.all(np.isneginf(gl[~has])) and np.allclose(gl[has], wlse[has], atol=2e-3, rtol=1e-4)


def test_fp8_gqa_seq_order_is_bit_identical(monkeypatch):
    rng = np.random.default_rng(5)
    q, k8, v8, ks, vs, sl = _problem(rng, SHAPES["1-head-per-workgroup"], "bf16")
    sl = torch.from_numpy(sl).to(DEV)
    _no_fallback(monkeypatch)
    o0, l0 = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs)
    with seq_order(longest_first(sl)):
        o1, l1 = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


# ---- the whole operator ---------------------------------------------------------------------------------------------------------
def _operator_case(rng, n_levels, P=96, B=128, dt="bf16", S=96):
    Hq, Hkv, D = 32, 8, 128
    q, k8, v8, ks, vs, sl = _problem(rng, (B, Hq, Hkv, 1, D, S), dt, "arbitrary")
    shared_ks, shared_vs = _hier(rng, n_levels, B, Hkv, D, dt, P=P)
    return q, k8, v8, ks, vs, sl, shared_ks, shared_vs


def _operator_check(monkeypatch, case, what, oracle_rows=6):
    q, k8, v8, ks, vs, sl, shared_ks, shared_vs = case
    sl_t = torch.from_numpy(sl).to(DEV)
    h16 = hydragen_attention_nopad(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), shared_ks, shared_vs, sl_t)
    with monkeypatch.context() as m:
        _no_fallback(m)
        h8 = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl_t, k_scale=ks, v_scale=vs)
        h8b = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl_t, k_scale=ks, v_scale=vs)  # (the cached struct)
    torch.cuda.synchronize()
    assert torch.equal(h8, h16) and torch.equal(h8b, h16), what
    # float64 oracle for the first sequences (they sit in group 0 of every level) on what the MFMAs read: the caches as
    # dequantize_kv widens them (poisoned rows are past the lengths: zeroed for numpy, which would multiply them by zero weights)
    idx = list(range(oracle_rows))
    kz = dequantize_kv(_rows(k8, idx), ks, q.dtype).float().nan_to_num(0.0).cpu().numpy()
    vz = dequantize_kv(_rows(v8, idx), vs, q.dtype).float().nan_to_num(0.0).cpu().numpy()
    n = len(shared_ks)
    want = O.hydragen_attention(q[:oracle_rows].float().cpu().numpy(), kz, vz, [x[:1].float().cpu().numpy() for x in shared_ks],
                                [x[:1].float().cpu().numpy() for x in shared_vs], [None] * n, [None] * n, [False] * n, sl[:oracle_rows])
    assert_close_l2(h8.float().cpu().numpy()[:oracle_rows], want, "bf16", what)


@pytest.mark.parametrize("n_levels", [1, 2, 3])
@pytest.mark.parametrize("f32", [False, True])
def test_hydragen_attention_fp8_gqa_equals_dequantized_call(monkeypatch, n_levels, f32):
    rng = np.random.default_rng(n_levels * 10 + f32)
    case = _operator_case(rng, n_levels)
    prev = A.set_f32_partials(f32)
    try:
        _operator_check(monkeypatch, case, f"fp8 gqa unique + {n_levels} levels, f32 partials {f32}")
    finally:
        A.set_f32_partials(prev)


def _planned_splits(B, Hq, Hkv, D, P, tok_stride):
    pp = _lib.PrefixParams()
    pp.dtype, pp.B, pp.nq, pp.Hq, pp.Hkv, pp.D, pp.sb, pp.kv_len = _lib.HYD_BF16, B, 1, Hq, Hkv, D, 1, P
    pp.k_tok_stride = pp.v_tok_stride = tok_stride
    ns = C.c_int32()
    _lib.check(_lib.load().hyd_prefix_plan(C.byref(pp), C.byref(ns), None, None))
    return ns.value


def test_hydragen_attention_fp8_gqa_with_a_split_level(monkeypatch):
    B, Hq, Hkv, D = 128, 32, 8, 128
    P = next((p for p in (2048, 8192, 32768) if _planned_splits(B, Hq, Hkv, D, p, Hkv * D) > 1), None)
    assert P is not None, "the planner splits none of the candidate levels"
    rng = np.random.default_rng(77)
    q, k8, v8, ks, vs, sl, _, _ = _operator_case(rng, 1)
    sk = torch.randn((1, P, Hkv, D), device=DEV).to(torch.bfloat16)
    sv = torch.randn((1, P, Hkv, D), device=DEV).to(torch.bfloat16)
    _operator_check(monkeypatch, (q, k8, v8, ks, vs, sl, [sk], [sv]), f"fp8 gqa unique + a split level of {P} keys", oracle_rows=3)


def test_hydragen_attention_fp8_gqa_two_stream(monkeypatch):
    rng = np.random.default_rng(3)
    case = _operator_case(rng, 1, P=256)
    prev = A.set_two_stream("on")
    try:
        _operator_check(monkeypatch, case, "fp8 gqa unique, two-stream form")
    finally:
        A.set_two_stream(prev)


def test_tiny_grouped_query_calls_keep_the_fallback(monkeypatch):
    """B = 6 with 50 own keys on a 96-key prefix runs as ONE launch with 16-bit caches: the fp8 call is refused by the library and dequantized here,
    so its result stays the one-launch form's."""
    rng = np.random.default_rng(9)
    q, k8, v8, ks, vs, sl, shared_ks, shared_vs = _operator_case(rng, 1, B=6, S=50)
    sl_t = torch.from_numpy(sl).to(DEV)
    h16 = hydragen_attention_nopad(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), shared_ks, shared_vs, sl_t)
    calls = []
    real = F.dequantize_kv
    monkeypatch.setattr(F, "dequantize_kv", lambda *a, **k: [calls.append(1), real(*a, **k)][1])
    for _ in range(2):  # (second call: the cached refusal)
        h8 = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl_t, k_scale=ks, v_scale=vs)
        assert torch.equal(h8, h16)
    assert len(calls) == 4


def test_captured_fp8_gqa_step_equals_eager(monkeypatch):
    rng = np.random.default_rng(8)
    q, k8, v8, ks, vs, sl, shared_ks, shared_vs = _operator_case(rng, 1, P=128)
    # (nothing poisoned: the lengths grow between the replays)
    k8, v8, ks, vs = _caches(rng, 128, 96, 8, 128, "bf16")
    sl = torch.from_numpy(rng.integers(1, 40, 128).astype(np.int32)).to(DEV)
    _no_fallback(monkeypatch)
    step = lambda: hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl, k_scale=ks, v_scale=vs)  # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = step()
    for t in range(3):
        sl.add_(7 * t)
        ks.mul_(1.25)  # scales are read at replay time, like the lengths
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, step()), t


# ---- the model shell ----------------------------------------------------------------------------------------------------------
def _model(seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=8 * 128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=seed, std=0.05)


def _gen(model, kv, graph, nret=64, new=8, seed=5):
    # 64 sequences x 2 kv heads x (40 + 80) keys: more than the one-launch form of tiny calls takes, so the step is the kernel pair
    g = torch.Generator(device=DEV).manual_seed(seed)
    prefix = torch.randint(1, 512, (1, 40), device=DEV, generator=g)
    overrides = torch.randint(1, 512, (nret, new), device=DEV, generator=g)
    model.graph(graph)
    model.setup_caches(max_unique_batch_size=nret, max_unique_seq_length=64 + 16, max_shared_batch_sizes=[1],
                       max_shared_seq_lengths=[40], kv_cache_dtype=kv)
    return model.generate(input_ids=prefix, num_return_sequences=nret, max_new_tokens=new, temperature=0.0, return_logits=True,
                          token_overrides=overrides)


def test_model_fp8_gqa_decodes_on_the_fp8_kernel(monkeypatch):
    model = _model()
    _, lg_b = _gen(model, None, graph=True)
    with monkeypatch.context() as m:
        _no_fallback(m)  # (the shared prefill reads no unique cache: nothing may reach the fallback at all)
        out_g, lg_g = _gen(model, FP8_DTYPE, graph=True)
        out_e, lg_e = _gen(model, FP8_DTYPE, graph=False)
    assert torch.equal(out_g, out_e)
    a, b = torch.stack(lg_g[1:]).float(), torch.stack(lg_b[1:]).float()
    l2 = float((a - b).norm() / b.norm())
    print(f"fp8 vs bf16 logits, 8 q / 2 kv heads: all decode steps relative L2 {l2:.2e}")
    assert l2 <= FP8_LOGITS_REL_L2
    assert torch.equal(lg_g[0], lg_b[0])
