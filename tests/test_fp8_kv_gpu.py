"""-m gpu: fp8 (e4m3fn) unique K/V caches on the MI355X -- the fp8 token-row suffix kernel (csrc/suffix_attn_fp8.hip) against the
float64 oracle on the DEQUANTIZED caches (the widening is exact, so the 16-bit gates of gpu_util apply unchanged), the whole
operator with 16-bit shared levels, the fp8 RoPE + append kernel bit for bit against kv_quant.quantize_kv, graph capture, and the
dequantizing fallback of non-native shapes."""
import numpy as np
import pytest
import torch

from hydragen_amd import attention as A
from hydragen_amd.attention import hydragen_attention_nopad
from hydragen_amd.flash import flash_attention_seqlen, longest_first, seq_order
from hydragen_amd.fused_decode import rope_append_decode
from hydragen_amd.kv_quant import FP8_DTYPE, dequantize_kv, quantize_kv
from oracle import hydragen_oracle as O
from tests.gpu_util import TORCH_DT, assert_close_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _caches(rng, B, S, H, D, dt, scales=True, kstd=1.0):
    """fp8 caches quantized from random 16-bit values with distinct per-head scales (a head / scale mix-up fails)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(int(rng.integers(1 << 31)))
    k = (torch.randn((B, S, H, D), generator=g, device=DEV) * kstd).to(TORCH_DT[dt])
    v = torch.randn((B, S, H, D), generator=g, device=DEV).to(TORCH_DT[dt])
    ks = vs = None
    if scales:  # 4 significant bits: fp8 value x scale is exact in bf16 / f16, so the dequantized 16-bit caches are exact too
        ks = torch.from_numpy(((1 + rng.integers(0, 8, H) / 8) * 2.0 ** rng.integers(-3, 3, H)).astype(np.float32)).to(DEV)
        vs = torch.from_numpy(((1 + rng.integers(0, 8, H) / 8) * 2.0 ** rng.integers(-3, 3, H)).astype(np.float32)).to(DEV)
    return quantize_kv(k, ks), quantize_kv(v, vs), ks, vs


def _fp8_zeros(*shape):
    return torch.zeros(shape, dtype=torch.uint8, device=DEV).view(FP8_DTYPE)


def _rows(x8, idx):
    """sequences `idx` of an fp8 tensor (indexed as bytes)"""
    return x8.view(torch.uint8)[torch.as_tensor(idx, device=x8.device)].view(FP8_DTYPE)


def _deq(x8, s):
    return dequantize_kv(x8, s, torch.float32).cpu().numpy()


def _check_rows(got, want, dt, what):
    assert_close_l2(got, want, dt, what)


def _oracle_subset(q, k8, v8, ks, vs, sl, idx):
    """float64 oracle on the dequantized caches for the sequences `idx`."""
    qn = q.float().cpu().numpy()[idx]
    kn, vn = _deq(_rows(k8, idx), ks), _deq(_rows(v8, idx), vs)
    return O.flash_attention_seqlen(qn, kn, vn, sl[idx])


def _lens(rng, B, S):
    sl = rng.integers(1, min(S, 128) + 1, B).astype(np.int32)
    sl[: min(B, 3)] = [S, 1, 0][: min(B, 3)]
    return sl


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("hmul", [1, 2, 4])  # Hkv = the heads of one wave instruction (token split), 8, 32
@pytest.mark.parametrize("B", [1, 7, 1024])
def test_suffix_fp8_matches_oracle_on_dequantized_caches(dt, D, hmul, B):
    hpi = 64 // (D // 8)
    H = {1: hpi, 2: 8, 4: 32}[hmul]
    S = 160 if B < 1024 else 48
    rng = np.random.default_rng(D + 3 * hmul + B)
    k8, v8, ks, vs = _caches(rng, B, S, H, D, dt)
    q = torch.from_numpy(rng.standard_normal((B, 1, H, D)).astype(np.float32)).to(DEV, TORCH_DT[dt])
    sl = _lens(rng, B, S)
    out, lse = flash_attention_seqlen(q, k8, v8, torch.from_numpy(sl).to(DEV), k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    idx = np.unique(np.concatenate([np.arange(min(B, 3)), rng.integers(0, B, 12)]))
    want, wlse = _oracle_subset(q, k8, v8, ks, vs, sl, idx)
    got = out.float().cpu().numpy()[idx]
    has = sl[idx] > 0
    _check_rows(got[has], want[has], dt, f"fp8 suffix {dt} D={D} H={H} B={B}")
    gl = lse.cpu().numpy()[idx]
    assert np.all(np.isneginf(gl[~has])) and np.allclose(gl[has], wlse[has], atol=2e-3, rtol=1e-4)
    # the 16-bit kernel on the dequantized caches (scales folded into 16-bit values: one rounding each) agrees closely
    if ks is not None:
        ref, _ = flash_attention_seqlen(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), torch.from_numpy(sl).to(DEV))
        assert_close_l2(out.float().cpu().numpy(), ref.float().cpu().numpy(), dt, "fp8 vs 16-bit kernel")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_suffix_fp8_long_cache_unit_scales_int64_lengths(dt):
    rng = np.random.default_rng(11)
    B, S, H, D = 8, 2176, 32, 128
    k8, v8, _, _ = _caches(rng, B, S, H, D, dt, scales=False)
    q = torch.from_numpy(rng.standard_normal((B, 1, H, D)).astype(np.float32)).to(DEV, TORCH_DT[dt])
    sl = rng.integers(1, S + 1, B).astype(np.int64)
    sl[0], sl[1] = S, 2175
    out, _ = flash_attention_seqlen(q, k8, v8, torch.from_numpy(sl).to(DEV))
    idx = np.arange(6)
    want, _ = _oracle_subset(q, k8, v8, None, None, sl, idx)
    _check_rows(out.float().cpu().numpy()[idx], want, dt, "fp8 2176-row cache")


def test_suffix_fp8_seq_order_is_bit_identical():
    rng = np.random.default_rng(5)
    B, S, H, D = 1024, 128, 32, 128
    k8, v8, ks, vs = _caches(rng, B, S, H, D, "bf16")
    q = torch.from_numpy(rng.standard_normal((B, 1, H, D)).astype(np.float32)).to(DEV, torch.bfloat16)
    sl = torch.from_numpy(rng.integers(0, S + 1, B).astype(np.int32)).to(DEV)
    o0, l0 = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs)
    with seq_order(longest_first(sl)):
        o1, l1 = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


def _hier(rng, n_levels, B, H, D, dt, P=96):
    shared_ks, shared_vs = [], []
    for i in range(n_levels):
        sb = [1, 2, 4][i]
        shared_ks.append(torch.from_numpy(rng.standard_normal((sb, P - 16 * i, H, D)).astype(np.float32)).to(DEV, TORCH_DT[dt]))
        shared_vs.append(torch.from_numpy(rng.standard_normal((sb, P - 16 * i, H, D)).astype(np.float32)).to(DEV, TORCH_DT[dt]))
    return shared_ks, shared_vs


def _oracle_hier(q, k8, v8, ks, vs, sl, shared_ks, shared_vs):
    n = len(shared_ks)
    return O.hydragen_attention(q.float().cpu().numpy(), _deq(k8, ks), _deq(v8, vs), [x.float().cpu().numpy() for x in shared_ks],
                                [x.float().cpu().numpy() for x in shared_vs], [None] * n, [None] * n, [False] * n, sl)


@pytest.mark.parametrize("n_levels", [1, 2, 3])
@pytest.mark.parametrize("f32", [False, True])
def test_hydragen_attention_fp8_unique_with_shared_levels(n_levels, f32):
    rng = np.random.default_rng(n_levels * 10 + f32)
    B, S, H, D, dt = 16, 72, 8, 128, "bf16"
    k8, v8, ks, vs = _caches(rng, B, S, H, D, dt)
    q = torch.from_numpy(rng.standard_normal((B, 1, H, D)).astype(np.float32)).to(DEV, torch.bfloat16)
    sl = _lens(rng, B, S)
    shared_ks, shared_vs = _hier(rng, n_levels, B, H, D, dt)
    prev = A.set_f32_partials(f32)
    try:
        out = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, torch.from_numpy(sl).to(DEV), k_scale=ks, v_scale=vs)
        out2 = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, torch.from_numpy(sl).to(DEV), k_scale=ks, v_scale=vs)
    finally:
        A.set_f32_partials(prev)
    assert torch.equal(out, out2)  # (second call: the cached marshalled struct)
    want = _oracle_hier(q, k8, v8, ks, vs, sl, shared_ks, shared_vs)
    assert_close_l2(out.float().cpu().numpy(), want, dt, f"fp8 unique + {n_levels} shared levels")


def test_two_stream_matches_one_call_with_fp8_unique():
    rng = np.random.default_rng(3)
    B, S, H, D = 64, 64, 32, 128
    k8, v8, ks, vs = _caches(rng, B, S, H, D, "bf16")
    q = torch.from_numpy(rng.standard_normal((B, 1, H, D)).astype(np.float32)).to(DEV, torch.bfloat16)
    sl = torch.from_numpy(_lens(rng, B, S)).to(DEV)
    shared_ks, shared_vs = _hier(rng, 1, B, H, D, "bf16", P=256)
    one = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl, k_scale=ks, v_scale=vs)
    prev = A.set_two_stream("on")
    try:
        two = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl, k_scale=ks, v_scale=vs)
        torch.cuda.synchronize()
    finally:
        A.set_two_stream(prev)
    assert_close_l2(two.float().cpu().numpy(), one.float().cpu().numpy(), "bf16", "two-stream vs one call")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_rope_append_fp8_is_bit_identical_to_quantize_kv(dt, D):
    rng = np.random.default_rng(D)
    B, Hq, Hkv, S = 9, 8, 8, 40
    tdt = TORCH_DT[dt]
    q = torch.from_numpy(rng.standard_normal((B, 1, Hq, D)).astype(np.float32)).to(DEV, tdt)
    k = torch.from_numpy((rng.standard_normal((B, 1, Hkv, D)) * 300).astype(np.float32)).to(DEV, tdt)  # past 448 * scale too
    v = torch.from_numpy((rng.standard_normal((B, 1, Hkv, D)) * 100).astype(np.float32)).to(DEV, tdt)
    k[3, 0, 2, 5] = float("nan")  # NaN passes through the quantizer (RoPE spreads it to its rotation partner)
    v[4, 0, 1, 7] = float("nan")
    ang = np.arange(64)[:, None] * (1e4 ** (-np.arange(D // 2) / (D // 2)))[None]
    emb = np.concatenate([ang, ang], 1)
    cos = torch.from_numpy(np.cos(emb).astype(np.float32)).to(DEV)
    sin = torch.from_numpy(np.sin(emb).astype(np.float32)).to(DEV)
    pos = torch.from_numpy(rng.integers(8, 8 + S, (B, 1))).to(DEV)
    shared_len = torch.full((B,), 8, dtype=torch.int64, device=DEV)
    ks = torch.from_numpy((0.1 + rng.random(Hkv)).astype(np.float32)).to(DEV)
    vs = torch.from_numpy((0.1 + rng.random(Hkv)).astype(np.float32)).to(DEV)
    kc16 = torch.zeros((B, S, Hkv, D), dtype=tdt, device=DEV)
    vc16 = torch.zeros_like(kc16)
    kc8 = _fp8_zeros(B, S, Hkv, D)
    vc8 = _fp8_zeros(B, S, Hkv, D)
    q16, sl16 = rope_append_decode(q, k, v, cos, sin, pos, shared_len, kc16, vc16)
    q8, sl8 = rope_append_decode(q, k, v, cos, sin, pos, shared_len, kc8, vc8, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert torch.equal(q16, q8) and torch.equal(sl16, sl8)
    for c16, c8, sc in ((kc16, kc8, ks), (vc16, vc8, vs)):
        want = quantize_kv(c16, sc)
        nan = torch.isnan(c16)
        assert nan.any() and torch.equal(torch.isnan(c8.float()), nan)  # NaN exactly where the 16-bit cache has one
        assert torch.equal(want.view(torch.uint8)[~nan], c8.view(torch.uint8)[~nan])  # every other byte bit for bit
    assert (kc16.float().abs() / ks[:, None] > 448).any()  # saturation was exercised


def test_captured_decode_step_with_fp8_caches_equals_eager():
    rng = np.random.default_rng(8)
    B, S, H, D = 256, 96, 32, 128
    k8, v8, ks, vs = _caches(rng, B, S, H, D, "bf16")
    q = torch.from_numpy(rng.standard_normal((B, 1, H, D)).astype(np.float32)).to(DEV, torch.bfloat16)
    shared_ks, shared_vs = _hier(rng, 1, B, H, D, "bf16", P=128)
    sl = torch.from_numpy(rng.integers(1, 40, B).astype(np.int32)).to(DEV)
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


@pytest.mark.parametrize("shape", [dict(Hq=32, Hkv=8, nq=1, D=128), dict(Hq=8, Hkv=8, nq=2, D=128), dict(Hq=8, Hkv=8, nq=1, D=96),
                                   dict(Hq=2, Hkv=2, nq=1, D=128)])
def test_fallback_shapes_equal_existing_path_on_dequantized_caches(shape):
    rng = np.random.default_rng(shape["Hkv"] + shape["D"])
    B, S, dt = 6, 50, "bf16"
    Hq, Hkv, nq, D = shape["Hq"], shape["Hkv"], shape["nq"], shape["D"]
    k8, v8, ks, vs = _caches(rng, B, S, Hkv, D, dt)
    q = torch.from_numpy(rng.standard_normal((B, nq, Hq, D)).astype(np.float32)).to(DEV, torch.bfloat16)
    sl = torch.from_numpy(_lens(rng, B, S)).to(DEV)
    kd, vd = dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype)
    o8, l8 = flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs)
    o16, l16 = flash_attention_seqlen(q, kd, vd, sl)
    assert torch.equal(o8, o16) and torch.equal(l8, l16)
    shared_ks, shared_vs = _hier(rng, 1, B, Hkv, D, dt)
    h8 = hydragen_attention_nopad(q, k8, v8, shared_ks, shared_vs, sl, k_scale=ks, v_scale=vs)
    h16 = hydragen_attention_nopad(q, kd, vd, shared_ks, shared_vs, sl)
    assert torch.equal(h8, h16)


# ---- the model shell with fp8 unique caches ---------------------------------------------------------------------------------
def _model(dtype=torch.bfloat16, kv_heads=4, head_dim=128, layers=2, seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=4 * head_dim, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=4,
                      num_key_value_heads=kv_heads, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=DEV, seed=seed, std=0.05)


def _gen(model, kv, graph, disable_hydragen=False, nret=8, new=8, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    prefix = torch.randint(1, 512, (1, 40), device=DEV, generator=g)
    overrides = torch.randint(1, 512, (nret, new), device=DEV, generator=g)
    model.graph(graph)
    model.setup_caches(max_unique_batch_size=nret, max_unique_seq_length=64 + 16, max_shared_batch_sizes=[1],
                       max_shared_seq_lengths=[40], kv_cache_dtype=kv)
    return model.generate(input_ids=prefix, num_return_sequences=nret, max_new_tokens=new, temperature=0.0, return_logits=True,
                          token_overrides=overrides, disable_hydragen=disable_hydragen)


def test_model_fp8_arenas_are_half_the_bytes_with_unit_scales():
    model = _model()
    nbytes = {}
    for kv in (None, FP8_DTYPE):
        model.setup_caches(max_unique_batch_size=8, max_unique_seq_length=64, max_shared_batch_sizes=[1], max_shared_seq_lengths=[40],
                           kv_cache_dtype=kv)
        c = model.model.layers[0].self_attn.kv_cache
        nbytes[kv] = c.per_completion_k_cache.untyped_storage().nbytes()
        assert c.per_completion_k_cache.dtype == (FP8_DTYPE if kv else torch.bfloat16)
        assert c.shared_caches[0].k_cache.dtype == torch.bfloat16  # shared caches stay 16-bit
        if kv:
            assert torch.equal(c.k_scale, torch.ones(4, device=DEV)) and torch.equal(c.v_scale, torch.ones(4, device=DEV))
            assert int(c.per_completion_k_cache.view(torch.uint8).count_nonzero()) == 0
        else:
            assert c.k_scale is None
    assert nbytes[FP8_DTYPE] * 2 == nbytes[None]
    with pytest.raises(NotImplementedError):
        model.setup_caches(max_unique_batch_size=8, max_unique_seq_length=64, max_shared_batch_sizes=[1], max_shared_seq_lengths=[40],
                           kv_cache_dtype=torch.float16)


# relative L2 of the decode steps' logits, fp8 against bf16 unique caches (same weights, same forced tokens).  Measured with these
# seeds: first decode step 1.5e-2 (4 kv heads, native kernel) / 1.2e-2 (2 kv heads, fallback), all 7 decode steps 2.0e-2 / 1.9e-2;
# only the generated tokens sit in the fp8 cache.  The no-sharing mode quantizes the whole 40-token prompt too: 7.1e-2, the error
# of attention over fp8 keys of tests/test_fp8_kv.py.
FP8_LOGITS_REL_L2 = 0.05
FP8_LOGITS_REL_L2_NO_SHARING = 0.12


@pytest.mark.parametrize("kv_heads", [4, 2])  # 4: the native fp8 kernel; 2: grouped-query heads through the dequantizing fallback
def test_model_fp8_greedy_tokens_graph_on_off_and_logits_vs_bf16(kv_heads):
    model = _model(kv_heads=kv_heads)
    out_g, lg_g = _gen(model, FP8_DTYPE, graph=True)
    out_e, lg_e = _gen(model, FP8_DTYPE, graph=False)
    assert torch.equal(out_g, out_e)
    _, lg_b = _gen(model, None, graph=True)
    a, b = torch.stack(lg_g[1:]).float(), torch.stack(lg_b[1:]).float()  # decode steps (logits[0]: after the shared prefill)
    l2 = float((a - b).norm() / b.norm())
    first = float((lg_g[1].float() - lg_b[1].float()).norm() / lg_b[1].float().norm())
    print(f"fp8 vs bf16 logits, kv_heads={kv_heads}: first decode step relative L2 {first:.2e}, all decode steps {l2:.2e}")
    assert first <= FP8_LOGITS_REL_L2 and l2 <= FP8_LOGITS_REL_L2
    assert torch.equal(lg_g[0], lg_b[0])  # the shared prefill reads no unique cache


def test_model_fp8_no_sharing_mode_quantizes_the_copied_prefix():
    """disable_hydragen: copy_shared_to_unique quantizes the prefix into the fp8 arena, the unique prefill reads it dequantized."""
    model = _model()
    _, lg8 = _gen(model, FP8_DTYPE, graph=False, disable_hydragen=True)
    _, lg16 = _gen(model, None, graph=False, disable_hydragen=True)
    a, b = torch.stack(lg8[1:]).float(), torch.stack(lg16[1:]).float()
    assert float((a - b).norm() / b.norm()) <= FP8_LOGITS_REL_L2_NO_SHARING


def test_placement_probes_fp8_arenas_with_the_fp8_kernel():
    from hydragen_amd import placement

    prev = placement.set_candidates(3)
    try:
        shape = (2048, 256, 4, 128)  # 512 MiB of fp8 per arena: large enough to be placed
        arenas, rep = placement.place_kv_arenas(2, shape, FP8_DTYPE, DEV, 4, q_dtype=torch.bfloat16)
    finally:
        placement.set_candidates(prev)
    assert rep["probed"] is True or rep.get("why", "").startswith("not enough free memory"), rep
    if rep.get("probed"):
        assert len(rep["probe_us"]) > 2 and all(t > 0 for t in rep["probe_us"])
    for a in arenas:
        assert a.dtype == FP8_DTYPE and tuple(a.shape) == (2,) + shape
        assert int(a.view(torch.uint8).count_nonzero()) == 0
    del arenas
    torch.cuda.empty_cache()
    # and through the model: several candidates, fp8 arenas
    model = _model(layers=1)
    prev = placement.set_candidates(3)
    try:
        model.setup_caches(max_unique_batch_size=2048, max_unique_seq_length=256, max_shared_batch_sizes=[1],
                           max_shared_seq_lengths=[40], kv_cache_dtype=FP8_DTYPE)
    finally:
        placement.set_candidates(prev)
    assert model.model.layers[0].self_attn.kv_cache.per_completion_k_cache.dtype == FP8_DTYPE
    assert model.kv_placement.get("probed") is True or "memory" in model.kv_placement.get("why", ""), model.kv_placement
