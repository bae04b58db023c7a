"""-m gpu: the per-head q/k RMSNorm inside the RoPE + append kernels (rope_append.hip: hyd_rope_append_decode_qkn,
hyd_rope_append_multi_qkn) held to the float64 definition and the derived bound of tests/qk_norm_ref.py, and a Qwen3-style model
(LlamaConfig.head_dim / qk_norm) held to transformers' recorded logits (tests/golden/qwen3_tiny.npz) and to its own unfused path.

Every cache is pre-filled with a sentinel and compared WHOLE: what the call may not touch is bit-identical afterwards."""
import numpy as np
import pytest
import torch

from hydragen_amd.fused_decode import rope_append_decode, rope_append_multi
from hydragen_amd.kv_quant import FP8_DTYPE, quantize_kv
from tests import glue_ref as R
from tests import qk_norm_ref as N
from tests import qwen3_golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
MAX_POS, L = 48, 12  # table rows, cache length


def rdiff(a, b, eps=1e-8):
    return 2 * (a - b).abs() / (a.abs() + b.abs() + eps)


_TABLES = {}


def tables(D):
    if D not in _TABLES:
        _TABLES[D] = N.rotary_tables(D, MAX_POS)
    return _TABLES[D]


def _positions(B, bad=()):
    """pos, shared int64 [B]: cache indices that cover 0 and L - 1 at table rows spread over the table.  bad: {row: index} overrides."""
    idx = (np.arange(B) * 5 + (L - 1)) % L
    if B > 1:
        idx[-1] = 0
    for b, i in dict(bad).items():
        idx[b] = i
    shared = (np.arange(B) * 7 + 3) % (MAX_POS - L)
    return torch.from_numpy(idx + shared), torch.from_numpy(shared), idx


def _dev_inputs(q, k, v, fused):
    """Device q / k / v [B, 1, H, D]: three tensors, or views into one fused projection buffer (non-trivial batch strides)."""
    B, Hq, D = q.shape
    Hkv = k.shape[1]
    if not fused:
        return q[:, None].to(DEV), k[:, None].to(DEV), v[:, None].to(DEV)
    qkv = torch.cat([q.reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)], 1).to(DEV)[:, None]
    return (qkv[..., : Hq * D].view(B, 1, Hq, D), qkv[..., Hq * D: (Hq + Hkv) * D].view(B, 1, Hkv, D),
            qkv[..., (Hq + Hkv) * D:].view(B, 1, Hkv, D))


def _run_one_token(dtype, D, B, Hq, Hkv, eps, fused=False, bad=(), fp8=None, seed=0):
    """One hyd_rope_append_decode_qkn call on N.make_inputs; returns everything the checks need (host copies)."""
    q, k, v, qw, kw = N.make_inputs(dtype, B, Hq, Hkv, D, seed)
    cos, sin = tables(D)
    pos, shared, idx = _positions(B, bad)
    qd, kd, vd = _dev_inputs(q, k, v, fused)
    if fp8 is None:
        kc0, vc0 = R.sentinel16((B + 1, L, Hkv, D), dtype, 1), R.sentinel16((B + 1, L, Hkv, D), dtype, 2)
        kc, vc, sc = kc0.to(DEV), vc0.to(DEV), {}
    else:
        kc0, vc0 = R.sentinel8((B + 1, L, Hkv, D), 1), R.sentinel8((B + 1, L, Hkv, D), 2)
        kc, vc = kc0.to(DEV).view(FP8_DTYPE), vc0.to(DEV).view(FP8_DTYPE)
        ks, vs = R.fp8_scales(fp8, Hkv)
        sc = {} if ks is None else dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    qo, sl = rope_append_decode(qd, kd, vd, cos.to(DEV), sin.to(DEV), pos[:, None].to(DEV), shared.to(DEV), kc, vc,
                                q_norm=qw.to(DEV), k_norm=kw.to(DEV), norm_eps=eps, **sc)
    torch.cuda.synchronize()
    return dict(q=q, k=k, v=v, qw=qw, kw=kw, cos=cos.numpy()[pos.numpy()], sin=sin.numpy()[pos.numpy()], idx=idx, qo=qo[:, 0].cpu(), sl=sl.cpu(),
                kc=kc.cpu(), vc=vc.cpu(), kc0=kc0, vc0=vc0)


def _within(got, want, bound, what):
    err = np.abs(got.double().numpy() - want)
    assert np.isfinite(got.float().numpy()).all(), what + ": not finite"
    worst = float((err / bound).max())
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements outside the bound, worst error / bound = {worst:.3g}"


# ---- the kernel against the float64 definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("B, Hq, Hkv, fused, eps", [(3, 5, 1, False, 1e-6), (37, 8, 2, True, 1e-5)], ids=["ragged-3x5x1", "fused-37x8x2"])
def test_norm_preamble_against_float64(dtype, D, B, Hq, Hkv, fused, eps):
    """B = 3, 5 / 1 heads: seven rows per sequence -- at D = 64 the last wave has 20 live lanes and one wave mixes q, k and v rows of
    two sequences.  B = 37, 8 / 2 heads: q / k / v are views into one fused projection buffer."""
    r = _run_one_token(dtype, D, B, Hq, Hkv, eps, fused)
    want_q, nq = N.qk_norm_rope_ref64(N.f64(r["q"]), N.f64(r["qw"]), eps, r["cos"], r["sin"])
    want_k, nk = N.qk_norm_rope_ref64(N.f64(r["k"]), N.f64(r["kw"]), eps, r["cos"], r["sin"])
    _within(r["qo"], want_q, N.qk_norm_rope_bound(want_q, nq, dtype), "q_out")
    bi = torch.arange(B)
    idx = torch.from_numpy(r["idx"])
    _within(r["kc"][bi, idx], want_k, N.qk_norm_rope_bound(want_k, nk, dtype), "K rows")
    # the all-zero heads: exact zeros, and the single-element head is +-sqrt(D) * w rotated (inside the bound above, and non-zero)
    assert not r["qo"][0, Hq - 1].float().any() and not r["kc"][B - 1, idx[B - 1], Hkv - 1].float().any()
    assert r["qo"][B - 1, 0].float().abs().max() > 0
    if dtype == torch.float16:
        assert r["q"][B // 2, min(1, Hq - 1)].float().abs().min() > 5e4  # the head whose squares overflow f16
    # untouched memory: v rows copied bit for bit, every other cache row as it was
    assert torch.equal(r["sl"], (idx + 1).int())
    assert torch.equal(R.bits(r["vc"][bi, idx]), R.bits(r["v"]))
    for got, before in ((r["kc"], r["kc0"]), (r["vc"], r["vc0"])):
        before = before.clone()
        before[bi, idx] = got[bi, idx]
        assert torch.equal(R.bits(got), R.bits(before))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fp8", [None, "mixed"], ids=["16bit", "fp8"])
def test_rows_outside_the_cache_write_no_kv_but_their_q(dtype, fp8):
    """A row at position shared_len - 1 (index -1) and one at index cache_len: no K / V byte changes, q_out is written, seq_lens
    still reports index + 1 (0 for the retired row)."""
    B, Hq, Hkv, D, eps = 4, 5, 1, 64, 1e-6
    r = _run_one_token(dtype, D, B, Hq, Hkv, eps, bad={1: -1, 2: L}, fp8=fp8)
    want_q, nq = N.qk_norm_rope_ref64(N.f64(r["q"]), N.f64(r["qw"]), eps, r["cos"], r["sin"])
    _within(r["qo"], want_q, N.qk_norm_rope_bound(want_q, nq, dtype), "q_out")
    assert r["sl"].tolist() == [int(i) + 1 for i in r["idx"]] and r["sl"][1] == 0 and r["sl"][2] == L + 1
    for got, before in ((r["kc"], r["kc0"]), (r["vc"], r["vc0"])):
        got = got.view(torch.uint8) if fp8 else got
        for b in (1, 2, B):
            assert torch.equal(R.bits(got[b]), R.bits(before[b])), b
        for b in (0, 3):
            assert not torch.equal(R.bits(got[b, r["idx"][b]]), R.bits(before[b, r["idx"][b]]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("scales", ["mixed", "none"])
def test_fp8_caches_hold_quantize_kv_of_the_16bit_run(dtype, D, scales):
    B, Hq, Hkv, eps = 5, 4, 2, 1e-5
    a = _run_one_token(dtype, D, B, Hq, Hkv, eps)
    b = _run_one_token(dtype, D, B, Hq, Hkv, eps, fp8=scales)
    assert torch.equal(R.bits(a["qo"]), R.bits(b["qo"])) and torch.equal(a["sl"], b["sl"])
    ks, vs = R.fp8_scales(scales, Hkv)
    bi, idx = torch.arange(B), torch.from_numpy(a["idx"])
    want_k, want_v = b["kc0"].clone(), b["vc0"].clone()
    want_k[bi, idx] = quantize_kv(a["kc"][bi, idx], ks).view(torch.uint8)
    want_v[bi, idx] = quantize_kv(a["v"], vs).view(torch.uint8)
    assert torch.equal(b["kc"].view(torch.uint8), want_k) and torch.equal(b["vc"].view(torch.uint8), want_v)


# ---- the multi-token kernel: the one-token kernel's bits -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [2, 8])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_multi_token_rows_equal_the_one_token_kernel(dtype, T, D):
    B, Hq, Hkv, eps = 3, 5, 1, 1e-6
    cos, sin = (t.to(DEV) for t in tables(D))
    toks = [N.make_inputs(dtype, B, Hq, Hkv, D, seed=10 + i) for i in range(T)]
    qw, kw = toks[0][3].to(DEV), toks[0][4].to(DEV)
    q, k, v = (torch.stack([t[j] for t in toks], 1).to(DEV) for j in range(3))  # [B, T, H, D]
    idx0 = np.array([2, -1, 0])  # row 1 is retired: position shared_len - 1
    shared = torch.tensor([5, 9, 11])
    pos = torch.from_numpy(idx0) + shared
    kc0, vc0 = R.sentinel16((B + 1, L, Hkv, D), dtype, 3), R.sentinel16((B + 1, L, Hkv, D), dtype, 4)
    kc, vc = kc0.to(DEV), vc0.to(DEV)
    qo, sl = rope_append_multi(q, k, v, cos, sin, pos.to(DEV), shared.to(DEV), kc, vc, q_norm=qw, k_norm=kw, norm_eps=eps)
    torch.cuda.synchronize()
    assert sl.tolist() == [2 + T, 0, T]
    want_k, want_v = kc0.clone(), vc0.clone()
    for i in range(T):
        k1, v1 = kc0.to(DEV), vc0.to(DEV)
        q1, _ = rope_append_decode(q[:, i:i + 1].contiguous(), k[:, i:i + 1].contiguous(), v[:, i:i + 1].contiguous(), cos, sin,
                                   (pos + i)[:, None].to(DEV), shared.to(DEV), k1, v1, q_norm=qw, k_norm=kw, norm_eps=eps)
        assert torch.equal(R.bits(qo[:, i]), R.bits(q1[:, 0])), i
        for b in (0, 2):  # the retired row's later tokens have index >= 0 in the one-token form: only its q is compared
            want_k[b, idx0[b] + i], want_v[b, idx0[b] + i] = k1[b, idx0[b] + i].cpu(), v1[b, idx0[b] + i].cpu()
            assert torch.equal(R.bits(want_v[b, idx0[b] + i]), R.bits(v[b, i].cpu()))
    assert torch.equal(R.bits(kc.cpu()), R.bits(want_k)) and torch.equal(R.bits(vc.cpu()), R.bits(want_v))
    assert torch.equal(R.bits(kc.cpu()[1]), R.bits(kc0[1]))  # none of the retired row's T rows


def test_python_faces_refuse_what_the_kernels_do_not_take():
    D = 96
    q = torch.zeros(2, 1, 4, D, dtype=torch.float16, device=DEV)
    kc = torch.zeros(2, 16, 4, D, dtype=torch.float16, device=DEV)
    cos, sin = (t.to(DEV) for t in N.rotary_tables(D, 8))
    w = torch.ones(D, dtype=torch.float16, device=DEV)
    pos = torch.zeros(2, 1, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="head_dim 96"):
        rope_append_decode(q, q, q, cos, sin, pos, None, kc, kc.clone(), q_norm=w, k_norm=w, norm_eps=1e-6)
    with pytest.raises(ValueError, match="both"):
        rope_append_decode(q, q, q, cos, sin, pos, None, kc, kc.clone(), q_norm=w, norm_eps=1e-6)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def tiny_model(dtype):
    """The model of tests/qwen3_golden.py in the shell, weights from its seed (exact in both 16-bit dtypes)."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    m = HydragenLlamaForCausalLM(LlamaConfig(**G.CFG, qk_norm=True))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in G.tiny_weights().items()}, strict=True)
    m.to(device=DEV, dtype=dtype)
    m.model.rotary_emb.float()
    m.device, m.dtype = torch.device(DEV), dtype
    return m


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_qwen3_model_against_the_recorded_transformers_logits(dtype, graph):
    """Prefill of two right-padded shared prompts (9 and 5 tokens), then decode steps fed the forced tokens: every step's logits
    against transformers' fp32 logits of the same weights, within the bounds tests/test_model_gpu.py takes from the reference's
    own comparison with HF (max abs < 0.75, mean relative difference < 0.05; bf16: 0.15)."""
    z = G.load_fixture()
    model = tiny_model(dtype)
    model.graph(graph)
    prompts, forced = torch.from_numpy(z["prompts"]).to(DEV), torch.from_numpy(z["forced"]).to(DEV)
    lens = [int(n) for n in z["prompt_lens"]]
    B = forced.shape[0]
    model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=16, max_shared_batch_sizes=[2], max_shared_seq_lengths=[9])
    assert model.model.layers[0].self_attn.kv_cache.per_completion_k_cache.shape[-1] == 64  # head_dim, not hidden // heads = 16
    out, logits = model.generate(input_ids=[prompts], seq_lens=[torch.tensor(lens, device=DEV)], num_return_sequences=G.NRET,
                                 max_new_tokens=G.NEW, temperature=0.0, return_logits=True, token_overrides=forced)
    got = torch.stack(list(logits), 1).float().cpu()  # [B, NEW, V]
    want = torch.stack([torch.from_numpy(z["logits"][j, lens[j // G.NRET] - 1: lens[j // G.NRET] - 1 + G.NEW]) for j in range(B)])
    assert out.shape == forced.shape and got.shape == want.shape  # (out holds the model's own choices; the forced tokens were fed)
    err, rel = float((got - want).abs().max()), float(rdiff(got, want).mean())
    print(f"{dtype} graph={graph}: max |logits - transformers fp32| = {err:.4f}, mean relative difference = {rel:.4f}")
    assert err < 0.75
    assert rel < (0.05 if dtype == torch.float16 else 0.15)


def norm_model(dtype, seed=0):
    """hidden 256 on 4 / 2 heads of 128: head_dim is not hidden // heads; random gains (from_config leaves them at 1)."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-6, head_dim=128, qk_norm=True)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=DEV, seed=seed, std=0.05)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for layer in m.model.layers:
            for nm in (layer.self_attn.q_norm, layer.self_attn.k_norm):
                nm.weight.copy_((1 + 0.3 * torch.randn(128, generator=g)).to(DEV, dtype))
    return m


def _fused_and_unfused_logits(model, graph, **cache_kw):
    g = torch.Generator(device=DEV).manual_seed(7)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)  # noqa: E731
    prefix, mid, new, nret = rnd(1, 21), rnd(2, 6), 6, 3
    overrides = rnd(2 * nret, new)
    model.setup_caches(max_unique_batch_size=2 * nret, max_unique_seq_length=16, max_shared_batch_sizes=[1, 2], max_shared_seq_lengths=[21, 6],
                       **cache_kw)
    kw = dict(input_ids=[prefix, mid], num_return_sequences=nret, max_new_tokens=new, temperature=0.0, return_logits=True, token_overrides=overrides)
    runs = []
    for fused in (True, False):
        for layer in model.model.layers:
            layer.self_attn.use_fused_decode = fused
        model.graph(False)
        model.graph(graph)
        runs.append(torch.stack(list(model.generate(**kw)[1])).float())
    assert torch.isfinite(runs[0]).all() and torch.isfinite(runs[1]).all()
    return runs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_fused_preamble_against_the_unfused_path(dtype):
    a, b = _fused_and_unfused_logits(norm_model(dtype), graph=False)
    rel = float(rdiff(a, b).mean())
    print(f"{dtype}: fused vs unfused mean relative difference = {rel:.5f}")
    assert rel < (0.02 if dtype == torch.float16 else 0.08)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("what", ["fp8-caches", "fp8-weights"])
def test_norm_composes_with_fp8_caches_and_fp8_weights_under_the_graph(dtype, what):
    model = norm_model(dtype, seed=2)
    kw = {}
    if what == "fp8-caches":
        kw = dict(kv_cache_dtype=FP8_DTYPE)
    else:
        model.quantize_weights()
        assert model.model.layers[0].self_attn.qkv_proj is not None and model.model.layers[0].self_attn.q_norm is not None
    a, b = _fused_and_unfused_logits(model, graph=True, **kw)
    rel = float(rdiff(a, b).mean())
    print(f"{dtype} {what}: fused vs unfused mean relative difference = {rel:.5f}")
    assert rel < (0.02 if dtype == torch.float16 else 0.08)


def test_drafts_return_plain_greedy_decoding():
    """generate(draft_tokens=3, draft=<plain run's tokens>) on a qk_norm model: the multi-token preamble with the norm.  Compared on
    the positions the top-2 gap rule of tests/test_speculative_gpu.py admits."""
    from tests.test_speculative_gpu import compared

    model = norm_model(torch.float16, seed=4)
    new = 16
    prompts = torch.randint(1, 512, (2, 24), generator=torch.Generator().manual_seed(4)).to(DEV)
    model.setup_caches(max_unique_batch_size=6, max_unique_seq_length=new + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[24])
    plain, logits = model.generate([prompts], num_return_sequences=3, max_new_tokens=new, temperature=0, return_logits=True)
    top2 = torch.stack(list(logits), 1).float().topk(2, -1).values
    n = compared((top2[..., 0] - top2[..., 1]).cpu())
    out, stats = model.generate([prompts], num_return_sequences=3, max_new_tokens=new, temperature=0, draft_tokens=3, draft=plain,
                                return_draft_stats=True)
    plain, out = plain.cpu(), out.cpu()
    print(f"compared positions per row: {n.tolist()}, accepted {stats.accepted.tolist()} of {stats.proposed.tolist()}")
    assert out.shape == plain.shape == (6, new) and int(stats.proposed.sum()) > 0
    for b in range(6):
        assert torch.equal(out[b, : n[b]], plain[b, : n[b]]), (b, out[b].tolist(), plain[b].tolist())
