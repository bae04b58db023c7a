"""-m "not gpu": Qwen3-style attention in the model shell -- LlamaConfig.head_dim / qk_norm, the loader (from_hf_model), the
tensor-parallel rewrite -- and the host side of the two entry points that carry the per-head q/k RMSNorm into the RoPE + append
kernels (hyd_rope_append_decode_qkn, hyd_rope_append_multi_qkn).  tests/test_qk_norm_gpu.py holds the kernels and the model on
the device to tests/qk_norm_ref.py and tests/golden/qwen3_tiny.npz."""
import ctypes as C
import re
import subprocess
from copy import deepcopy
from pathlib import Path

import numpy as np
import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd.fused_decode import QkNorm
from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig
from tests import abi_table, qk_norm_ref as N, qwen3_golden as G
from tests import glue_ref as R

REPO = Path(__file__).resolve().parent.parent
TINY = dict(hidden_size=256, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=64,
            max_position_embeddings=64)


def _meta(cfg):
    with torch.device("meta"):
        return HydragenLlamaForCausalLM(cfg)


# ---- config ----------------------------------------------------------------------------------------------------------------
def test_defaults_leave_a_llama_model_as_it_was():
    """The new fields sit at the END of the dataclass (the loader builds it positionally) and change nothing at their defaults."""
    import dataclasses

    names = [f.name for f in dataclasses.fields(LlamaConfig)]
    assert names[-2:] == ["head_dim", "qk_norm"] and names[10] == "pad_token_id"
    cfg = LlamaConfig(**TINY)
    assert cfg.head_dim is None and cfg.qk_norm is False and cfg.get_head_dim() == 64
    sd = _meta(cfg).state_dict()
    assert not [k for k in sd if "q_norm" in k or "k_norm" in k]
    assert sd["model.layers.0.self_attn.q_proj.weight"].shape == (256, 256) and sd["model.layers.1.self_attn.k_proj.weight"].shape == (128, 256)
    assert len(sd) == 3 + 2 * 9
    with pytest.raises(ValueError, match="divisible"):  # the divisibility check of a config without head_dim stays
        _meta(LlamaConfig(**{**TINY, "hidden_size": 250}))


def test_explicit_head_dim_and_qk_norm():
    m = _meta(LlamaConfig(**TINY, head_dim=128, qk_norm=True))
    sd = m.state_dict()
    a = m.model.layers[0].self_attn
    assert a.head_dim == 128 and sd["model.layers.0.self_attn.q_proj.weight"].shape == (512, 256)
    assert sd["model.layers.0.self_attn.k_proj.weight"].shape == (256, 256) and sd["model.layers.0.self_attn.o_proj.weight"].shape == (256, 512)
    assert sd["model.layers.1.self_attn.q_norm.weight"].shape == (128,) and sd["model.layers.1.self_attn.k_norm.weight"].shape == (128,)
    assert a.q_norm.variance_epsilon == m.config.rms_norm_eps
    assert m.model.rotary_emb.cos_cached.shape[-1] == 128
    with pytest.raises(NotImplementedError, match="96"):
        _meta(LlamaConfig(**TINY, head_dim=96, qk_norm=True))
    _meta(LlamaConfig(**TINY, head_dim=96))  # without the norm a narrow head dim stays a model
    q8 = LlamaConfig.qwen3_8b()
    assert q8.get_head_dim() == 128 and q8.qk_norm and q8.num_key_value_heads == 8


def test_cpu_model_applies_the_norm_modules_before_the_rotation():
    """The unfused path: q_norm / k_norm are applied per head between the projection and RoPE (checked on the attention
    module's own pieces in float64, no device)."""
    from hydragen_amd.llama import apply_rotary_pos_emb

    torch.manual_seed(0)
    m = HydragenLlamaForCausalLM(LlamaConfig(**TINY, head_dim=64, qk_norm=True)).double()
    a = m.model.layers[0].self_attn
    with torch.no_grad():
        a.q_norm.weight.copy_(1 + 0.3 * torch.randn(64))
        a.k_norm.weight.copy_(1 - 0.3 * torch.randn(64))
    x = torch.randn(2, 3, 4, 64, dtype=torch.float64)
    want = N.qk_norm_ref64(x.numpy(), a.q_norm.weight.detach().numpy(), m.config.rms_norm_eps)
    assert np.allclose(a.q_norm(x).detach().numpy(), want, rtol=1e-12, atol=1e-12)
    assert not torch.equal(a.q_norm.weight, a.k_norm.weight)


# ---- loading ----------------------------------------------------------------------------------------------------------------
def test_from_hf_model_loads_an_in_memory_qwen3():
    tf = pytest.importorskip("transformers")
    cfg = tf.Qwen3Config(**G.CFG, tie_word_embeddings=False)
    hf = tf.Qwen3ForCausalLM(cfg).to(torch.bfloat16)
    with torch.no_grad():
        for name, p in hf.named_parameters():
            if "q_norm" in name or "k_norm" in name:
                p.copy_(1 + 0.3 * torch.randn_like(p.float()))
    m = HydragenLlamaForCausalLM.from_hf_model(hf)
    c = m.config
    assert (c.head_dim, c.qk_norm, c.hidden_size, c.num_attention_heads, c.num_key_value_heads) == (64, True, 64, 4, 2)
    assert c.rms_norm_eps == cfg.rms_norm_eps and c.get_head_dim() == 64 != c.hidden_size // c.num_attention_heads
    want = {k: v for k, v in hf.state_dict().items() if "inv_freq" not in k}
    got = m.state_dict()
    assert sorted(got) == sorted(want)  # no key missing, none unexpected
    for k in want:
        assert got[k].dtype == torch.bfloat16 and torch.equal(got[k], want[k]), k
    assert m.model.rotary_emb.cos_cached.dtype == torch.float32 and m.dtype == torch.bfloat16
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        HydragenLlamaForCausalLM.from_hf_model(tf.Qwen3ForCausalLM(cfg))


def test_from_hf_model_still_loads_a_llama():
    tf = pytest.importorskip("transformers")
    kw = {k: v for k, v in G.CFG.items() if k != "head_dim"}
    hf = tf.LlamaForCausalLM(tf.LlamaConfig(**kw, tie_word_embeddings=False)).to(torch.float16)
    m = HydragenLlamaForCausalLM.from_hf_model(hf)
    assert m.config.qk_norm is False and m.config.get_head_dim() == 16 and m.model.layers[0].self_attn.q_norm is None
    want = {k: v for k, v in hf.state_dict().items() if "inv_freq" not in k}
    assert sorted(m.state_dict()) == sorted(want) and all(torch.equal(m.state_dict()[k], v) for k, v in want.items())


# ---- the golden ----------------------------------------------------------------------------------------------------------------
def test_golden_is_what_the_recorder_describes():
    z = G.load_fixture()
    prompts, forced = G.tokens(int(z["seed"]))
    assert int(z["seed"]) == G.SEED and np.array_equal(z["prompts"], prompts) and np.array_equal(z["forced"], forced)
    assert tuple(z["prompt_lens"]) == G.PROMPT_LENS == (9, 5)
    seqs = G.full_sequences(prompts, forced)
    assert z["logits"].shape == (4, 13, 64) and z["logits"].dtype == np.float32 and [len(s) for s in seqs] == [13, 13, 9, 9]
    assert np.isfinite(z["logits"]).all() and not z["logits"][2:, 9:].any() and np.abs(z["logits"][:, :9]).min() > 0
    w = G.tiny_weights()
    for k, v in w.items():  # every weight is exact in both 16-bit dtypes
        t = torch.from_numpy(v)
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t), k
    qn, kn = w["model.layers.0.self_attn.q_norm.weight"], w["model.layers.0.self_attn.k_norm.weight"]
    assert not np.array_equal(qn, kn) and 0.15 < qn.std() < 0.45 and abs(qn.mean() - 1) < 0.2
    assert G.FIXTURE.stat().st_size < 64 * 1024


def test_golden_logits_are_what_transformers_computes():
    pytest.importorskip("transformers")
    z = G.load_fixture()
    assert np.allclose(G.hf_logits(int(z["seed"])), z["logits"], rtol=0, atol=1e-4)


def test_tiny_weights_load_into_the_model_shell():
    m = HydragenLlamaForCausalLM(LlamaConfig(**G.CFG, qk_norm=True))
    report = m.load_state_dict({k: torch.from_numpy(v) for k, v in G.tiny_weights().items()}, strict=True)
    assert not report.missing_keys and not report.unexpected_keys


# ---- tensor parallelism ------------------------------------------------------------------------------------------------------
def test_apply_tp_shards_heads_and_keeps_the_gains_whole():
    from hydragen_amd.tp import apply_tp

    m = _meta(LlamaConfig(**TINY, head_dim=128, qk_norm=True))
    apply_tp(m.model, rank=1, world_size=2)
    a, c = m.model.layers[1].self_attn, m.config
    assert (c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.get_head_dim()) == (2, 1, 128, 128)
    assert (a.num_heads, a.num_key_value_heads, a.head_dim) == (2, 1, 128)
    assert a.q_proj.weight.shape == (256, 256) and a.k_proj.weight.shape == (128, 256) and a.o_proj.weight.shape == (256, 256)
    assert a.q_norm.weight.shape == (128,) and a.k_norm.weight.shape == (128,)
    plain = _meta(LlamaConfig(**TINY))  # and a config without head_dim keeps deriving it
    apply_tp(plain.model, rank=0, world_size=2)
    assert plain.config.head_dim is None and plain.config.get_head_dim() == 64 == plain.model.layers[0].self_attn.head_dim


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_block_and_its_layout():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    new = {"hyd_rope_append_decode_qkn", "hyd_rope_append_multi_qkn"}
    assert new <= declared and new <= set(_lib.EXPORTS) and all(hasattr(lib, n) for n in new)
    assert lib.hyd_version() == 500
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(hyd_qk_norm), '
           "offsetof(hyd_qk_norm, q_weight), offsetof(hyd_qk_norm, k_weight), offsetof(hyd_qk_norm, eps), offsetof(hyd_qk_norm, flags));return 0;}\n")
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got == [C.sizeof(QkNorm), QkNorm.q_weight.offset, QkNorm.k_weight.offset, QkNorm.eps.offset, QkNorm.flags.offset] == [24, 0, 8, 16, 20]


def _qn(**kw):
    qn = QkNorm(abi_table.PTR, abi_table.PTR, 1e-6, 0)
    for k, v in kw.items():
        setattr(qn, k, v)
    return qn


def _call(entry, p, kq, qn):
    lib = _lib.load()
    qn = None if qn is None else C.byref(qn)
    if entry == "decode":
        rc = lib.hyd_rope_append_decode_qkn(C.byref(p), None if kq is None else C.byref(kq), qn, None)
    else:
        rc = lib.hyd_rope_append_multi_qkn(C.byref(p), qn, None)
    return rc, lib.hyd_last_error_string().decode()


needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="refusals are replayed on machines without a device only")
BAD_NORMS = [(dict(q_weight=None), -1, "q_weight is null"), (dict(k_weight=None), -1, "k_weight is null"),
             (dict(q_weight=abi_table.MIS8), -1, "q_weight must be 16-byte aligned"), (dict(k_weight=abi_table.ODD), -1, "k_weight must be 16-byte aligned"),
             (dict(eps=0.0), -1, "eps"), (dict(eps=-1e-6), -1, "eps"), (dict(eps=float("nan")), -1, "eps"), (dict(eps=float("inf")), -1, "eps"),
             (dict(flags=1), -1, "flags"), (dict(flags=-1), -1, "flags")]


@needs_no_device
@pytest.mark.parametrize("kw, code, frag", BAD_NORMS)
def test_bad_norm_blocks_are_refused(kw, code, frag):
    for entry, p, kq in (("decode", abi_table.rope(), None), ("decode", abi_table.rope(), abi_table.kvq()), ("multi", abi_table.rope_multi(), None)):
        rc, msg = _call(entry, p, kq, _qn(**kw))
        assert rc == code and frag in msg, (entry, rc, msg)


@needs_no_device
def test_norm_with_a_narrow_head_dim_is_unsupported():
    rc, msg = _call("decode", abi_table.rope(head_dim=96), None, _qn())
    assert rc == -2 and "head_dim 96" in msg
    assert _call("decode", abi_table.rope(head_dim=96), None, None)[0] == abi_table.HYD_ERR_LAUNCH  # the narrow call itself is taken
    assert _call("decode", abi_table.rope(head_dim=128), None, _qn())[0] == abi_table.HYD_ERR_LAUNCH  # head_dim == D is the native row
    rc, msg = _call("multi", abi_table.rope_multi(D=96), None, _qn())
    assert rc == -2 and "head_dim 96" in msg  # the existing head-dim refusal answers first


@needs_no_device
def test_a_valid_norm_call_passes_every_check():
    """Without a device a call that passes validation ends at the launch: HYD_ERR_LAUNCH, never a refusal."""
    for entry, p, kq in (("decode", abi_table.rope(), None), ("decode", abi_table.rope(), abi_table.kvq()), ("multi", abi_table.rope_multi(), None),
                         ("decode", abi_table.rope(D=64, dtype=0), None), ("multi", abi_table.rope_multi(D=256, T=8), None)):
        for qn in (None, _qn(), _qn(eps=1e-5)):
            rc, msg = _call(entry, p, kq, qn)
            assert rc == abi_table.HYD_ERR_LAUNCH, (entry, rc, msg)


@needs_no_device
def test_the_null_norm_call_answers_what_the_existing_entry_points_answer():
    """Every recorded refusal of hyd_rope_append_decode, _kvq and hyd_rope_append_multi (tests/golden/abi_table.json), replayed
    through the _qkn entry points with qn == NULL: the same code and the same string -- and, with a valid norm block beside it,
    still the same answer: the norm's own checks come last."""
    table = abi_table.load_fixture()
    lib = _lib.load()
    seen = 0
    for cid, entry, kw in abi_table.REFUSAL_CASES:
        if entry not in ("hyd_rope_append_decode", "hyd_rope_append_decode_kvq", "hyd_rope_append_multi"):
            continue
        kw = dict(kw)
        null, kq = kw.pop("null", False), kw.pop("kq", None)
        multi = entry == "hyd_rope_append_multi"
        p = None if null else C.byref((abi_table.rope_multi if multi else abi_table.rope)(**kw))
        kq = None if kq is None else C.byref(abi_table.kvq(**kq))
        for qn in (None, _qn()):
            qp = None if qn is None else C.byref(qn)
            rc = lib.hyd_rope_append_multi_qkn(p, qp, None) if multi else lib.hyd_rope_append_decode_qkn(p, kq, qp, None)
            assert {"rc": rc, "error": lib.hyd_last_error_string().decode()} == table[cid], cid
        seen += 1
    assert seen > 60


def test_python_faces_take_both_gains_or_neither():
    from hydragen_amd.fused_decode import qk_norm_params

    q = torch.zeros(1, 1, 2, 64, dtype=torch.float16)
    w = torch.ones(64, dtype=torch.float16)
    assert qk_norm_params(q, 64, None, None, None) is None
    for args in ((w, None, 1e-6), (None, w, 1e-6), (w, w, None), (None, None, 1e-6)):
        with pytest.raises(ValueError):
            qk_norm_params(q, 64, *args)


# ---- the definition and its bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp32_emulation_of_the_kernel_is_inside_the_bound(dtype, D):
    """The bound is derived, not measured; an fp32 evaluation in the kernel's order of operations (numpy, host) has to fit, in both
    summation orders tried, and one that sums the squares over TWO heads has to miss it by orders of magnitude."""
    B, Hq, Hkv = 3, 5, 1
    q, _, _, qw, _ = N.make_inputs(dtype, B, Hq, Hkv, D)
    cos, sin = N.rotary_tables(D, 32)
    pos = np.array([3, 17, 31])
    c, s = cos.numpy()[pos], sin.numpy()[pos]
    x64, w64 = N.f64(q), N.f64(qw)
    want, n = N.qk_norm_rope_ref64(x64, w64, 1e-6, c, s)
    bound = N.qk_norm_rope_bound(want, n, dtype)
    x, w = x64.astype(np.float32), w64.astype(np.float32)

    def emulate(ss):
        r = (np.float32(1) / np.sqrt((ss * np.float32(1.0 / D) + np.float32(1e-6)).astype(np.float32))).astype(np.float32)
        nn = (x * r).astype(np.float32) * w
        return R.rope_emulate_fp32(nn, c, s, dtype).double().numpy()

    sq = (x * x).astype(np.float32)
    orders = [sq.sum(-1, keepdims=True, dtype=np.float32), sq.reshape(B, Hq, D // 16, 16).sum(-1, dtype=np.float32).sum(-1, keepdims=True, dtype=np.float32)]
    for ss in orders:
        got = emulate(ss)
        assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()
    assert not want[0, Hq - 1].any() and not emulate(orders[0])[0, Hq - 1].any()  # the all-zero head: exact zeros
    two_heads = orders[0] + np.roll(orders[0], 1, axis=1)
    excess = np.abs(emulate(two_heads) - want) / bound
    assert excess.max() > 100
    assert 2.0 ** -18 < N.qk_norm_c(D) < 2.0 ** -14
