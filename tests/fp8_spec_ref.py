"""CPU helper of tests/test_fp8_causal_gpu.py: the float64 reference model of tests/test_speculative_gpu.py (`ref_logits64`) with the
one rounding an fp8 unique cache adds.  The K (after RoPE) and V of the positions >= `first_fp8` -- the generated tokens: the prompts
of those tests sit in a 16-bit shared level -- pass through quantize_kv / dequantize_kv at fp16 with scale 1, the bytes a unit-scale
e4m3fn cache holds; everything else is float64.  With roundtrip=False it is ref_logits64 (tests/test_fp8_causal.py holds them equal)."""
import numpy as np
import torch

from hydragen_amd.kv_quant import dequantize_kv, quantize_kv


def fp8_roundtrip(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the value an fp16 model reads back from a unit-scale e4m3fn cache, as float64."""
    return dequantize_kv(quantize_kv(x.to(torch.float16)), None, torch.float16).double()


@torch.no_grad()
def ref_logits64_fp8(model, ids, first_fp8: int, roundtrip: bool = True):
    """float64 causal transformer over full sequences ids [b, n] with the model's weights, on the CPU; the keys and values of
    positions >= first_fp8 are read through the fp8 round trip."""
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
        if roundtrip and first_fp8 < n:
            k = torch.cat([k[:, :first_fp8], fp8_roundtrip(k[:, first_fp8:])], 1)
            v = torch.cat([v[:, :first_fp8], fp8_roundtrip(v[:, first_fp8:])], 1)
        k, v = k.repeat_interleave(H // Hkv, 2), v.repeat_interleave(H // Hkv, 2)
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5
        s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("-inf"))
        h = h + torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(b, n, H * D) @ f(a.o_proj.weight).T
        x = norm(h, layer.post_attention_layernorm.weight)
        h = h + (torch.nn.functional.silu(x @ f(m.gate_proj.weight).T) * (x @ f(m.up_proj.weight).T)) @ f(m.down_proj.weight).T
    return norm(h, model.model.norm.weight) @ f(model.lm_head.weight).T


@torch.no_grad()
def greedy64_fp8(model, prompts, new: int, fan: int = 1):
    """Greedy decoding of `new` tokens with the model above: (tokens [b * fan, new], top-2 gap of every decision [b * fan, new]).
    (The rows of a prompt are identical under greedy decoding: fan only repeats them, as num_return_sequences does.)"""
    ids = prompts.cpu()
    first = ids.shape[1]
    toks, gaps = [], []
    for _ in range(new):
        top = ref_logits64_fp8(model, ids, first)[:, -1].topk(2, -1)
        toks.append(top.indices[:, 0])
        gaps.append(top.values[:, 0] - top.values[:, 1])
        ids = torch.cat([ids, toks[-1][:, None]], 1)
    return torch.stack(toks, 1).repeat_interleave(fan, 0), torch.stack(gaps, 1).repeat_interleave(fan, 0)
