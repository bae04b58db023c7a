"""
Model shell around the hot path: the counterpart of /root/reference/hydragen/llama.py with the same
class / method names and semantics (`HydragenLlamaForCausalLM.setup_caches / graph / append_shared /
process_unique / generate / empty_shared_cache / truncate_shared_caches`), written from scratch so it
does not depend on a particular `transformers` version (the reference pins 4.37.2, llama.py:1-10).

What is native here: every attention call goes to the HIP kernels (hydragen_amd.attention / flash), and
the per-token RoPE + unique-KV append + seq_lens computation of the decode step is ONE HIP kernel
(`hyd_rope_append_decode`, replacing llama.py:236-262,317-330,485-501,565-569).  The dense layers
(q/k/v/o projections, SwiGLU MLP, lm_head) are plain torch matmuls (hipBLASLt) -- plumbing, as in the
reference.  Weights are random-initialised from a config (`from_config`); loading Hugging Face
checkpoints is out of scope here (no network), but `load_state_dict` of a HF Llama state dict works
because parameter names match (llama.py:1398-1422).

Decode runs under a HIP graph exactly like the reference's CUDA-graph wrapper (llama.py:781-866).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Union

import torch
from torch import Tensor, nn

from . import generation, layer_ops, placement, sampling, scoring, speculative
from .attention import hydragen_attention
from . import flash as _flash
from .flash import flash_attention, flash_attention_seqlen, padded_head_dim
from . import kv_quant as _kv_quant
from .kv_quant import FP8_DTYPE, dequantize_kv, quantize_kv, scale_constant
from .tp import all_reduce_sum
from .weight_quant import Fp8Linear, W8Scratch


@dataclass
class LlamaConfig:
    """The subset of transformers.LlamaConfig the reference reads (llama.py:423-462,635-653)."""

    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 32
    vocab_size: int = 32000
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0
    max_position_embeddings: int = 4096
    attention_bias: bool = False
    pad_token_id: Optional[int] = None
    # Qwen3-style attention (new fields stay at the END: from_hf_model and callers build the config positionally)
    head_dim: Optional[int] = None  # None: hidden_size // num_attention_heads
    qk_norm: bool = False           # RMSNorm over every query head and every key head between the projection and RoPE

    def get_head_dim(self) -> int:
        """The one place that knows a head's width: `head_dim` when the checkpoint states it, else hidden_size // heads."""
        return self.hidden_size // self.num_attention_heads if self.head_dim is None else self.head_dim

    @staticmethod
    def llama2_7b(**kw):
        return LlamaConfig(**kw)

    @staticmethod
    def qwen3_8b(**kw):
        return LlamaConfig(hidden_size=4096, intermediate_size=12288, num_hidden_layers=36, num_attention_heads=32,
                           num_key_value_heads=8, vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1000000.0,
                           max_position_embeddings=40960, head_dim=128, qk_norm=True, **kw)

    @staticmethod
    def llama3_70b(**kw):
        return LlamaConfig(hidden_size=8192, intermediate_size=28672, num_hidden_layers=80, num_attention_heads=64,
                           num_key_value_heads=8, vocab_size=128256, rope_theta=500000.0,
                           max_position_embeddings=8192, **kw)


def repeat_to_batch_size(tensors: list[Tensor], target_batch_size: int | None = None):
    """llama.py:32-46."""
    if target_batch_size is None:
        target_batch_size = max(t.shape[0] for t in tensors)
    out = []
    for t in tensors:
        assert target_batch_size % t.shape[0] == 0
        out.append(t.repeat_interleave(target_batch_size // t.shape[0], dim=0))
    return out


class RMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, x):
        # one fused kernel (fp32 statistics inside) instead of the seven elementwise / reduce launches of the spelled-out
        # form (float, pow, mean, add + rsqrt, mul, cast, mul): 2 norms x 32 layers of them were 13 % of a decode step.
        # Deviation from transformers' LlamaRMSNorm (stated): that one rounds x * rsqrt(var + eps) to the
        # 16-bit dtype BEFORE the multiply by `weight`; this form (and hyd_add_rmsnorm, csrc/layer_ops.hip) multiplies in
        # fp32 and rounds once -- at most one 16-bit ulp per element apart, the closer of the two to the fp32 formula
        # (tests/test_layer_ops_gpu.py bounds both against it).
        return nn.functional.rms_norm(x, (x.shape[-1],), self.weight, self.variance_epsilon)


def _fused_weight(cache: Optional[Tensor], linears) -> Optional[Tensor]:
    """One [sum of out_features, in_features] weight behind several column-parallel nn.Linear modules that read the same
    input (q|k|v, gate|up): the decode step then runs one GEMM instead of two or three (MI355X, batch 1024, Llama-2-7B:
    129 -> 86 us for q, k, v and 167 -> 154 us for gate, up per layer; tests/probes/gemm_fusion_probe.py).  The modules'
    own `weight` parameters become VIEWS of the fused tensor, so state dicts, in-place loading, `make_tp_files` and the
    reference's attribute names keep working and no memory is added; anything that replaces ANY of the weights (`apply_tp`,
    `.to()`, a quantised or merged single projection) is noticed by its address and everything is fused again.  The shared
    storage means that a per-tensor ownership check (safetensors `save_file`) sees aliases: save `state_dict()` clones or
    call `unfuse_weights(model)` first.  None when it does not apply (biases, meta / CPU weights, graph capture)."""
    w0 = linears[0].weight
    if cache is not None and w0.shape[1] == cache.shape[1]:
        # every module's weight must still BE its slice of the fused tensor: any of them may have been replaced on its own
        # (quantisation, a LoRA merge, load_state_dict(assign=True) on part of the modules)
        off, row = cache.data_ptr(), cache.shape[1] * cache.element_size()
        for l in linears:
            if l.weight.data_ptr() != off or l.weight.dtype != cache.dtype or not l.weight.is_contiguous():
                break
            off += l.weight.shape[0] * row
        else:
            if off == cache.data_ptr() + cache.shape[0] * row:
                return cache
    if any(l.bias is not None for l in linears) or not w0.is_cuda or torch.cuda.is_current_stream_capturing():
        return None
    with torch.no_grad():
        w = torch.cat([l.weight for l in linears], 0)
        o = 0
        for l in linears:
            n = l.weight.shape[0]
            l.weight.data = w[o:o + n]
            o += n
    return w


def unfuse_weights(module: nn.Module) -> None:
    """Give every projection its own storage again (undoes `_fused_weight` until the next forward fuses anew)."""
    for m in module.modules():
        for attr, names in (("_gate_up", ("gate_proj", "up_proj")), ("_qkv", ("q_proj", "k_proj", "v_proj"))):
            if getattr(m, attr, None) is not None:
                for n in names:
                    lin = getattr(m, n)
                    lin.weight.data = lin.weight.data.clone()
                setattr(m, attr, None)


class LlamaMLP(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.gate_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.up_proj = nn.Linear(config.hidden_size, config.intermediate_size, bias=False)
        self.down_proj = nn.Linear(config.intermediate_size, config.hidden_size, bias=False)
        self.tp_reduce = False  # row-parallel down_proj needs the all-reduce of tp.py:83-87
        self._gate_up: Optional[Tensor] = None
        self.gate_up_proj = None  # weight_quant.Fp8Linear once the model is quantized (gate_proj / up_proj are then None)

    def forward(self, x):
        if self.gate_up_proj is not None:  # fp8 weights (quantize_weights): gate|up is one module, _fused_weight has nothing to fuse
            g, u = self.gate_up_proj(x).split(self.gate_up_proj.out_features // 2, dim=-1)
            y = self.down_proj(layer_ops.swiglu(g, u) if layer_ops.supported(g) else nn.functional.silu(g) * u)
            return all_reduce_sum(y) if self.tp_reduce else y
        self._gate_up = w = _fused_weight(self._gate_up, (self.gate_proj, self.up_proj))
        if w is not None:
            g, u = nn.functional.linear(x, w).split(self.gate_proj.weight.shape[0], dim=-1)
        else:
            g, u = self.gate_proj(x), self.up_proj(x)
        # silu(gate) * up: one HIP kernel over the two column halves of the fused GEMM output (the strided silu and the
        # strided multiply were 15 + 19 us per layer at batch 1024); the torch form on CPU / fp32 / odd widths
        y = self.down_proj(layer_ops.swiglu(g, u) if layer_ops.supported(g) else nn.functional.silu(g) * u)
        return all_reduce_sum(y) if self.tp_reduce else y


class RotaryTable(nn.Module):
    """cos/sin cache [max_pos, head_dim] in the rotate-half convention the reference uses through HF's
    apply_rotary_pos_emb (llama.py:49-55,494-501)."""

    def __init__(self, dim, max_position_embeddings, base, device=None):
        super().__init__()
        inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32, device=device) / dim))
        t = torch.arange(max_position_embeddings, dtype=torch.float32, device=device)
        freqs = torch.outer(t, inv_freq)
        emb = torch.cat((freqs, freqs), dim=-1)
        self.register_buffer("cos_cached", emb.cos(), persistent=False)
        self.register_buffer("sin_cached", emb.sin(), persistent=False)


def rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2 :]
    return torch.cat((-x2, x1), dim=-1)


def apply_rotary_pos_emb(q, k, cos, sin, position_ids):
    """q,k [b, s, h, d]; cos/sin [max_pos, d]; position_ids [b, s] absolute (llama.py:485-501)."""
    cos = cos[position_ids].unsqueeze(2).to(q.dtype)
    sin = sin[position_ids].unsqueeze(2).to(q.dtype)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def narrow_kv_head_dim(head_dim: int, n_kv_heads: int, n_q_heads: Optional[int] = None) -> int:
    """The head dim the attention kernels run a model's q and shared caches at when its UNIQUE cache can keep rows of the true
    width (narrow unique caches, flash.narrow_kv_native: head_dim % 16 == 0 and not 64 / 128 / 256, as many kv as query heads, whole
    lane groups of the token-row suffix kernel), else 0: the model then keeps every tensor at head_dim, as always."""
    if head_dim in (64, 128, 256) or head_dim % 16 or not 16 <= head_dim < 256 or n_q_heads not in (None, n_kv_heads):
        return 0
    D = padded_head_dim(head_dim)
    return D if n_kv_heads % (64 // (D // 8)) == 0 else 0


class SharedCache(nn.Module):
    """llama.py:58-170: one shared level, sequences packed back to back in [maxB*maxP, Hkv, D].  D may be wider than the model's
    head dim (narrow_kv_head_dim): `fill` writes the leading columns, the others keep the zeros they were allocated with."""

    def __init__(self, max_batch_size, max_seq_length, num_heads, head_dim, dtype, device):
        super().__init__()
        self.register_buffer("k_cache", torch.zeros((max_batch_size * max_seq_length, num_heads, head_dim), dtype=dtype, device=device), persistent=False)
        self.register_buffer("v_cache", torch.zeros_like(self.k_cache), persistent=False)
        self.register_buffer("seq_lens", torch.zeros((max_batch_size,), dtype=torch.int32, device=device), persistent=False)
        self.register_buffer("cumsum_lengths", torch.zeros((max_batch_size + 1,), dtype=torch.int32, device=device), persistent=False)
        self.max_batch_size = max_batch_size
        self.max_sequence_length = max_seq_length
        self.current_batch_size = 0
        self.use_varlen = False
        self.sliced_sequence_length = None

    def get_current_batch_size(self):
        return self.current_batch_size

    def fill(self, key_states: Tensor, value_states: Tensor, seq_lens: Tensor):
        bs = key_states.shape[0]
        if bs > self.max_batch_size:
            raise ValueError(f"Batch size {bs} exceeds max batch size {self.max_batch_size}")
        if key_states.shape[1] > self.max_sequence_length:
            raise ValueError(f"Sequence length {key_states.shape[1]} exceeds max sequence length {self.max_sequence_length}")
        lens = [int(x) for x in seq_lens.tolist()]  # host sync, as llama.py:159-167
        ks = torch.cat([key_states[i, : lens[i]] for i in range(bs)], dim=0)
        vs = torch.cat([value_states[i, : lens[i]] for i in range(bs)], dim=0)
        self.k_cache[: ks.shape[0], :, : ks.shape[-1]] = ks
        self.v_cache[: vs.shape[0], :, : vs.shape[-1]] = vs
        self.seq_lens[:bs] = seq_lens.to(torch.int32)
        self.cumsum_lengths[0] = 0
        self.cumsum_lengths[1 : bs + 1] = seq_lens.cumsum(0).to(torch.int32)
        self.use_varlen = max(lens) != min(lens)
        self.sliced_sequence_length = None if self.use_varlen else lens[0]
        self.current_batch_size = bs

    def get_used_cumsum_lengths(self):
        return self.cumsum_lengths[: self.current_batch_size + 1]


class PerLayerKVCache(nn.Module):
    """llama.py:173-346."""

    def __init__(self, max_unique_batch_size, max_unique_seq_length, max_shared_batch_sizes, max_shared_seq_lengths,
                 n_kv_heads, head_dim, device, dtype, arena: Optional[Tensor] = None, kv_cache_dtype: Optional[torch.dtype] = None,
                 n_q_heads: Optional[int] = None, kv_scales: str = "unit", kv_scale_margin: float = 2.0):
        super().__init__()
        shape = (max_unique_batch_size, max_unique_seq_length, n_kv_heads, head_dim)
        self.head_dim = head_dim
        # kv_cache_dtype = torch.float8_e4m3fn: the unique arena holds e4m3fn bytes (kv_quant.py) with one fp32 scale per kv head
        # for K and for V (k_scale / v_scale: 1.0 with kv_scales = "unit"; "calibrate" rewrites them in place from the prompts'
        # K / V -- kv_amax, the freeze rule below -- so a captured graph keeps their pointers); the shared caches stay in `dtype`
        udtype = dtype if kv_cache_dtype is None else kv_cache_dtype
        if udtype not in (dtype, FP8_DTYPE):
            raise NotImplementedError(f"unique KV cache dtype {udtype}: the model's {dtype} or {FP8_DTYPE}")
        self.fp8 = udtype == FP8_DTYPE
        # Narrow unique caches (head dims 80 / 96 / 192 ... on multi-head models): the unique arena keeps rows of head_dim elements --
        # the suffix pass reads exactly those bytes --, the shared caches and q run at the kernels' head dim with zero pad columns
        self.kernel_head_dim = (0 if self.fp8 else narrow_kv_head_dim(head_dim, n_kv_heads, n_q_heads)) or head_dim
        self.narrow = self.kernel_head_dim != head_dim
        if self.fp8:
            self.register_buffer("k_scale", torch.ones((n_kv_heads,), dtype=torch.float32, device=device), persistent=False)
            self.register_buffer("v_scale", torch.ones((n_kv_heads,), dtype=torch.float32, device=device), persistent=False)
        else:
            self.k_scale = self.v_scale = None
        if kv_scales not in ("unit", "calibrate"):
            raise ValueError(f'kv_scales {kv_scales!r}: "unit" or "calibrate"')
        if kv_scales != "unit" and not self.fp8:
            raise ValueError(f"kv_scales={kv_scales!r} belongs to fp8 unique caches, this cache is {udtype}")
        # "calibrate": the running max |K|, max |V| per kv head of the prefills' 16-bit K / V (kv_quant.observe_absmax), allocated
        # once; None with "unit": nothing is observed and nothing new is launched.  The scales are rewritten from it only inside a
        # window that generate() / score() open and the first write to the unique cache closes: while no row of it is alive
        self.kv_scale_margin = float(kv_scale_margin)
        scale_constant(self.kv_scale_margin)  # (refuses a margin that is not finite and positive)
        self._scale_window = False
        if kv_scales == "calibrate":
            self.register_buffer("kv_amax", torch.zeros((2, n_kv_heads), dtype=torch.float32, device=device), persistent=False)
        else:
            self.kv_amax = None
        dtype_unique = udtype
        # One allocation per layer (the reference's two attribute names, llama.py:186-198, stay as views of it): a sequence's K rows,
        # then its V rows (placement.kv_arena: the suffix pass streams that 1.5-3 % faster than all K, then all V).  WHERE the arena
        # sits in HBM matters too (profiles/r05_gqa_placement.md): `setup_caches` hands in arenas chosen by hydragen_amd/placement.py;
        # without one, a plain allocation of the same layout.
        if arena is None:
            arena = placement.kv_arena(shape, dtype_unique, device, zero=True)
        assert tuple(arena.shape) == (2,) + shape and arena.dtype == dtype_unique, f"{tuple(arena.shape)} {arena.dtype}"
        self.register_buffer("per_completion_k_cache", arena[0])
        self.register_buffer("per_completion_v_cache", arena[1])
        self.shared_caches = nn.ModuleList([
            SharedCache(b, s, n_kv_heads, self.kernel_head_dim, dtype, device)
            for b, s in zip(max_shared_batch_sizes, max_shared_seq_lengths)
        ])
        self.num_used_shared_caches = 0

    def empty_shared_cache(self):
        self.truncate_shared_caches(0)

    def get_num_total_shared_caches(self):
        return len(self.shared_caches)

    def truncate_shared_caches(self, n: int):
        assert n <= self.get_num_total_shared_caches(), f"{n} {self.get_num_total_shared_caches()}"
        self.num_used_shared_caches = n
        if n == 0 and self.kv_amax is not None:
            self.kv_amax.zero_()  # a fresh hierarchy is calibrated from its own prompts (kept levels keep the running maximum)

    # ---- calibrated scales ("calibrate"): observe -> window -> freeze -----------------------------------------------------------
    def observe_kv(self, k: Tensor, v: Tensor, row_lens: Optional[Tensor] = None):
        """A prefill's 16-bit K (after RoPE) and V, as they come: one hyd_kv_absmax launch into kv_amax."""
        if self.kv_amax is not None:
            _kv_quant.observe_absmax(k, v, self.kv_amax, row_lens)

    def open_scale_window(self):
        """generate() / score() start: the unique cache holds no row that a later launch of the call reads, the scales may move."""
        self._scale_window = self.kv_amax is not None

    def close_scale_window(self, write: bool = True):
        """The first write to the unique cache of a call (or the call's end, write=False): the scales are written once from
        kv_amax and stay as they are until the next window -- every fp8 row is read with the scales it was written with."""
        if self._scale_window:
            self._scale_window = False
            if write:
                _kv_quant.scales_from_absmax(self.kv_amax, self.k_scale, self.v_scale, self.kv_scale_margin)

    def reset_kv_scales(self):
        """Forget the running maxima and set the scales back to 1.0 (in place: captured graphs keep the pointers)."""
        self._scale_window = False
        if self.kv_amax is not None:
            self.kv_amax.zero_()
        if self.fp8:
            self.k_scale.fill_(1.0)
            self.v_scale.fill_(1.0)

    def scales(self) -> dict:
        """The k_scale / v_scale keywords of the attention operators (empty for 16-bit caches)."""
        return dict(k_scale=self.k_scale, v_scale=self.v_scale) if self.fp8 else {}

    def _store(self, cache: Tensor, x: Tensor, scale: Optional[Tensor]):
        """(cache bytes, value bytes): fp8 caches receive quantize_kv(x, scale), moved as bytes."""
        if not self.fp8:
            return cache, x
        return cache.view(torch.uint8), quantize_kv(x, scale).view(torch.uint8)

    def update_per_completion_kvs(self, input_pos: Tensor, k_val: Tensor, v_val: Tensor):
        """input_pos [bs, sl]; k_val/v_val [bs, sl, h, d] -> scatter into the caches (llama.py:236-262)."""
        assert input_pos.shape[1] == k_val.shape[1], f"{input_pos.shape} {k_val.shape}"
        self.close_scale_window()
        bs, sl, h, d = k_val.shape
        idx = input_pos[:, :, None, None].expand(bs, -1, h, d).to(torch.int64)
        kc, kv = self._store(self.per_completion_k_cache, k_val, self.k_scale)
        vc, vv = self._store(self.per_completion_v_cache, v_val, self.v_scale)
        kc[:bs].scatter_(1, idx, kv)
        vc[:bs].scatter_(1, idx, vv)
        return self.per_completion_k_cache[:bs], self.per_completion_v_cache[:bs]

    @torch.no_grad()
    def copy_shared_to_unique(self, total_num_sequences: int):
        """llama.py:264-298 (the no-sharing baseline materialises the prefix per sequence)."""
        assert self.num_used_shared_caches == 1, "Cannot copy shared without exactly one active shared cache"
        self.close_scale_window()
        sc: SharedCache = self.shared_caches[0]
        sb = sc.get_current_batch_size()
        assert total_num_sequences % sb == 0
        rep = total_num_sequences // sb
        cu = sc.cumsum_lengths.tolist()
        d = self.head_dim  # (the shared caches may be wider: zero pad columns)
        kc, kv = self._store(self.per_completion_k_cache, sc.k_cache[..., :d], self.k_scale)
        vc, vv = self._store(self.per_completion_v_cache, sc.v_cache[..., :d], self.v_scale)
        for i in range(sb):
            n = cu[i + 1] - cu[i]
            kc[i * rep : (i + 1) * rep, :n] = kv[cu[i] : cu[i + 1]].unsqueeze(0)
            vc[i * rep : (i + 1) * rep, :n] = vv[cu[i] : cu[i + 1]].unsqueeze(0)

    @torch.no_grad()
    def repeat_per_completion_cache_for_num_samples(self, current_size: int, num_samples: int):
        if num_samples == 1:
            return
        for c in (self.per_completion_k_cache, self.per_completion_v_cache):
            c = c.view(torch.uint8) if self.fp8 else c  # a byte copy either way
            c[: current_size * num_samples] = c[:current_size].repeat_interleave(num_samples, 0)

    def get_used_shared_caches(self) -> list[SharedCache]:
        return list(self.shared_caches)[: self.num_used_shared_caches]

    def get_shared_len(self, final_batch_size: int):
        """llama.py:317-330: per-sequence total shared length [B] (long)."""
        if self.num_used_shared_caches == 0:
            return torch.zeros((final_batch_size,), dtype=torch.long, device=self.per_completion_k_cache.device)
        lens = [c.seq_lens[: c.current_batch_size] for c in self.get_used_shared_caches()]
        return sum(repeat_to_batch_size(lens, final_batch_size)).long()

    def has_shared(self):
        return self.num_used_shared_caches > 0

    def append_shared(self, key_states, value_states, seq_lens):
        if self.num_used_shared_caches >= self.get_num_total_shared_caches():
            raise ValueError(f"No more available shared caches: {self.num_used_shared_caches} {self.get_num_total_shared_caches()}")
        self.shared_caches[self.num_used_shared_caches].fill(key_states, value_states, seq_lens)
        self.num_used_shared_caches += 1

    @torch.no_grad()
    def promote_unique(self, rows: Tensor, lens: Tensor, host_lens, use_kernel: bool = True):
        """Fork (hydragen_amd/fork.py): the first lens[i] cached tokens of unique sequence rows[i] become sequence i of the next
        free shared level -- K and V gathered by one hyd_kv_promote launch (use_kernel=False: its torch definition), no forward
        pass; fp8 unique caches are widened with this cache's scales.  rows / lens: [k] device vectors; host_lens: the same
        lengths on the host (the caller has them: nothing is synchronised here).  The level is left exactly as SharedCache.fill
        leaves it for the same data, and the same errors are raised: no free level, batch or length over the level's maximum."""
        from .fork import promote_kv, promote_kv_reference

        if self.num_used_shared_caches >= self.get_num_total_shared_caches():
            raise ValueError(f"No more available shared caches: {self.num_used_shared_caches} {self.get_num_total_shared_caches()}")
        sc: SharedCache = self.shared_caches[self.num_used_shared_caches]
        host_lens = [int(x) for x in host_lens]
        bs = len(host_lens)
        if bs > sc.max_batch_size:
            raise ValueError(f"Batch size {bs} exceeds max batch size {sc.max_batch_size}")
        if max(host_lens) > sc.max_sequence_length:
            raise ValueError(f"Sequence length {max(host_lens)} exceeds max sequence length {sc.max_sequence_length}")
        cu = (promote_kv if use_kernel else promote_kv_reference)(
            self.per_completion_k_cache, self.per_completion_v_cache, rows, lens, sc.k_cache, sc.v_cache,
            max_len=max(host_lens), **self.scales())
        sc.seq_lens[:bs] = lens.to(torch.int32)
        sc.cumsum_lengths[: bs + 1] = cu
        sc.use_varlen = max(host_lens) != min(host_lens)
        sc.sliced_sequence_length = None if sc.use_varlen else host_lens[0]
        sc.current_batch_size = bs
        self.num_used_shared_caches += 1

    @torch.no_grad()
    def promote_unique_merged(self, base: int, rows: Tensor, lens: Tensor, host_path_lens, *, old_batch: int, max_len: Optional[int] = None,
                              staging: Optional[Tensor] = None, use_kernel: bool = True):
        """Fork with merged levels (hydragen_amd/fork.py gather_paths): sequence i of level `base` becomes the whole path of
        survivor rows[i] -- its parent's sequence in every level of [base, used), then the first lens[i] cached tokens of unique
        sequence rows[i] -- and the levels behind `base` are dropped: num_used_shared_caches = base + 1.  One hyd_kv_gather_paths
        launch (use_kernel=False: its torch definition) into `staging` ([2, >= sum(host_path_lens), Hkv, D] of the levels' dtype;
        None: allocated here -- a caller with many layers passes one and reuses it), then ONE contiguous copy_ each of K and V
        into slot `base`'s own buffers: the gather may not write what it reads (slot `base` is a chain level itself), and the
        slot keeps its addresses, so a captured decode graph of the same key -- batch sizes, varlen flags, sliced lengths --
        is replayed on it.  rows / lens: [k] device vectors; host_path_lens: the k path lengths in tokens on the host (the caller
        computed them to check the room: nothing is synchronised here); old_batch: the batch rows index into.  The slot is left
        exactly as SharedCache.fill leaves it for the concatenated paths, and fill's errors are raised before anything is written."""
        from .fork import gather_paths, gather_paths_reference

        base = int(base)
        used = self.num_used_shared_caches
        if not 0 <= base <= used:
            raise ValueError(f"merge_from {base} outside [0, {used}] (the levels in use)")
        if base >= self.get_num_total_shared_caches():
            raise ValueError(f"No more available shared caches: {used} {self.get_num_total_shared_caches()}")
        sc: SharedCache = self.shared_caches[base]
        host_path_lens = [int(x) for x in host_path_lens]
        bs, total = len(host_path_lens), sum(host_path_lens)
        if bs > sc.max_batch_size:
            raise ValueError(f"Batch size {bs} exceeds max batch size {sc.max_batch_size}")
        if max(host_path_lens) > sc.max_sequence_length:
            raise ValueError(f"Sequence length {max(host_path_lens)} exceeds max sequence length {sc.max_sequence_length}")
        if total > sc.k_cache.shape[0]:
            raise ValueError(f"{total} path tokens exceed the {sc.k_cache.shape[0]} tokens level {base} holds")
        if staging is None:
            staging = torch.empty((2, max(total, 1)) + tuple(sc.k_cache.shape[1:]), dtype=sc.k_cache.dtype, device=sc.k_cache.device)
        if staging.ndim != 4 or staging.shape[0] != 2 or staging.shape[1] < total or staging.shape[2:] != sc.k_cache.shape[1:] \
                or staging.dtype != sc.k_cache.dtype or not staging.is_contiguous():
            raise ValueError(f"staging must be a contiguous [2, >= {total}, {sc.k_cache.shape[1]}, {sc.k_cache.shape[2]}] {sc.k_cache.dtype} "
                             f"tensor, got {tuple(staging.shape)} {staging.dtype}")
        chain = [(c.k_cache, c.v_cache, c.cumsum_lengths, c.current_batch_size) for c in list(self.shared_caches)[base:used]]
        cu = (gather_paths if use_kernel else gather_paths_reference)(
            chain, self.per_completion_k_cache, self.per_completion_v_cache, rows, lens, staging[0], staging[1], old_batch=old_batch,
            max_len=max_len, max_path=max(host_path_lens), **self.scales())
        sc.k_cache[:total].copy_(staging[0, :total])
        sc.v_cache[:total].copy_(staging[1, :total])
        sc.seq_lens[:bs] = cu[1:] - cu[:-1]
        sc.cumsum_lengths[: bs + 1] = cu
        sc.use_varlen = max(host_path_lens) != min(host_path_lens)
        sc.sliced_sequence_length = None if sc.use_varlen else host_path_lens[0]
        sc.current_batch_size = bs
        self.num_used_shared_caches = base + 1


class AttentionMode:
    SHARED_PREFILL = "shared-prefill"
    UNIQUE_PREFILL = "unique-prefill"
    DECODE = "decode"


def shared_level_args(shared_caches: list[SharedCache]) -> dict:
    """The shared caches as the attention operators' level arguments (views only, no copies)."""
    keys, values, cu_seqlens, max_seqlens, use_varlens = [], [], [], [], []
    for sc in shared_caches:
        if sc.use_varlen:
            keys.append(sc.k_cache)
            values.append(sc.v_cache)
            cu_seqlens.append(sc.get_used_cumsum_lengths())
            max_seqlens.append(sc.max_sequence_length)
        else:
            b, s = sc.get_current_batch_size(), sc.sliced_sequence_length
            keys.append(sc.k_cache[: b * s].view(b, s, *sc.k_cache.shape[1:]))
            values.append(sc.v_cache[: b * s].view(b, s, *sc.v_cache.shape[1:]))
            cu_seqlens.append(None)
            max_seqlens.append(None)
        use_varlens.append(sc.use_varlen)
    return dict(shared_ks=keys, shared_vs=values, shared_cu_seq_lens=cu_seqlens, shared_max_seq_lens=max_seqlens, use_varlens=use_varlens)


def hydragen_attention_on_caches(q, k, v, shared_caches: list[SharedCache], seq_len: Optional[Tensor] = None, **scales):
    """llama.py:355-414: adapt the caches to the operator's arguments.  scales: k_scale / v_scale of fp8 unique caches (and
    causal_tail of a multi-token decode step)."""
    return hydragen_attention(q, k, v, **shared_level_args(shared_caches), seq_lens=seq_len, **scales)


class HydragenLlamaAttention(nn.Module):
    """llama.py:417-595."""

    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = config.get_head_dim()
        self.num_key_value_heads = config.num_key_value_heads
        self.disable_hydragen = False
        self.disable_attention = False
        if config.head_dim is None and self.head_dim * self.num_heads != self.hidden_size:
            raise ValueError(f"hidden_size must be divisible by num_heads (got `hidden_size`: {self.hidden_size} and `num_heads`: {self.num_heads}).")
        b = config.attention_bias
        self.q_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=b)
        self.k_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=b)
        self.v_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=b)
        self.o_proj = nn.Linear(self.num_heads * self.head_dim, self.hidden_size, bias=b)
        # per-head q/k RMSNorm (Qwen3; HF's state-dict names): one gain vector of head_dim elements for all query heads, one for
        # all key heads.  The fused decode preambles apply them inside the kernel, every other path calls the modules.
        self.q_norm = self.k_norm = None
        if config.qk_norm:
            if self.head_dim not in (64, 128, 256):
                raise NotImplementedError(f"qk_norm with head_dim {self.head_dim}: the per-head norm is implemented for 64 / 128 / 256")
            self.q_norm = RMSNorm(self.head_dim, eps=config.rms_norm_eps)
            self.k_norm = RMSNorm(self.head_dim, eps=config.rms_norm_eps)
        self.kv_cache: Optional[PerLayerKVCache] = None
        self.mode: Optional[str] = None
        self.rotary_emb: Optional[RotaryTable] = None
        self.tp_reduce = False  # row-parallel o_proj needs the all-reduce of tp.py:108-112
        self.use_fused_decode = True
        self._qkv: Optional[Tensor] = None
        self.qkv_proj = None  # weight_quant.Fp8Linear once the model is quantized (q_proj / k_proj / v_proj are then None)

    def _qk_norm_args(self) -> dict:
        """The gains and eps the fused preambles take (nothing without qk_norm)."""
        if self.q_norm is None:
            return {}
        return dict(q_norm=self.q_norm.weight, k_norm=self.k_norm.weight, norm_eps=self.q_norm.variance_epsilon)

    def _decode_multi(self, q, k, v, cos, sin, position_ids, shared_len):
        """Attention of a MULTI-TOKEN decode step (speculative.py): q / k / v [B, T, H, D] are T consecutive tokens per row,
        position_ids [B, T] their absolute positions (column 0 + i).  With the fused preamble: hyd_rope_append_multi, then the
        causal-tail operator; otherwise, and for a call the library refuses, the definition assembled from existing operators
        (speculative.assembled_causal_tail_attention).  Every token sees all shared keys and the unique keys up to itself.
        fp8 unique caches: the preamble quantizes the T new rows (hyd_rope_append_multi_kvq) and the fp8 causal-tail kernel reads
        the cache as it is; the assembled route -- a shape the library refuses, or use_fused_decode = False -- runs on
        dequantize_kv of the whole cache rows with the scales they were written with: functional, not fast."""
        bsz, q_len = q.shape[:2]
        kvc = self.kv_cache
        if not 2 <= q_len <= speculative.MAX_DRAFTS + 1:
            raise NotImplementedError(f"a decode step feeds 1 to {speculative.MAX_DRAFTS + 1} tokens per row, got {q_len}")
        if kvc.narrow or self.head_dim not in (64, 128, 256) or self.disable_attention:
            raise NotImplementedError("multi-token decode steps take unique caches of head dim 64 / 128 / 256 (no narrow head dims, no "
                                      "disable_attention)")
        if self.disable_hydragen:
            shared_len = None
        elif shared_len is None:
            shared_len = kvc.get_shared_len(bsz)
        shared = [] if self.disable_hydragen else kvc.get_used_shared_caches()
        if self.use_fused_decode:
            from .fused_decode import rope_append_multi

            q, seq_lens = rope_append_multi(q, k, v, cos, sin, position_ids, shared_len, kvc.per_completion_k_cache, kvc.per_completion_v_cache,
                                            **self._qk_norm_args(), **kvc.scales())
            ks, vs = kvc.per_completion_k_cache[:bsz], kvc.per_completion_v_cache[:bsz]
            try:
                if not shared:
                    return flash_attention_seqlen(q, ks, vs, seq_len=seq_lens, causal_tail=True, **kvc.scales())[0]
                return hydragen_attention_on_caches(q, ks, vs, shared, seq_len=seq_lens, causal_tail=True, **kvc.scales())
            except NotImplementedError:  # a shape the library refuses: the same attention from the existing launches
                pass
        else:
            unique_position_ids = position_ids if shared_len is None else position_ids - shared_len.unsqueeze(-1)
            if self.q_norm is not None:
                q, k = self.q_norm(q), self.k_norm(k)
            q, k = apply_rotary_pos_emb(q, k, cos, sin, position_ids)
            ks, vs = kvc.update_per_completion_kvs(unique_position_ids, k, v)
            seq_lens = unique_position_ids[:, -1] + 1
        if kvc.fp8:  # the assembled route reads 16-bit rows (its T x T block is a prefix-kernel pass)
            ks, vs = dequantize_kv(ks, kvc.k_scale, q.dtype), dequantize_kv(vs, kvc.v_scale, q.dtype)
        return speculative.assembled_causal_tail_attention(q, ks, vs, seq_lens, **shared_level_args(shared))

    def forward(self, hidden_states: Tensor, position_ids: Tensor, shared_len: Optional[Tensor] = None):
        """shared_len: the per-sequence total shared length [B] (get_shared_len) when the caller already has it -- it is
        the same for every layer of a forward pass, and computing it is three small launches (~17 us) per layer."""
        bsz, q_len, _ = hidden_states.shape
        if self.qkv_proj is not None:  # fp8 weights (quantize_weights): q|k|v is one module, _fused_weight has nothing to fuse
            nq, nk = self.num_heads * self.head_dim, self.num_key_value_heads * self.head_dim
            q, k, v = self.qkv_proj(hidden_states).split([nq, nk, nk], dim=-1)
        else:
            self._qkv = w = _fused_weight(self._qkv, (self.q_proj, self.k_proj, self.v_proj))
            if w is not None:
                nq, nk = self.q_proj.weight.shape[0], self.k_proj.weight.shape[0]
                q, k, v = nn.functional.linear(hidden_states, w).split([nq, nk, nk], dim=-1)
            else:
                q, k, v = self.q_proj(hidden_states), self.k_proj(hidden_states), self.v_proj(hidden_states)
        q = q.view(bsz, q_len, self.num_heads, self.head_dim)
        k = k.view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        v = v.view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        cos, sin = self.rotary_emb.cos_cached, self.rotary_emb.sin_cached

        if self.mode == AttentionMode.DECODE and q_len > 1:
            out = self.o_proj(self._decode_multi(q, k, v, cos, sin, position_ids, shared_len).reshape(bsz, q_len, -1))
            return all_reduce_sum(out) if self.tp_reduce else out
        fused = self.mode == AttentionMode.DECODE and self.use_fused_decode and q_len == 1
        if fused:
            # one HIP kernel: RoPE(q, k) at absolute positions, append k/v at (position - shared length),
            # seq_lens = that index + 1  (replaces llama.py:485-501,565-569 and the scatter_ of :236-262)
            from .fused_decode import rope_append_decode

            if self.disable_hydragen:
                shared_len = None
            elif shared_len is None:
                shared_len = self.kv_cache.get_shared_len(bsz)
            sc = self.kv_cache.scales()
            if self.head_dim not in (64, 128, 256) and not self.kv_cache.narrow:
                raise NotImplementedError(f"head_dim {self.head_dim}: the fused decode preamble takes 64, 128 and 256, or narrow unique "
                                          "caches (narrow_kv_head_dim); set use_fused_decode = False")
            # narrow unique caches: the preamble takes head_dim-wide q / k / v and caches and returns q at the kernels' head dim with
            # zero pad columns; the operators then copy nothing (shared caches that wide, the unique cache as it is) and so is their output
            q, seq_lens = rope_append_decode(q, k, v, cos, sin, position_ids, shared_len,
                                             self.kv_cache.per_completion_k_cache, self.kv_cache.per_completion_v_cache, **sc,
                                             **self._qk_norm_args())
            key_states = self.kv_cache.per_completion_k_cache[:bsz]
            value_states = self.kv_cache.per_completion_v_cache[:bsz]
            if self.disable_attention:
                # llama.py:433-437,503-504: attention replaced by the identity on the rotated q.  The same preamble kernel as
                # the other modes, so that this mode's step is the decode step minus exactly the attention kernels.
                attn_output = q
            elif not self.kv_cache.has_shared() or self.disable_hydragen:
                attn_output, _ = flash_attention_seqlen(q, key_states, value_states, seq_len=seq_lens, **sc)
            else:
                attn_output = hydragen_attention_on_caches(q, key_states, value_states,
                                                           self.kv_cache.get_used_shared_caches(), seq_len=seq_lens, **sc)
            if self.kv_cache.narrow:  # one copy of B x Hq x head_dim elements: o_proj reads the true columns
                attn_output = attn_output[..., : self.head_dim]
            out = self.o_proj(attn_output.reshape(bsz, q_len, -1))
            return all_reduce_sum(out) if self.tp_reduce else out

        if self.disable_hydragen:
            unique_position_ids = position_ids
        else:
            unique_position_ids = position_ids - self.kv_cache.get_shared_len(position_ids.shape[0]).unsqueeze(-1)
        if self.q_norm is not None:  # prefill, use_fused_decode = False, CPU models: the modules, then the rotation
            q, k = self.q_norm(q), self.k_norm(k)
        q, k = apply_rotary_pos_emb(q, k, cos, sin, position_ids)
        if self.kv_cache is not None and self.kv_cache.kv_amax is not None and self.mode in (AttentionMode.SHARED_PREFILL, AttentionMode.UNIQUE_PREFILL):
            # calibrated fp8 scales: this prefill's K / V before any of it is stored.  A shared level stores the rows inside the
            # lengths, a unique prefill every row it is given
            lens = (unique_position_ids.max(1).values + 1).to(torch.int32) if self.mode == AttentionMode.SHARED_PREFILL else None
            self.kv_cache.observe_kv(k, v, lens)

        if self.disable_attention:
            attn_output = q
        elif self.mode == AttentionMode.SHARED_PREFILL:
            if not self.kv_cache.has_shared():
                attn_output, _ = flash_attention(q, k, v, causal=True)
            else:
                attn_output = hydragen_attention_on_caches(q, k, v, self.kv_cache.get_used_shared_caches())
            self.kv_cache.append_shared(k, v, unique_position_ids.max(1).values + 1)
        elif self.mode == AttentionMode.UNIQUE_PREFILL:
            if self.disable_hydragen:
                ks, vs = self.kv_cache.update_per_completion_kvs(unique_position_ids, k, v)
                n = int(unique_position_ids.max().item()) + 1
                ks, vs = ks[:, :n], vs[:, :n]
                if self.kv_cache.fp8:  # the 16-bit prefix kernel reads the cache: dequantized rows
                    ks, vs = dequantize_kv(ks, self.kv_cache.k_scale, q.dtype), dequantize_kv(vs, self.kv_cache.v_scale, q.dtype)
                attn_output, _ = flash_attention(q, ks, vs, causal=True)
            else:
                if not self.kv_cache.has_shared():
                    attn_output, _ = flash_attention(q, k, v, causal=True)
                else:
                    attn_output = hydragen_attention_on_caches(q, k, v, self.kv_cache.get_used_shared_caches())
                self.kv_cache.update_per_completion_kvs(unique_position_ids, k, v)
        elif self.mode == AttentionMode.DECODE:
            ks, vs = self.kv_cache.update_per_completion_kvs(unique_position_ids, k, v)
            seq_lens = unique_position_ids.squeeze(-1) + 1
            sc = self.kv_cache.scales()
            if not self.kv_cache.has_shared() or self.disable_hydragen:
                attn_output, _ = flash_attention_seqlen(q, ks, vs, seq_len=seq_lens, **sc)
            else:
                attn_output = hydragen_attention_on_caches(q, ks, vs, self.kv_cache.get_used_shared_caches(), seq_len=seq_lens,
                                                           **sc)
        else:
            raise ValueError(f"Unknown mode {self.mode}")

        out = self.o_proj(attn_output.reshape(bsz, q_len, -1))
        return all_reduce_sum(out) if self.tp_reduce else out


class HydragenLlamaDecoderLayer(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.self_attn = HydragenLlamaAttention(config)
        self.mlp = LlamaMLP(config)
        self.input_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, hidden_states, position_ids):
        hidden_states = hidden_states + self.self_attn(self.input_layernorm(hidden_states), position_ids)
        return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))


class HydragenLlamaModel(nn.Module):
    """llama.py:636-765."""

    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size, config.pad_token_id)
        self.layers = nn.ModuleList([HydragenLlamaDecoderLayer(config) for _ in range(config.num_hidden_layers)])
        self.norm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.rotary_emb = RotaryTable(config.get_head_dim(), config.max_position_embeddings, config.rope_theta)
        for layer in self.layers:
            layer.self_attn.rotary_emb = self.rotary_emb

    def set_disable_hydragen(self, disable=True):
        for layer in self.layers:
            layer.self_attn.disable_hydragen = disable

    def get_disable_hydragen(self):
        return self.layers[0].self_attn.disable_hydragen

    def set_disable_attention(self, disable=True):
        for layer in self.layers:
            layer.self_attn.disable_attention = disable

    def get_disable_attention(self):
        return self.layers[0].self_attn.disable_attention

    def copy_shared_cache_to_unique(self, total_num_sequences):
        for layer in self.layers:
            layer.self_attn.kv_cache.copy_shared_to_unique(total_num_sequences)

    def _used(self):
        return self.layers[0].self_attn.kv_cache.get_used_shared_caches()

    def get_shared_batch_sizes(self):
        return [c.get_current_batch_size() for c in self._used()]

    def get_shared_varlens(self):
        return [c.use_varlen for c in self._used()]

    def get_shared_slice_seq_lens(self):
        return [c.sliced_sequence_length for c in self._used()]

    def forward(self, input_ids, position_ids):
        h = self.embed_tokens(input_ids)
        layers = list(self.layers)
        w0 = self.norm.weight
        if not layers or not layer_ops.supported(h) or w0.dtype != h.dtype:
            for layer in layers:  # CPU / fp32 / odd widths: the spelled-out layer (llama.py:610-633)
                h = layer(h, position_ids=position_ids)
            return self.norm(h)
        # Same dataflow with every residual add fused into the norm that consumes it (llama.py:615-631: `residual +
        # hidden_states`, then the next LlamaRMSNorm): one kernel that reads the block output and the residual stream
        # once and writes the new stream and its normalised form, instead of an add and a norm launch per block.
        first = layers[0].input_layernorm
        _, normed = layer_ops.add_rms_norm(h, None, first.weight, first.variance_epsilon)
        # decode: the shared lengths (llama.py:317-330) once per forward instead of once per layer -- the layers' caches are
        # filled in lockstep, so every layer would compute the same [B] tensor with three small launches
        a0 = layers[0].self_attn
        shared_len = None
        if a0.mode == AttentionMode.DECODE and a0.kv_cache is not None and not a0.disable_hydragen and h.shape[1] <= 8:
            shared_len = a0.kv_cache.get_shared_len(h.shape[0])
        for i, layer in enumerate(layers):
            post = layer.post_attention_layernorm
            h, normed = layer_ops.add_rms_norm(layer.self_attn(normed, position_ids, shared_len=shared_len), h, post.weight,
                                               post.variance_epsilon)
            nxt = layers[i + 1].input_layernorm if i + 1 < len(layers) else self.norm
            h, normed = layer_ops.add_rms_norm(layer.mlp(normed), h, nxt.weight, nxt.variance_epsilon)
        return normed


@dataclass
class CaptureData:
    graph: "torch.cuda.CUDAGraph"
    static_input_ids: Tensor
    static_position_ids: Tensor
    static_hidden: Tensor
    key: tuple


class GraphedHydragenLlamaModel(nn.Module):
    """HIP-graph replay of the decode forward; re-captures on the same invalidation keys as
    llama.py:791-823 (shapes, shared batch sizes, varlen flags, sliced lengths, disable flags)."""

    def __init__(self, model: HydragenLlamaModel):
        super().__init__()
        self.model = model
        self.capture_data: Optional[CaptureData] = None

    def invalidate(self):
        self.capture_data = None

    def _key(self, input_ids, position_ids):
        m = self.model
        order = _flash.current_seq_order()  # (its pointer is baked into the captured launches)
        return (tuple(input_ids.shape), tuple(position_ids.shape), tuple(m.get_shared_batch_sizes()),
                m.get_disable_hydragen(), m.get_disable_attention(), tuple(m.get_shared_varlens()),
                tuple(m.get_shared_slice_seq_lens()), None if order is None else (order.data_ptr(), order.numel()))

    def forward(self, input_ids, position_ids):
        key = self._key(input_ids, position_ids)
        if self.capture_data is not None and self.capture_data.key != key:
            self.invalidate()
        if self.capture_data is None:
            self.capture(input_ids, position_ids, key)
        self.capture_data.static_input_ids.copy_(input_ids)
        self.capture_data.static_position_ids.copy_(position_ids)
        self.capture_data.graph.replay()
        return self.capture_data.static_hidden

    def capture(self, input_ids, position_ids, key):
        static_input_ids = input_ids.clone()
        static_position_ids = position_ids.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):  # warm-up on a side stream (llama.py:838-845)
                self.model(input_ids=static_input_ids, position_ids=static_position_ids)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_hidden = self.model(input_ids=static_input_ids, position_ids=static_position_ids)
        self.capture_data = CaptureData(g, static_input_ids, static_position_ids, static_hidden, key)


class SharedCacheOp:
    WIPE = "wipe"
    EXTEND = "extend"
    PRESERVE = "preserve"


class HydragenLlamaForCausalLM(nn.Module):
    """llama.py:875-1422."""

    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        self.model = HydragenLlamaModel(config)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.kv_cache_allocated = False
        self.weights_quantized = False  # quantize_weights()
        self.graphed_model: Optional[GraphedHydragenLlamaModel] = None
        self.mode: Optional[str] = None
        # one presence bitmap [sb, ceil(V / 32)] int32 per used shared level, recorded by append_shared (the penalties' context)
        self.shared_bitmaps: list[Tensor] = []

    # ---- construction -----------------------------------------------------------------------------
    @classmethod
    def from_config(cls, config: LlamaConfig, dtype=torch.bfloat16, device="cuda", seed: int = 0, std: float = 0.02,
                    tp_shard: Optional[tuple] = None):
        """Random-weight model of the given architecture (synthetic benchmarks / tests).  `tp_shard=(rank, world)`
        builds only that rank's tensor-parallel shard (tp.py:115-132) without ever materialising the full model."""
        if tp_shard is not None:
            from copy import deepcopy
            from .tp import apply_tp

            with torch.device("meta"):
                model = cls(deepcopy(config))
            apply_tp(model.model, rank=tp_shard[0], world_size=tp_shard[1])
            model.to_empty(device=device)
            c = model.config
            model.model.rotary_emb = RotaryTable(c.get_head_dim(), c.max_position_embeddings, c.rope_theta, device=device)
            for layer in model.model.layers:
                layer.self_attn.rotary_emb = model.model.rotary_emb
            with torch.no_grad():
                for prm in model.parameters():
                    if prm.ndim == 1:
                        prm.fill_(1.0)  # RMSNorm gains
        else:
            with torch.device(device):
                model = cls(config)
        model.to(dtype=dtype)
        model.model.rotary_emb.float()  # cos/sin tables stay fp32 (cast per use, like HF's rotary embedding)
        g = torch.Generator(device=device).manual_seed(seed)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if p.ndim >= 2:
                    p.normal_(0.0, std, generator=g)
        model.device, model.dtype = torch.device(device), dtype
        return model

    @classmethod
    def from_pretrained(cls, model_name_or_path: str, **kwargs):
        """llama.py:1398-1422.  Needs `transformers` weights on disk; not exercised offline.  Llama and Qwen3 checkpoints."""
        from transformers import AutoModelForCausalLM  # pragma: no cover

        return cls.from_hf_model(AutoModelForCausalLM.from_pretrained(model_name_or_path, **kwargs))  # pragma: no cover

    @classmethod
    def from_hf_model(cls, hf):
        """The model of an in-memory transformers `LlamaForCausalLM` or `Qwen3ForCausalLM` (fp16 / bf16): its config mapped onto
        LlamaConfig -- `head_dim` where the config states one, `qk_norm` when the state dict carries `self_attn.q_norm` or the
        model type is qwen3 -- and its state dict loaded, every tensor accounted for."""
        if hf.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"Model must be in float16 or bfloat16, not {hf.dtype}")
        c = hf.config
        kind = getattr(c, "model_type", "llama")
        if kind not in ("llama", "qwen3"):
            raise NotImplementedError(f"model type '{kind}': llama and qwen3 are implemented")
        if getattr(c, "use_sliding_window", False):
            raise NotImplementedError("sliding-window attention is not implemented")
        sd = hf.state_dict()
        rp = getattr(c, "rope_parameters", None) or {}
        cfg = LlamaConfig(c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads,
                          c.num_key_value_heads, c.vocab_size, c.rms_norm_eps,
                          getattr(c, "rope_theta", rp.get("rope_theta", 10000.0)), c.max_position_embeddings,
                          getattr(c, "attention_bias", False), c.pad_token_id, getattr(c, "head_dim", None),
                          kind == "qwen3" or any(k.endswith("self_attn.q_norm.weight") for k in sd))
        scaling = getattr(c, "rope_scaling", None) or {}
        rope = scaling.get("rope_type", scaling.get("type", "default")) or rp.get("rope_type", "default")
        if rope not in ("default", None):
            raise NotImplementedError(f"rope scaling '{rope}' is not implemented (plain theta-only RoPE tables)")
        model = cls(cfg)
        report = model.load_state_dict(sd, strict=False)
        extra = [k for k in report.unexpected_keys if "inv_freq" not in k]
        if report.missing_keys or extra:
            raise RuntimeError(f"checkpoint does not match: missing {report.missing_keys[:5]}, unexpected {extra[:5]}")
        model.to(device=hf.device, dtype=hf.dtype)
        model.model.rotary_emb.float()
        model.device, model.dtype = hf.device, hf.dtype
        return model

    # ---- cache / graph management -------------------------------------------------------------------
    def set_mode(self, mode):
        self.mode = mode
        for layer in self.model.layers:
            layer.self_attn.mode = mode

    def graph(self, do_graph: bool = True):
        """Controls whether decoding replays a HIP graph (llama.py:898-907)."""
        if do_graph:
            if self.graphed_model is None:
                self.graphed_model = GraphedHydragenLlamaModel(self.model)
        else:
            self.graphed_model = None

    def quantize_weights(self, dtype: torch.dtype = FP8_DTYPE, skip=("lm_head",)) -> None:
        """Store the decoder layers' linear weights in fp8 (weight_quant.py: e4m3fn codes with one power-of-two scale per output
        channel; activations, accumulators and outputs stay 16-bit) and release the 16-bit storage.  q|k|v and gate|up become one
        Fp8Linear each (`self_attn.qkv_proj`, `mlp.gate_up_proj`: the projections are quantized one by one and concatenated, so
        fusing changes no value; `q_proj` ... `up_proj` become None), o_proj and down_proj are replaced in place.  `skip` names
        modules to leave alone: "lm_head" (the default; remove it to quantize the head too), or any of "qkv_proj", "o_proj",
        "gate_up_proj", "down_proj".  The embedding is never quantized.  Call it after the weights are loaded and after apply_tp
        (a rank quantizes its own shards); a second call, and apply_tp / make_tp_files afterwards, raise.  A step with up to
        weight_quant.W8_MAX_ROWS rows (batch x tokens per row) runs hyd_linear_w8, larger ones widen the weight into one scratch
        buffer of the model (sized here for the largest quantized weight, so that no forward allocates and captured graphs hold
        static addresses) and run the 16-bit GEMM on it.  state_dict() carries `weight` / `weight_scale` of the new modules;
        loading it into a model quantized the same way restores it bit for bit."""
        if dtype != FP8_DTYPE:
            raise NotImplementedError(f"quantize_weights(dtype={dtype}): {FP8_DTYPE} is the one format")
        if self.weights_quantized:
            raise RuntimeError("quantize_weights() was already called on this model")
        skip = set(skip)
        unknown = skip - {"lm_head", "qkv_proj", "o_proj", "gate_up_proj", "down_proj"}
        if unknown:
            raise ValueError(f"quantize_weights(skip=...): unknown module names {sorted(unknown)}")
        if any(p.device.type == "meta" for p in self.parameters()):
            raise RuntimeError("quantize_weights() needs loaded weights (the model is on the meta device)")
        self.maybe_invalidate()
        unfuse_weights(self.model)  # every projection owns its rows again: the fused 16-bit tensors are released with them
        scratch = W8Scratch()
        for layer in self.model.layers:
            attn, mlp = layer.self_attn, layer.mlp
            if "qkv_proj" not in skip:
                attn.qkv_proj = Fp8Linear.from_linears((attn.q_proj, attn.k_proj, attn.v_proj), scratch)
                attn.q_proj = attn.k_proj = attn.v_proj = None
            if "o_proj" not in skip:
                attn.o_proj = Fp8Linear.from_linears((attn.o_proj,), scratch)
            if "gate_up_proj" not in skip:
                mlp.gate_up_proj = Fp8Linear.from_linears((mlp.gate_proj, mlp.up_proj), scratch)
                mlp.gate_proj = mlp.up_proj = None
            if "down_proj" not in skip:
                mlp.down_proj = Fp8Linear.from_linears((mlp.down_proj,), scratch)
        if "lm_head" not in skip:
            self.lm_head = Fp8Linear.from_linears((self.lm_head,), scratch)
        self.weights_quantized = True

    def maybe_invalidate(self):
        if self.graphed_model is not None:
            self.graphed_model.invalidate()

    def get_num_heads(self):
        return self.config.num_attention_heads

    def setup_caches(self, max_unique_batch_size: int, max_unique_seq_length: int,
                     max_shared_batch_sizes: list[int], max_shared_seq_lengths: list[int], kv_cache_dtype: Optional[torch.dtype] = None,
                     kv_scales: str = "unit", kv_scale_margin: float = 2.0):
        """Allocate the unique KV cache and the shared cache levels at every layer (llama.py:921-955).  kv_cache_dtype =
        torch.float8_e4m3fn makes every layer's unique arena fp8 (half the bytes; per-kv-head k_scale / v_scale buffers on each
        PerLayerKVCache); None = the model's dtype.  Shared caches stay in the model's dtype.

        kv_scales (fp8 caches only; anything but "unit" on a 16-bit cache is a ValueError): "unit" keeps every scale at 1.0 and
        launches nothing new.  "calibrate" sets them per layer and kv head from the prompts' K / V (kv_quant.py): every shared and
        unique prefill folds max |K| (after RoPE) and max |V| of its 16-bit K / V into the layer's kv_amax [2, Hkv] (one
        hyd_kv_absmax launch per layer and prefill; decode steps observe nothing), and scale = the smallest power of two >=
        amax * kv_scale_margin / 448.  The scales are rewritten only while the layer's unique cache holds no live row: generate()
        and score() open a window when they start, and the first write to the unique cache of that call closes it, writing the
        scales once -- copy_shared_to_unique (no-sharing mode), the unique prefill's store after its own K / V were observed, or
        else the call's first decode step.  Outside a window they never change: an append_shared() between a generate() and a
        fork() observes but does not rescale, and fork() widens fp8 rows with the scales they were written with.  kv_amax is
        zeroed whenever no shared level is left in use (empty_shared_cache, truncate_shared_caches(0), the "preserve" truncation of
        a generate() that started from none, setup_caches): a fresh hierarchy is calibrated from its own prompts; kept levels
        ("extend", fork flows) keep the running maximum, so a scale never shrinks under rows that are alive.  reset_kv_scales()
        zeroes the maxima and sets the scales back to 1.0.  A tensor-parallel rank calibrates its own kv heads: no collective.
        Limits: the K / V of generated tokens, and of unique prompts in the no-sharing mode (disable_hydragen: the copied prefix
        closes the window first), are not observed before they are written -- kv_scale_margin is their headroom, beyond it the
        quantizer's clamp at +-448 * scale applies, as with scale 1.  Calibration fixes range, not mantissa (kv_quant.py)."""
        self.maybe_invalidate()
        max_unique_seq_length = (max_unique_seq_length + 15) // 16 * 16
        head_dim = self.config.get_head_dim()
        device, dtype = self.lm_head.weight.device, self.model.embed_tokens.weight.dtype  # (the lm_head's weight may be fp8)
        # the layers' unique caches, placed where the suffix pass streams them fastest (placement.py: more candidates than layers
        # are allocated, each timed once with the suffix pass over all of its keys, the slowest go back; off the data path)
        self.kv_cache_allocated = False
        for layer in self.model.layers:
            layer.self_attn.kv_cache = None  # a second setup_caches: the old arenas are free before the candidates are made
        udtype = dtype if kv_cache_dtype is None else kv_cache_dtype
        if udtype not in (dtype, FP8_DTYPE):
            raise NotImplementedError(f"kv_cache_dtype {kv_cache_dtype}: the model's {dtype} or {FP8_DTYPE}")
        arenas, self.kv_placement = placement.place_kv_arenas(
            len(self.model.layers), (max_unique_batch_size, max_unique_seq_length, self.config.num_key_value_heads, head_dim),
            udtype, device, self.config.num_attention_heads, q_dtype=dtype)
        for layer, arena in zip(self.model.layers, arenas):
            layer.self_attn.kv_cache = PerLayerKVCache(
                max_unique_batch_size=max_unique_batch_size, max_unique_seq_length=max_unique_seq_length,
                max_shared_batch_sizes=max_shared_batch_sizes, max_shared_seq_lengths=max_shared_seq_lengths,
                n_kv_heads=self.config.num_key_value_heads, head_dim=head_dim, device=device, dtype=dtype, arena=arena,
                kv_cache_dtype=udtype, n_q_heads=self.config.num_attention_heads, kv_scales=kv_scales,
                kv_scale_margin=kv_scale_margin)
        # the decode loop's schedule hint (flash.seq_order): one buffer for the model's lifetime, so that a captured decode graph
        # keeps pointing at the current generation's order
        self.seq_order_buf = torch.arange(max_unique_batch_size, dtype=torch.int32, device=device)
        self.kv_cache_allocated = True

    def empty_shared_cache(self):
        for layer in self.model.layers:
            layer.self_attn.kv_cache.empty_shared_cache()
        self.shared_bitmaps.clear()

    def reset_kv_scales(self):
        """Calibrated fp8 scales (setup_caches kv_scales="calibrate"): zero every layer's running maxima and set the scales back
        to 1.0, in place."""
        for layer in self.model.layers:
            layer.self_attn.kv_cache.reset_kv_scales()

    def _scale_windows(self, op: str, **kw):
        for layer in self.model.layers:
            getattr(layer.self_attn.kv_cache, op)(**kw)

    def truncate_shared_caches(self, new_num_shared_caches: int):
        for layer in self.model.layers:
            layer.self_attn.kv_cache.truncate_shared_caches(new_num_shared_caches)
        del self.shared_bitmaps[new_num_shared_caches:]

    def get_shared_cache_len(self, batch_size):
        return self.model.layers[0].self_attn.kv_cache.get_shared_len(batch_size)

    def get_num_used_shared_caches(self):
        return self.model.layers[0].self_attn.kv_cache.num_used_shared_caches

    def repeat_per_completion_cache_for_num_samples(self, current_size, num_samples):
        for layer in self.model.layers:
            layer.self_attn.kv_cache.repeat_per_completion_cache_for_num_samples(current_size, num_samples)

    # ---- forward -------------------------------------------------------------------------------------
    def forward(self, input_ids, position_ids, seq_lens=None, use_graph=False, full_logits=False, raw_logits=False):
        """Logits in fp32 as the reference returns them (llama.py:1063-1070); raw_logits=True keeps the lm_head's own
        dtype (the decode loop's fused sampler reads them once, without the fp32 copy)."""
        model = self.graphed_model if use_graph else self.model
        assert model is not None
        hidden = model(input_ids=input_ids, position_ids=position_ids)
        if full_logits:
            to_lm_head = hidden
        elif seq_lens is not None:
            to_lm_head = hidden[torch.arange(hidden.shape[0], device=hidden.device), seq_lens - 1].unsqueeze(1)
        else:
            to_lm_head = hidden[:, -1:]
        logits = self.lm_head(to_lm_head)
        return logits if raw_logits else logits.float()

    def apply_top_p(self, logits, top_p, min_tokens_to_keep=1, filter_value=-float("Inf")):
        return sampling.apply_top_p(logits, top_p, min_tokens_to_keep, filter_value)

    def sample_route(self, cuda, unit_rows, temperature, num_samples=1, top_p=None, top_k=None, min_p=None, return_logprobs=False,
                     penalties=None, constraint=None, seed=None, offset=0) -> sampling.SampleRoute:
        """sampling.sample_route of a sample_from_logits call on logits that are on the GPU (cuda) and 2-D of unit last stride
        (unit_rows), with the model's two switches as they are now."""
        if generation.per_row_sampling(temperature, top_k, top_p, min_p, penalties, seed):
            return sampling.sample_route(cuda, cuda and unit_rows, cuda, num_samples, constraint is not None,
                                         penalties is not None and penalties.active(), True, return_logprobs, per_row=True)
        ok = cuda and temperature >= 0
        return sampling.sample_route(cuda, ok and unit_rows, ok, num_samples, constraint is not None,
                                     penalties is not None and penalties.active(), sampling.filters_active(top_k, top_p, min_p),
                                     return_logprobs, self.fused_sampling_filters, self.fused_sampling_penalties)

    def sample_from_logits(self, logits, temperature, num_samples=1, top_p=None, top_k=None, min_p=None,
                           return_logprobs=False, penalties=None, constraint=None, seed=None, offset=0):
        """Tokens [B, num_samples] (and, with return_logprobs, their fp32 log softmax(logits) [B, num_samples]).  The cuts
        act on the unscaled softmax(logits), before the temperature (hydragen_amd/sampling.py).  penalties (a
        layer_ops.Penalties with something switched on): cuts, draw and log-prob act on the penalised logits instead; the
        drawn tokens are appended to its list when it says so.  constraint = (dfa, state int32 [B * num_samples]): every rule
        acts on the logits behind the automaton's mask and `state` advances in place.  Which kernel or torch stage does what
        is sampling.sample_route's table; generate() decides it once for its first draw and once for its steps.  temperature,
        the cuts and the penalties' scalars may be per row (lists or [B * num_samples] tensors), seed one integer per row with
        offset (layer_ops.sample_tokens): the per_row routes, one launch whatever num_samples is."""
        args = (temperature, num_samples, top_p, top_k, min_p, return_logprobs, penalties, constraint, seed, offset)
        route = self.sample_route(logits.is_cuda, logits.ndim == 2 and logits.stride(-1) == 1, *args)
        tok, lp = generation.draw_tokens(route, logits, *args)
        return (tok, lp) if return_logprobs else tok

    def _positions(self, input_ids):
        shared_lens = self.get_shared_cache_len(input_ids.shape[0])
        n = input_ids.shape[1]
        return shared_lens[:, None] + torch.arange(n, device=input_ids.device, dtype=torch.long)[None, :]

    @torch.no_grad()
    def append_shared(self, input_ids, seq_lens=None, full_logits=False):
        """Add a new level of shared cache (llama.py:1073-1116).  Padding on the right."""
        self.set_mode(AttentionMode.SHARED_PREFILL)
        position_ids = self._positions(input_ids)
        if seq_lens is not None:
            last = position_ids.gather(1, (seq_lens.long() - 1)[:, None])
            ar = torch.arange(input_ids.shape[1], device=input_ids.device)[None, :]
            position_ids = torch.where(ar >= seq_lens.long()[:, None], last, position_ids)
        logits = self(input_ids=input_ids, position_ids=position_ids, seq_lens=seq_lens, full_logits=full_logits)
        # the level's token set, for the sampling penalties (hydragen_amd/sampling.py): ALWAYS recorded, because a level
        # outlives the call that appends it ("extend", starting_logits=) and a later call may ask for penalties; it is one
        # memset and one launch next to a prefill forward, keeps no reference to the caller's tensor, and syncs nothing.
        # After the forward: a refused level (no free shared cache) leaves the list as it was
        del self.shared_bitmaps[self.get_num_used_shared_caches() - 1:]
        lens = None if seq_lens is None else seq_lens.to(input_ids.device)
        self.shared_bitmaps.append(layer_ops.token_bitmap(input_ids.long(), lens, self.vocab_size))
        return logits

    @torch.no_grad()
    def fork(self, rows, seq_lens, token_ids, old_batch: int, use_kernel: bool = True, merge_from: Optional[int] = None) -> int:
        """Promote completions of the previous decode batch to a new shared level, without a forward pass: the first seq_lens[i]
        cached tokens of unique sequence rows[i] become sequence i of the next free shared level at every layer (one
        hyd_kv_promote launch per layer; use_kernel=False: the torch definition, hydragen_amd/fork.py).  The level comes directly
        after the levels in use, so the rows' absolute RoPE positions stay valid.  Returns the number of levels in use.

        rows [k]: batch indices of the previous decode batch of `old_batch` sequences (a list or a tensor); old_batch is passed
        explicitly -- it cannot be told from the rows, and the rule below depends on it.  seq_lens [k]: cached tokens to promote, each
        at least 1 and at most what is cached.  token_ids [k, max(seq_lens)] (right-padded): the tokens those K/V rows belong to --
        their set is recorded next to the level for the sampling penalties, as append_shared does, because a later call may ask
        for penalties.  check_fork_rows (fork.py) must hold for the levels in use: the same number of survivors under every shared
        sequence of every level, listed in group order.  Every check runs on the host before the first launch; one host
        synchronisation if rows / seq_lens are device tensors, none per layer.  A captured decode graph stays valid: its key holds
        the levels' batch sizes, varlen flags and sliced lengths, and the level's buffers (K/V, lengths, offsets) are static.

        What is cached: after a generate() that returned n tokens, row b holds unique_prompt_len + n - 1 tokens in the unique
        cache -- its own prompt, then returned tokens 0 .. n - 2 (token_overrides where given): the last returned token was never
        fed.  On the stop-condition path a row that finished with `length` kept tokens holds at least unique_prompt_len + length - 1
        (a finished row is no longer fed; a stop sequence that was cut had its first tokens fed before it matched, they sit
        behind those and need not be promoted).  To continue, pass each survivor's first uncached token as a one-token unique
        prompt: generate(input_ids=last[rows].repeat_interleave(m, 0)[:, None], num_return_sequences=1, ...) samples every
        survivor m times and uses one level per fork.  Tensor-parallel ranks call fork with the same arguments: the caches are
        per-rank head shards, nothing else changes.

        merge_from=base (0 <= base <= levels in use; None: everything above, unchanged): fork with merged levels.  The levels
        [base, used) -- the chain earlier forks left -- and the promoted rows are gathered into ONE level that replaces them
        (PerLayerKVCache.promote_unique_merged: one hyd_kv_gather_paths launch and one copy per layer): sequence i of level
        `base` becomes survivor i's whole path, its parent's sequence in every chain level and then its own seq_lens[i] tokens
        (0 is allowed: the path alone), and base + 1 levels are in use afterwards, however many forks came before.  ANY distinct
        rows may survive: check_fork_rows has to hold for the levels below `base` only (the prompt's), so two children of one
        path and none of another is a valid selection -- what a global top-k needs.  Slot `base` must hold k sequences, each
        path must fit its max_sequence_length and their total its capacity.  The chain levels' lengths are read from the device
        once; every check runs on the host before the first launch, and a refused call leaves the levels, their count and the
        bitmaps as they were.  shared_bitmaps[base] becomes, per survivor, the OR of its parents' bitmap rows in the chain
        levels and token_bitmap(token_ids, seq_lens): the bitmap of the whole path's tokens.  merge_from == used is a chain of
        no levels: the same level bytes and logits as the plain fork."""
        from .fork import check_fork_rows

        if not self.kv_cache_allocated:
            raise RuntimeError("call setup_caches() before fork()")
        rows_l = [int(x) for x in (rows.tolist() if isinstance(rows, Tensor) else rows)]
        lens_l = [int(x) for x in (seq_lens.tolist() if isinstance(seq_lens, Tensor) else seq_lens)]
        k = len(rows_l)
        if k == 0 or len(lens_l) != k:
            raise ValueError(f"fork of {k} rows with {len(lens_l)} lengths")
        kv = self.model.layers[0].self_attn.kv_cache
        max_batch, room = kv.per_completion_k_cache.shape[:2]
        if not 1 <= int(old_batch) <= max_batch:
            raise ValueError(f"old_batch {old_batch}: the unique cache holds {max_batch} sequences")
        if merge_from is not None:
            return self._fork_merged(rows_l, lens_l, token_ids, int(old_batch), use_kernel, merge_from)
        check_fork_rows(rows_l, old_batch, [c.current_batch_size for c in kv.get_used_shared_caches()])
        if min(lens_l) < 1 or max(lens_l) > room:
            raise ValueError(f"seq_lens {lens_l}: each at least 1 and at most the {room} tokens a unique sequence caches")
        if not isinstance(token_ids, Tensor) or token_ids.ndim != 2 or token_ids.shape != (k, max(lens_l)):
            raise ValueError(f"token_ids must be [{k}, {max(lens_l)}] (right-padded to the longest promoted length), got "
                             f"{tuple(token_ids.shape) if isinstance(token_ids, Tensor) else type(token_ids)}")
        used = kv.num_used_shared_caches
        if used >= kv.get_num_total_shared_caches():
            raise ValueError(f"No more available shared caches: {used} {kv.get_num_total_shared_caches()}")
        sc = kv.shared_caches[used]
        if k > sc.max_batch_size:
            raise ValueError(f"Batch size {k} exceeds max batch size {sc.max_batch_size}")
        if max(lens_l) > sc.max_sequence_length:
            raise ValueError(f"Sequence length {max(lens_l)} exceeds max sequence length {sc.max_sequence_length}")
        dev = kv.per_completion_k_cache.device
        rows_t = torch.tensor(rows_l, dtype=torch.int32, device=dev)
        lens_t = torch.tensor(lens_l, dtype=torch.int32, device=dev)
        for layer in self.model.layers:
            layer.self_attn.kv_cache.promote_unique(rows_t, lens_t, lens_l, use_kernel=use_kernel)
        # the level's token set, with append_shared's discipline: after the level exists, whatever the list held beyond it dropped
        del self.shared_bitmaps[used:]
        ids = token_ids.to(dev).long()
        self.shared_bitmaps.append(layer_ops.token_bitmap(ids, lens_t.to(device=ids.device, dtype=torch.int64), self.vocab_size))
        return self.get_num_used_shared_caches()

    def _fork_merged(self, rows_l, lens_l, token_ids, old_batch: int, use_kernel: bool, base) -> int:
        """fork(merge_from=base): the host checks, one staging allocation, one gather + copy per layer, the merged bitmap."""
        from . import _lib
        from .fork import check_fork_rows

        kv = self.model.layers[0].self_attn.kv_cache
        room = kv.per_completion_k_cache.shape[1]
        used, k = kv.num_used_shared_caches, len(rows_l)
        if isinstance(base, bool) or not isinstance(base, int) or not 0 <= base <= used:
            raise ValueError(f"merge_from {base!r}: an index in [0, {used}] (the levels in use)")
        levels = kv.get_used_shared_caches()
        check_fork_rows(rows_l, old_batch, [c.current_batch_size for c in levels[:base]])
        chain = levels[base:]
        if len(chain) > _lib.HYD_MAX_LEVELS:
            raise ValueError(f"{len(chain)} levels to merge: at most {_lib.HYD_MAX_LEVELS} in one fork")
        for j, c in enumerate(chain):
            if old_batch % c.current_batch_size:
                raise ValueError(f"level {base + j}: {c.current_batch_size} shared sequences do not divide the previous batch of {old_batch}")
        if min(lens_l) < 0 or max(lens_l) > room:
            raise ValueError(f"seq_lens {lens_l}: each at least 0 and at most the {room} tokens a unique sequence caches")
        width = max(max(lens_l), 1)
        if not isinstance(token_ids, Tensor) or token_ids.ndim != 2 or token_ids.shape != (k, width):
            raise ValueError(f"token_ids must be [{k}, {width}] (right-padded to the longest promoted length), got "
                             f"{tuple(token_ids.shape) if isinstance(token_ids, Tensor) else type(token_ids)}")
        if base >= kv.get_num_total_shared_caches():
            raise ValueError(f"No more available shared caches: {used} {kv.get_num_total_shared_caches()}")
        sc = kv.shared_caches[base]
        if k > sc.max_batch_size:
            raise ValueError(f"Batch size {k} exceeds max batch size {sc.max_batch_size}")
        # the chain levels' lengths: one read of the device for all of them
        path = list(lens_l)
        parents = [[r // (old_batch // c.current_batch_size) for r in rows_l] for c in chain]
        if chain:
            host = torch.cat([c.seq_lens[: c.current_batch_size] for c in chain]).tolist()
            at = 0
            for c, par in zip(chain, parents):
                for i, p in enumerate(par):
                    path[i] += int(host[at + p])
                at += c.current_batch_size
        if max(path) > sc.max_sequence_length:
            raise ValueError(f"Sequence length {max(path)} exceeds max sequence length {sc.max_sequence_length}")
        if sum(path) > sc.k_cache.shape[0]:
            raise ValueError(f"{sum(path)} path tokens exceed the {sc.k_cache.shape[0]} tokens level {base} holds")
        dev = kv.per_completion_k_cache.device
        rows_t = torch.tensor(rows_l, dtype=torch.int32, device=dev)
        lens_t = torch.tensor(lens_l, dtype=torch.int32, device=dev)
        # the path's token set first (it reads the chain levels' bitmaps, which the list is about to drop)
        ids = token_ids.to(dev).long()
        bits = torch.zeros((k, (self.vocab_size + 31) // 32), dtype=torch.int32, device=ids.device)
        for j, par in enumerate(parents):
            bits |= self.shared_bitmaps[base + j].to(ids.device)[torch.tensor(par, dtype=torch.int64, device=ids.device)]
        bits = layer_ops.token_bitmap(ids, lens_t.to(device=ids.device, dtype=torch.int64), self.vocab_size, out=bits)
        staging = torch.empty((2, max(sum(path), 1)) + tuple(sc.k_cache.shape[1:]), dtype=sc.k_cache.dtype, device=sc.k_cache.device)
        for layer in self.model.layers:
            layer.self_attn.kv_cache.promote_unique_merged(base, rows_t, lens_t, path, old_batch=old_batch, max_len=max(max(lens_l), 1),
                                                           staging=staging, use_kernel=use_kernel)
        del self.shared_bitmaps[base:]
        self.shared_bitmaps.append(bits)
        return self.get_num_used_shared_caches()

    @torch.no_grad()
    def process_unique(self, input_ids, seq_lens=None):
        """Prefill of per-sequence (unique) prompts (llama.py:1118-1145)."""
        self.set_mode(AttentionMode.UNIQUE_PREFILL)
        return self(input_ids=input_ids, position_ids=self._positions(input_ids), seq_lens=seq_lens)

    # ---- switches of the decode loops (hydragen_amd/generation.py): class attributes, set on a model by tests and tools ------------
    schedule_longest_first = True  # (tests switch it off to compare: only the schedule may depend on it, never a token)
    # top-k / top-p / min-p in the sampling kernel (hyd_sample_tokens_filtered); False: torch cuts + hyd_sample_tokens, the
    # path before the kernel existed (tests switch it off to compare)
    fused_sampling_filters = True
    # penalties in the sampling kernel (hyd_sample_tokens_penalized); False: sampling.penalize_logits in torch, then the paths
    # above (tests and tools/sampler_bench.py switch it off to compare)
    fused_sampling_penalties = True
    # hyd_stop_update path: every this many decode steps the host starts a non-blocking copy of the running-row count of the
    # step just enqueued and looks at it one step later (tests shrink it)
    stop_poll_steps = 8
    # None: finished rows are retired from the unique K/V stream whenever the fused decode preamble is in use; False: never
    # (tools/stop_bench.py and the tests compare the two: only the step time may depend on it, never a token)
    stop_retire: Optional[bool] = None

    # ---- generation -----------------------------------------------------------------------------------
    # Contract (README.md:183-289 of the reference; llama.py:1156-1396): prompts form a hierarchy, outermost level
    # first.  With num_return_sequences > 1 every given level is shared and the completions hang off the last one;
    # otherwise the last given level is each sequence's own (unique) prompt.  shared_cache_op: "wipe" empties the
    # shared caches first, "preserve" drops the levels this call added when it returns, "extend" keeps them.
    def _prompt_levels(self, input_ids, seq_lens, fan_out, flatten_last):
        """-> (shared levels [(ids, lens)], unique level (ids, lens) or None)."""
        levels = [] if input_ids is None else ([input_ids] if isinstance(input_ids, Tensor) else list(input_ids))
        if seq_lens is None:
            lens = [torch.full((x.shape[0],), x.shape[1], device=x.device, dtype=torch.long) for x in levels]
        else:
            lens = [seq_lens] if isinstance(seq_lens, Tensor) else list(seq_lens)
        pairs = list(zip(levels, lens))
        if not pairs or (fan_out and not flatten_last):
            return pairs, None
        return pairs[:-1], pairs[-1]

    def _check_room(self, start_positions, new_tokens, extra=0):
        """The fused decode preamble cannot raise from the device: refuse on the host anything that would index past
        the unique cache or the rotary tables (the reference's scatter_/index ops device-assert).  extra: the K
        draft tokens a speculative step feeds behind a row's last token -- K more cache rows and positions."""
        if new_tokens < 2:
            return  # the first token comes from the prefill logits: no decode step runs
        new_tokens += extra
        room = self.model.layers[0].self_attn.kv_cache.per_completion_k_cache.shape[1]
        last_pos = int(start_positions.max().item()) + new_tokens - 2
        # cache index = position - shared length, PER SEQUENCE (llama.py:487-492 of the reference): with ragged shared
        # levels the longest position and the shortest shared length belong to different sequences
        starts = start_positions.reshape(start_positions.shape[0], -1)[:, 0]
        if self.model.get_disable_hydragen():
            first_idx = starts
        else:
            first_idx = starts - self.get_shared_cache_len(start_positions.shape[0]).to(starts.device)
        last_idx = int(first_idx.max().item()) + new_tokens - 2
        if last_idx >= room:
            raise ValueError(f"unique cache holds {room} tokens per sequence, decoding needs {last_idx + 1}")
        if last_pos >= self.config.max_position_embeddings:
            raise ValueError(f"position {last_pos} exceeds max_position_embeddings = {self.config.max_position_embeddings}")

    @torch.no_grad()
    def generate(self, input_ids: Optional[Union[Tensor, list[Tensor]]] = None,
                 seq_lens: Optional[Union[Tensor, list[Tensor]]] = None, starting_logits: Optional[Tensor] = None,
                 num_return_sequences: int = 1, max_new_tokens: int = 5, temperature: float = 1.0,
                 top_p: Optional[float] = None, eos_token_id: Optional[Union[int, list, tuple]] = None, return_logits: bool = False,
                 shared_cache_op: str = SharedCacheOp.PRESERVE, disable_hydragen: bool = False,
                 disable_attention: bool = False, disable_hierarchy: bool = False,
                 token_overrides: Optional[Tensor] = None, top_k: Optional[int] = None, min_p: Optional[float] = None,
                 return_logprobs: bool = False, top_logprobs: int = 0, repetition_penalty: Optional[float] = None,
                 presence_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None, logit_bias=None,
                 stop=None, pad_token_id: Optional[int] = None, include_stop: bool = False, return_finish: bool = False,
                 constraint=None, constraint_state: Optional[Tensor] = None, return_constraint_state: bool = False,
                 draft_tokens: Optional[int] = None, draft="prompt_lookup", ngram=(1, 3), return_draft_stats: bool = False,
                 seed=None):
        """Prompts and caches: input_ids is one level or a list of levels, outermost first, seq_lens their lengths (right padding;
        the contract above _prompt_levels); starting_logits instead of input_ids continues from levels kept by an earlier call.
        shared_cache_op: "wipe" / "preserve" / "extend".  disable_hydragen / disable_hierarchy / disable_attention are the
        reference's baselines.  The decode half -- argument checks, first draw, step loops -- is hydragen_amd/generation.py.

        Sampling: top_k / top_p / min_p cut the UNSCALED softmax(logits) (the reference's top-p order; HF applies the
        temperature first), then a token is drawn from softmax(logits / temperature) over the kept tokens.
        Penalties (hydragen_amd/sampling.py states the rules; None = off): repetition_penalty r > 0 (HF / vLLM: l / r if l > 0
        else l * r for every token of the row's context -- all shared levels on its path, levels kept by earlier calls included,
        and its own prompt -- or of its generated tokens), frequency_penalty / presence_penalty (OpenAI / vLLM: generated
        tokens only), logit_bias {token id: bias} or (ids, values), -inf bans a token.  "Generated" is what was fed back: the
        sampled tokens, or token_overrides where given.  Cuts, draw and return_logprobs then act on the PENALISED logits
        (log softmax of the penalised, unscaled, unfiltered logits: the distribution the draw's policy is defined by);
        return_logits and top_logprobs keep reporting the model's raw distribution.  With every penalty off, generate()
        runs exactly the launches it runs without these arguments.
        Constrained decoding (hydragen_amd/sampling.py states the rules, hydragen_amd/constraint.py builds the automata):
        constraint = a constraint.TokenDFA over the model's vocabulary restricts what every row may emit by what it has emitted
        so far; constraint_state = the rows' start states, int [leaf batch] (repeated for num_return_sequences) or [batch],
        default 0; a state outside the automaton leaves a row unconstrained.  The states live on the device for the whole call
        and advance with every draw, the one from the prefill logits included: no host synchronisation, and no [B, V] mask
        wherever sampling.sample_route's table routes a draw to hyd_sample_tokens_constrained (every draw of one sample per
        row).  It composes with the cuts, the penalties and the stop conditions: with TokenDFA.from_choices /
        from_regex(eos=ids) and eos_token_id=ids a row ends through the stop kernel once its output is
        complete.  return_logprobs reports the CONSTRAINED distribution (the same rule as for penalties); return_logits and
        top_logprobs stay raw.  Not with token_overrides.  With constraint=None, generate() runs exactly the launches it runs
        without these arguments.

        Per row (hyd_sample_tokens_rows, hyd_stop_update_rows; requests of different settings batched behind one shared
        prompt): temperature, top_k, top_p, min_p, repetition_penalty, presence_penalty and frequency_penalty may each be a list
        or 1-d tensor instead of a scalar, with one entry per prompt of the innermost level (repeated for num_return_sequences)
        or one per row of the batch -- constraint_state's rule; None inside a list switches the value off for that row (not for
        temperature).  The values are checked on the host, uploaded once and stay on the device for the call; every draw, the
        first one with its fan-out included, is then ONE launch in which each row samples with its own values, bit for bit what
        a call with that row's values in every row would give that row.  seed = one integer per row (same shape rule): the draw
        of output position t uses the row's seed and offset t, torch's generator is not advanced, and a row's tokens depend
        neither on its place in the batch nor on what torch drew earlier (on a CPU model the seeded draws come from torch
        generators of their own: the same property, other tokens than on the GPU).  max_new_tokens as a list or tensor gives
        every row a limit of its own (>= 1): the device-side stop path runs with it, a row that reaches its limit finishes
        with reason 3 and is padded, fed pad and retired like a row that met an EOS id, the result is [B, max(lengths)], and the
        penalties' list of generated tokens is sized by the largest limit.  A call that passes only scalars runs exactly the
        launches it ran without these forms.  Refused (before any launch): any of them with draft_tokens or token_overrides.

        Stopping, decided on the device (hyd_stop_update; hydragen_amd/stopping.py states the rules): eos_token_id given as a
        LIST or tuple of ids (a list of one included), stop = a list of token-id sequences (lists, tuples or 1-d tensors, ragged; up
        to 32 of 1..16 tokens), pad_token_id (default: the first EOS id if any, else 0) or return_finish select this path; an int
        eos_token_id alone keeps the loop and the result it always had.  No tokenizer is involved: stop sequences match TOKEN ids,
        which is not string matching across tokenisation boundaries (a stop string the tokenizer merges with its neighbours in
        context is not found: pass every tokenisation that should stop).  A row finishes at its first EOS id (kept) or stop sequence
        (cut unless include_stop); from then on its columns hold pad_token_id, it is fed pad, and -- with the fused decode preamble
        -- it leaves the unique K/V stream: no K/V is appended for it and the suffix pass sees length 0 (what that gives back of
        a step is measured in profiles/stopping.md).  The host does not look at a token per step:
        it polls the count of running rows every stop_poll_steps steps and leaves the loop when that is 0.  The returned matrix is
        [B, max(lengths)], whenever the exit was noticed.  With return_logprobs, entries at or past a row's length are 0.0; with
        top_logprobs, id -1 / -inf; the return_logits rows of a finished sequence past its length are unspecified.  Penalties keep
        working (what a finished row draws is ignored).  token_overrides cannot be combined with these arguments.

        Drafts (hydragen_amd/speculative.py states the scheme and why it is lossless): draft_tokens = K in 1..7
        makes every decode step feed each row its last token and K drafts, verify them in ONE forward pass over [B, K + 1] (the
        multi-token RoPE + append, the causal-tail attention) and keep the draws up to the first wrong draft; None or 0 runs
        exactly the launches generate() runs without it.  draft = "prompt_lookup": drafts are the tokens that followed the latest
        earlier occurrence of the row's last n-gram (ngram = (min, max) lengths, longest first) in the prompt levels GIVEN TO THIS
        CALL on the row's path, its own prompt and its generated tokens (hyd_draft_lookup; levels kept by earlier calls with
        shared_cache_op="extend" are not searched -- their ids are not given to this call); or an int tensor [B, max_new_tokens]
        whose column p is the draft for output position p (tests, benchmarks; no lookup launch).  Rows advance by different
        amounts; EOS ids and max_new_tokens are applied on the device (hyd_draft_accept) and the result is [B, max(lengths)] padded
        with pad_token_id, as on the stop path (an int eos_token_id is treated as a list of one).  Works with temperature, top_k /
        top_p / min_p, return_logprobs, eos_token_id, pad_token_id, return_finish, num_return_sequences, seq_lens, shared_cache_op
        and constraint, and with stop / include_stop and the penalties / logit_bias.  stop: the accept (hyd_draft_accept_stop) judges EVERY
        token a row emits in the step, in order, against the row's output so far -- a sequence may complete at any of them and
        may have begun in an earlier step --, so tokens, lengths and finish reasons are those of one-token decoding with the same
        stop.  Penalties and logit_bias: the draw behind the i-th fed token counts the drafts fed in
        front of it as already generated (hyd_sample_tokens_penalized_drafts), which keeps the scheme lossless; the sampler never
        appends there, the accept keeps the lists of generated tokens.  Refused (before any launch): penalties, logit_bias
        or stop together with constraint=, token_overrides, top_logprobs, return_logits, per-row values / seeds / limits,
        disable_hydragen / disable_attention / disable_hierarchy, narrow unique caches, a model on the CPU.  fp8 unique caches
        (setup_caches(kv_cache_dtype=torch.float8_e4m3fn), with or without kv_scales="calibrate") work: the preamble quantizes
        the T new rows and the causal-tail pass is the fp8 matrix-core kernel (head dim 256 with few units, which it does not
        take, runs the assembled attention on dequantized rows: functional, not fast).
        With constraint= every step walks its drafts through the automaton (hyd_draft_constrain): a state that allows exactly
        one token replaces the draft by that token -- accepted with probability 1, the masked sampler can draw nothing else --,
        a draft the automaton rejects ends the row's proposal, each of the step's K + 1 draws is masked by the state behind the
        tokens fed in front of it, and the accept (hyd_draft_accept_states) hands the row the state behind its last emitted
        token.  draft = "constraint" (needs constraint=) proposes that forced chain and nothing else: no lookup launch.

        Returns the tokens [B, generated] alone, or a tuple in this order, each part only if asked for: (tokens, the per-step
        fp32 logits (return_logits), the fp32 [B, generated] log softmax(logits) of every returned token, unscaled and unfiltered
        (return_logprobs), top_ids [B, generated, N] int64 and top_logprobs [B, generated, N] f32: for every returned token the N
        best alternatives of that step's distribution (top_logprobs = N > 0, needs return_logprobs; hyd_token_logprobs,
        hydragen_amd/scoring.py), a stopping.Finish(lengths, reasons, stop_index) (return_finish; int32 [B] each; reason 0 = ran
        to max_new_tokens, 1 = EOS, 2 = stop sequence, 3 = the row's own limit), the final int32 [B] automaton states (return_constraint_state), a
        speculative.DraftStats(steps, proposed, accepted) whose .forced holds, per row, the proposed drafts that were forced
        under a constraint (return_draft_stats))."""
        if not self.kv_cache_allocated:
            raise RuntimeError("call setup_caches() before generate()")
        call = generation.check_arguments(
            self, input_ids=input_ids, starting_logits=starting_logits, num_return_sequences=num_return_sequences,
            max_new_tokens=max_new_tokens, temperature=temperature, top_p=top_p, top_k=top_k, min_p=min_p, eos_token_id=eos_token_id,
            return_logits=return_logits, disable_hydragen=disable_hydragen, disable_attention=disable_attention,
            disable_hierarchy=disable_hierarchy, token_overrides=token_overrides, return_logprobs=return_logprobs,
            top_logprobs=top_logprobs, repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
            frequency_penalty=frequency_penalty, logit_bias=logit_bias, stop=stop, pad_token_id=pad_token_id, include_stop=include_stop,
            return_finish=return_finish, constraint=constraint, constraint_state=constraint_state,
            return_constraint_state=return_constraint_state, draft_tokens=draft_tokens, draft=draft, ngram=ngram,
            return_draft_stats=return_draft_stats, seed=seed)
        fan_out = num_return_sequences > 1
        flatten = disable_hierarchy or disable_hydragen  # the baselines keep the last level per sequence
        if shared_cache_op == SharedCacheOp.WIPE:
            self.empty_shared_cache()
        levels_before = self.get_num_used_shared_caches()
        shared, unique = self._prompt_levels(input_ids, seq_lens, fan_out, flatten)
        n_given = len(shared) + (unique is not None)
        depth = levels_before + n_given + (1 if fan_out else 0)
        if disable_hydragen and (depth != 2 or (n_given == 2 and shared[0][0].shape[0] != 1)):
            raise ValueError("disable_hydragen compares against ONE shared prompt: exactly two levels, the first of batch 1")
        if disable_hierarchy and not (depth == 3 and fan_out):
            raise ValueError("disable_hierarchy flattens a three-level hierarchy with num_return_sequences > 1")

        self.model.set_disable_attention(bool(disable_attention))
        self._scale_windows("open_scale_window")  # calibrated fp8 scales: they may move until this call first writes the unique cache
        logits = None if starting_logits is None else starting_logits.unsqueeze(1)
        for ids, lens in shared:
            logits = self.append_shared(ids, lens)
        leaf_batch = (unique[0].shape[0] if unique is not None else logits.shape[0])
        batch = leaf_batch * num_return_sequences
        if disable_hydragen:
            self.model.set_disable_hydragen(True)
            if self.get_num_used_shared_caches() > 0:
                self.model.copy_shared_cache_to_unique(batch)
        if unique is not None:
            logits = self.process_unique(*unique)
            self.repeat_per_completion_cache_for_num_samples(unique[0].shape[0], num_return_sequences)

        try:
            return generation.decode(self, call, logits[:, -1], shared, unique)
        finally:
            self._scale_windows("close_scale_window", write=False)  # (a call that raised before its first write)
            if shared_cache_op == SharedCacheOp.PRESERVE:
                self.truncate_shared_caches(levels_before)
            self.model.set_disable_hydragen(False)
            self.model.set_disable_attention(False)

    @torch.no_grad()
    def choose(self, input_ids, choices, eos_token_id: int, seq_lens=None, temperature: float = 0.0, **kw):
        """Multiple choice under shared prompts (the lm-eval-style call): every row answers with one of `choices` (token-id
        sequences; a list of lists of them gives row b of the leaf batch its own set, choices[b]) followed by eos_token_id.
        A thin wrapper over generate(constraint=TokenDFA.from_choices(...), eos_token_id=[eos_token_id]); kw goes to generate.
        Returns (choice index int64 [B] -- within the row's set, -1: not finished --, tokens [B, generated])."""
        from .constraint import TokenDFA

        dfa = TokenDFA.from_choices(choices, self.vocab_size, eos=[int(eos_token_id)], on_accept="eos")
        groups = dfa.meta["groups"]
        start = torch.tensor(dfa.start_states, dtype=torch.int32) if len(groups) > 1 else None
        longest = max(len(c) for g in groups for c in g) + 1
        out = self.generate(input_ids, seq_lens=seq_lens, max_new_tokens=longest, temperature=temperature,
                            eos_token_id=[int(eos_token_id)], constraint=dfa, constraint_state=start, return_constraint_state=True, **kw)
        return dfa.choice_of(out[-1]), out[0]

    # ---- scoring ----------------------------------------------------------------------------------------
    score_chunk_bytes = 1 << 30  # lm_head output per chunk of score()'s scored rows (tests shrink it)
    score_gemm_rows = 256        # rows per lm_head GEMM in score(): chunks are multiples of it

    @torch.no_grad()
    def score(self, input_ids: Union[Tensor, list[Tensor]], target_lens: Union[Tensor, list[int]],
              seq_lens: Optional[Union[Tensor, list[Tensor]]] = None, top_logprobs: int = 0,
              shared_cache_op: str = SharedCacheOp.PRESERVE, disable_hydragen: bool = False) -> scoring.ScoreResult:
        """Log-likelihood of given continuations (lm-eval `loglikelihood`, multiple choice, reranking).  input_ids / seq_lens follow
        generate()'s level contract with num_return_sequences == 1: every level but the last is shared (append_shared), the last
        [B, Lu] (right-padded) is each sequence's own.  The last target_lens[b] real tokens of sequence b's own level are scored,
        each under the distribution that precedes it; when target_lens[b] == its length, the first target's distribution is
        the innermost shared level's last-position logits (shared row b // (B / sb)), so that level must be given in this call.
        The decoder stack runs once over the unique level; lm_head and hyd_token_logprobs run on chunks of the scored rows
        (score_chunk_bytes of logits each), never on [B, Lu, V].  shared_cache_op and disable_hydragen act as in generate().
        The unique cache is overwritten; a captured decode graph is neither used nor invalidated.  Every argument and
        capacity is checked on the host before the first launch."""
        if not self.kv_cache_allocated:
            raise RuntimeError("call setup_caches() before score()")
        top_n = scoring.check_top_n(top_logprobs)
        shared, unique = self._prompt_levels(input_ids, seq_lens, False, True)
        if unique is None:
            raise ValueError("score() needs at least one prompt level: the last one holds the scored tokens")
        uids, ulens = unique
        B, Lu = uids.shape
        ul = [int(x) for x in ulens.reshape(-1).tolist()]
        tl = [int(x) for x in torch.as_tensor(target_lens).reshape(-1).tolist()]
        if len(tl) != B or len(ul) != B:
            raise ValueError(f"target_lens has {len(tl)} entries and seq_lens {len(ul)} for a batch of {B}")
        bad = [b for b in range(B) if not 1 <= tl[b] <= ul[b] or ul[b] > Lu]
        if bad:
            b = bad[0]
            raise ValueError(f"sequence {b}: target_lens {tl[b]} must be in [1, {ul[b]}] (its unique length, <= {Lu})")
        levels_before = 0 if shared_cache_op == SharedCacheOp.WIPE else self.get_num_used_shared_caches()
        depth = levels_before + len(shared) + 1
        if disable_hydragen and (depth != 2 or (shared and shared[0][0].shape[0] != 1)):
            raise ValueError("disable_hydragen compares against ONE shared prompt: exactly two levels, the first of batch 1")
        if any(t == u for t, u in zip(tl, ul)):
            if depth == 1:
                raise ValueError("target_lens == the unique length scores the first token with no context: give a shared level")
            if not shared:
                raise ValueError("target_lens == the unique length needs the innermost shared level's logits: pass that level in "
                                 "this call")
        kv = self.model.layers[0].self_attn.kv_cache
        if levels_before + len(shared) > kv.get_num_total_shared_caches():
            raise ValueError(f"{levels_before + len(shared)} shared levels, the caches hold {kv.get_num_total_shared_caches()}")
        shared_len = torch.zeros(B, dtype=torch.long)
        if levels_before:
            shared_len += self.get_shared_cache_len(B).cpu()
        for i, (ids, lens) in enumerate(shared):
            sc = kv.shared_caches[levels_before + i]
            if B % ids.shape[0] or ids.shape[0] > sc.max_batch_size or ids.shape[1] > sc.max_sequence_length:
                raise ValueError(f"shared level {levels_before + i}: [{ids.shape[0]}, {ids.shape[1]}] against a batch of {B} and a "
                                 f"cache of [{sc.max_batch_size}, {sc.max_sequence_length}]")
            shared_len += lens.reshape(-1).cpu().long().repeat_interleave(B // ids.shape[0])
        rows, room = kv.per_completion_k_cache.shape[:2]
        if B > rows:
            raise ValueError(f"batch {B} exceeds the unique cache's {rows} sequences")
        need = Lu + (int(shared_len.max()) if disable_hydragen else 0)
        if need > room:
            raise ValueError(f"unique cache holds {room} tokens per sequence, scoring needs {need}")
        last_pos = int((shared_len + Lu - 1).max())
        if last_pos >= self.config.max_position_embeddings:
            raise ValueError(f"position {last_pos} exceeds max_position_embeddings = {self.config.max_position_embeddings}")

        if shared_cache_op == SharedCacheOp.WIPE:
            self.empty_shared_cache()
        levels_before = self.get_num_used_shared_caches()
        self.model.set_disable_attention(False)
        self._scale_windows("open_scale_window")
        try:
            shared_logits = None
            for ids, lens in shared:
                shared_logits = self.append_shared(ids, lens)
            if disable_hydragen:
                self.model.set_disable_hydragen(True)
                if self.get_num_used_shared_caches() > 0:
                    self.model.copy_shared_cache_to_unique(B)
            self.set_mode(AttentionMode.UNIQUE_PREFILL)
            hidden = self.model(input_ids=uids, position_ids=self._positions(uids))
            return self._score_rows(hidden, shared_logits, uids, tl, ul, top_n)
        finally:
            self._scale_windows("close_scale_window", write=False)
            if shared_cache_op == SharedCacheOp.PRESERVE:
                self.truncate_shared_caches(levels_before)
            self.model.set_disable_hydragen(False)

    def _score_rows(self, hidden, shared_logits, uids, tl, ul, top_n):
        """Log-probs of the targets from the unique level's hidden states [B, Lu, H] (target at unique position p >= 1: the
        hidden state at p - 1) and the innermost shared level's last-position logits [sb, 1, V] (p == 0)."""
        B, Lu = uids.shape
        dev = uids.device
        T = max(tl)
        tl_t, ul_t = torch.tensor(tl, device=dev), torch.tensor(ul, device=dev)
        j = torch.arange(T, device=dev)
        pos = ul_t[:, None] - tl_t[:, None] + j[None, :]  # unique position of every target
        live = j[None, :] < tl_t[:, None]
        tgt = uids.long().gather(1, pos.clamp(0, Lu - 1))
        lp = torch.full((B, T), float("nan"), dtype=torch.float32, device=dev)
        greedy = torch.zeros((B, T), dtype=torch.bool, device=dev)
        top_ids = torch.full((B, T, top_n), -1, dtype=torch.int64, device=dev)
        top_lp = torch.full((B, T, top_n), float("-inf"), dtype=torch.float32, device=dev)
        V = self.lm_head.weight.shape[0]
        fp8_head = isinstance(self.lm_head, Fp8Linear)  # quantize_weights(skip=()): the module's own routes, block by block

        G = self.score_gemm_rows

        def run(bi, ji, logits_of, esz):
            per = max(G, self.score_chunk_bytes // (V * esz) // G * G)
            for s in range(0, bi.numel(), per):
                b, jj = bi[s : s + per], ji[s : s + per]
                o = layer_ops.token_logprobs(logits_of(b, jj), tgt[b, jj], top_n)
                lp[b, jj], greedy[b, jj] = o[0], o[1]
                if top_n:
                    top_ids[b, jj], top_lp[b, jj] = o[2], o[3]

        hb, hj = (live & (pos >= 1)).nonzero(as_tuple=True)
        def head(b, jj):
            # the 16-bit lm_head output goes straight into the kernel.  The GEMM always sees blocks of G rows (the last one
            # zero-padded): a row's logits come from the same GEMM shape whatever the chunk size and the batch
            h = hidden[b, pos[b, jj] - 1]
            r = h.shape[0]
            h = torch.cat([h, h.new_zeros(((-r) % G, h.shape[1]))]) if r % G else h
            out = h.new_empty((h.shape[0], V))
            for k in range(0, h.shape[0], G):
                if fp8_head:
                    out[k : k + G] = self.lm_head(h[k : k + G])
                else:
                    torch.mm(h[k : k + G], self.lm_head.weight.t(), out=out[k : k + G])
            return out[:r]

        run(hb, hj, head, hidden.element_size() if fp8_head else self.lm_head.weight.element_size())
        sb_, sj = (live & (pos == 0)).nonzero(as_tuple=True)
        if sb_.numel():
            sh = shared_logits[:, -1]
            rep = B // sh.shape[0]
            run(sb_, sj, lambda b, jj: sh[b // rep], sh.element_size())
        return scoring.ScoreResult(
            logprobs=lp, token_greedy=greedy, sum=torch.where(live, lp.double(), torch.zeros_like(lp, dtype=torch.float64)).sum(1),
            is_greedy=(greedy | ~live).all(1), top_ids=top_ids if top_n else None, top_logprobs=top_lp if top_n else None)
