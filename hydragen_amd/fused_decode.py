"""Python face of `hyd_rope_append_decode` (include/hydragen_hip.h): the fused RoPE + unique-KV append +
seq_lens kernel of the decode step (replaces /root/reference/hydragen/llama.py:236-262,485-501,565-569)."""

from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _lib
from ._lib import RopeParams
from .flash import _dtype_code, _require_gpu, _stream, check_kv_pair, kv_quant_params, padded_head_dim


class QkNorm(C.Structure):
    """hyd_qk_norm: the per-head q/k RMSNorm block of the _qkn entry points."""
    _fields_ = [("q_weight", C.c_void_p), ("k_weight", C.c_void_p), ("eps", C.c_float), ("flags", C.c_int32)]


def qk_norm_params(q, D: int, q_norm: Tensor | None, k_norm: Tensor | None, norm_eps: float | None):
    """None without gains, else the QkNorm of two gain vectors [D] of q's dtype (both or neither; norm_eps is required)."""
    if q_norm is None and k_norm is None:
        if norm_eps is not None:
            raise ValueError("norm_eps without q_norm / k_norm")
        return None
    if q_norm is None or k_norm is None:
        raise ValueError("q_norm and k_norm come together: both gain vectors, or neither")
    if norm_eps is None:
        raise ValueError("q_norm / k_norm need norm_eps")
    for w in (q_norm, k_norm):
        _require_gpu(w)
        if w.shape != (D,) or w.dtype != q.dtype or not w.is_contiguous():
            raise ValueError(f"q_norm / k_norm: contiguous [{D}] gains of {q.dtype}, got {tuple(w.shape)} {w.dtype}")
    return QkNorm(q_norm.data_ptr(), k_norm.data_ptr(), float(norm_eps), 0)


def rope_append_multi(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, position_ids: Tensor,
                      shared_len: Tensor | None, k_cache: Tensor, v_cache: Tensor, q_norm: Tensor | None = None,
                      k_norm: Tensor | None = None, norm_eps: float | None = None, *, k_scale: Tensor | None = None,
                      v_scale: Tensor | None = None):
    """hyd_rope_append_multi: the preamble of a MULTI-TOKEN decode step (speculative.py).  q [B,T,Hq,D], k/v [B,T,Hkv,D] with
    2 <= T <= 8, position_ids int64 [B] or [B, T] (column 0 is read: the first token's absolute position, token i uses + i),
    shared_len int64 [B] or None, caches [maxB, maxS, Hkv, D] with D 64 / 128 / 256.  Returns (rotated q [B,T,Hq,D],
    seq_lens int32 [B] = cache index of the first token + T); K (rotated) and V of token i are written at that index + i.  A
    row at position shared_len - 1 writes nothing and reports length 0.  q_norm / k_norm [D] of q's dtype with norm_eps: the
    per-head RMSNorm of q and k in front of the rotation (hyd_rope_append_multi_qkn), as in rope_append_decode.
    float8_e4m3fn caches (hyd_rope_append_multi_kvq) receive quantize_kv(k_rot, k_scale) / quantize_kv(v, v_scale) as in
    rope_append_decode: the bytes T one-token calls at positions + i would leave."""
    _require_gpu(q, k, v, cos, sin, position_ids, k_cache, v_cache)
    fp8 = check_kv_pair(k_cache, v_cache, k_scale, v_scale)
    B, T, Hq, D = q.shape
    if D not in (64, 128, 256) or k_cache.shape[-1] != D:
        raise NotImplementedError(f"head_dim {D} (caches {k_cache.shape[-1]}): the multi-token preamble takes 64 / 128 / 256")
    Hkv = k.shape[2]
    assert k.shape == (B, T, Hkv, D) and v.shape == k.shape and B <= k_cache.shape[0]
    for x in (q, k, v):
        assert x.stride(3) == 1 and x.stride(2) == D, "heads contiguous"
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.stride(1) == 1
    assert position_ids.dtype == torch.int64 and position_ids.shape[0] == B
    q_out = torch.empty((B, T, Hq, D), dtype=q.dtype, device=q.device)
    seq_lens = torch.empty((B,), dtype=torch.int32, device=q.device)
    p = _lib.RopeMultiParams()
    p.q, p.k, p.v, p.q_out = q.data_ptr(), k.data_ptr(), v.data_ptr(), q_out.data_ptr()
    p.k_cache, p.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    p.cos, p.sin = cos.data_ptr(), sin.data_ptr()
    p.position_ids = position_ids.data_ptr()
    if shared_len is not None:
        assert shared_len.dtype == torch.int64 and shared_len.shape == (B,)
        shared_len = shared_len.contiguous()
        p.shared_len = shared_len.data_ptr()
    p.seq_lens = seq_lens.data_ptr()
    p.q_batch_stride, p.k_batch_stride, p.v_batch_stride = q.stride(0), k.stride(0), v.stride(0)
    p.q_tok_stride, p.k_tok_stride, p.v_tok_stride = q.stride(1), k.stride(1), v.stride(1)
    p.kc_batch_stride, p.kc_tok_stride, p.kc_head_stride = k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)
    p.vc_batch_stride, p.vc_tok_stride, p.vc_head_stride = v_cache.stride(0), v_cache.stride(1), v_cache.stride(2)
    p.pos_stride, p.cs_stride = position_ids.stride(0), cos.stride(0)
    p.dtype, p.B, p.T, p.Hq, p.Hkv, p.D, p.cache_len = _dtype_code(q), B, T, Hq, Hkv, D, k_cache.shape[1]
    p.max_pos = cos.shape[0]
    qn = qk_norm_params(q, D, q_norm, k_norm, norm_eps)
    if fp8:
        kq = kv_quant_params(k_scale, v_scale)
        _lib.check(_lib.load().hyd_rope_append_multi_kvq(C.byref(p), C.byref(kq), None if qn is None else C.byref(qn), _stream()))
    elif qn is not None:
        _lib.check(_lib.load().hyd_rope_append_multi_qkn(C.byref(p), C.byref(qn), _stream()))
    else:
        _lib.check(_lib.load().hyd_rope_append_multi(C.byref(p), _stream()))
    return q_out, seq_lens


def rope_append_decode(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, position_ids: Tensor,
                       shared_len: Tensor | None, k_cache: Tensor, v_cache: Tensor, *, k_scale: Tensor | None = None,
                       v_scale: Tensor | None = None, q_norm: Tensor | None = None, k_norm: Tensor | None = None,
                       norm_eps: float | None = None):
    """q [B,1,Hq,D], k/v [B,1,Hkv,D] (this step's projections), cos/sin fp32 [max_pos, D],
    position_ids int64 [B,1] absolute, shared_len int64 [B] or None, caches [maxB, maxS, Hkv, D].
    Returns (rotated q [B,1,Hq,D], seq_lens int32 [B]); k (rotated) and v are written into the caches
    at index position - shared_len.  float8_e4m3fn caches receive quantize_kv(k_rot, k_scale) and
    quantize_kv(v, v_scale) (kv_quant.py), k_rot being the 16-bit rotated k a 16-bit cache would hold.
    Narrow head dims (d % 16 == 0, not 64 / 128 / 256; 16-bit caches): q / k / v, the cos / sin tables and the caches are d wide,
    the returned q is padded_head_dim(d) wide with zero pad columns -- what the attention operators take beside narrow unique
    caches (hyd_rope_params.head_dim).
    q_norm / k_norm [D] of q's dtype with norm_eps (both gains or neither): every q head and every k head is RMS-normalised with
    its gain vector in front of the rotation, in fp32 with one rounding at the end (hyd_rope_append_decode_qkn); 16-bit and fp8
    caches, head dims 64 / 128 / 256 only."""
    _require_gpu(q, k, v, cos, sin, position_ids, k_cache, v_cache)
    fp8 = check_kv_pair(k_cache, v_cache, k_scale, v_scale)
    lib = _lib.load()
    B, one, Hq, D = q.shape
    head_dim = 0
    if D not in (64, 128, 256):  # narrow rows in, the kernels' head dim out
        if fp8 or D % 16 or k_cache.shape[-1] != D or v_cache.shape[-1] != D:
            raise NotImplementedError(f"head_dim {D}: the fused preamble takes 64 / 128 / 256, or a multiple of 16 below 256 with "
                                      "16-bit caches of that width")
        head_dim, D = D, padded_head_dim(D)
    assert one == 1 and k.shape[:2] == (B, 1) and v.shape == k.shape
    dq = head_dim or D
    assert q.stride(3) == 1 and q.stride(2) == dq and k.stride(3) == 1 and k.stride(2) == dq and v.stride(2) == dq
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.stride(1) == 1
    assert position_ids.dtype == torch.int64 and position_ids.shape[0] == B
    assert B <= k_cache.shape[0]
    Hkv = k.shape[2]
    q_out = torch.empty((B, 1, Hq, D), dtype=q.dtype, device=q.device)
    seq_lens = torch.empty((B,), dtype=torch.int32, device=q.device)
    p = RopeParams()
    p.q, p.k, p.v, p.q_out = q.data_ptr(), k.data_ptr(), v.data_ptr(), q_out.data_ptr()
    p.k_cache, p.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    p.cos, p.sin = cos.data_ptr(), sin.data_ptr()
    p.position_ids = position_ids.data_ptr()
    if shared_len is not None:
        assert shared_len.dtype == torch.int64 and shared_len.shape == (B,)
        shared_len = shared_len.contiguous()
        p.shared_len = shared_len.data_ptr()
    p.seq_lens = seq_lens.data_ptr()
    p.q_batch_stride, p.k_batch_stride, p.v_batch_stride = q.stride(0), k.stride(0), v.stride(0)
    p.kc_batch_stride, p.kc_tok_stride, p.kc_head_stride = k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)
    p.vc_batch_stride, p.vc_tok_stride, p.vc_head_stride = v_cache.stride(0), v_cache.stride(1), v_cache.stride(2)
    p.pos_stride, p.cs_stride = position_ids.stride(0), cos.stride(0)
    p.dtype, p.B, p.Hq, p.Hkv, p.D, p.cache_len = _dtype_code(q), B, Hq, Hkv, D, k_cache.shape[1]
    p.max_pos = cos.shape[0]
    p.head_dim = head_dim
    qn = qk_norm_params(q, q.shape[-1], q_norm, k_norm, norm_eps)
    if qn is not None:
        if head_dim:
            raise NotImplementedError(f"q_norm / k_norm with head_dim {head_dim}: the per-head norm takes head dims 64 / 128 / 256")
        kq = kv_quant_params(k_scale, v_scale) if fp8 else None
        _lib.check(lib.hyd_rope_append_decode_qkn(C.byref(p), None if kq is None else C.byref(kq), C.byref(qn), _stream()))
    elif fp8:
        kq = kv_quant_params(k_scale, v_scale)
        _lib.check(lib.hyd_rope_append_decode_kvq(C.byref(p), C.byref(kq), _stream()))
    else:
        _lib.check(lib.hyd_rope_append_decode(C.byref(p), _stream()))
    return q_out, seq_lens
