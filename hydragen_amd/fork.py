"""
Fork completions: promote rows of the unique K/V caches to a new shared level (`hyd_kv_promote`, include/hydragen_hip.h).

A batch of completions has run for some tokens, a few of them are worth continuing, and each is to be sampled from several
times (step-level beam search, best-of-N with a step scorer, tree-of-thought, self-consistency with pruning).  The rotated K/V
of the chosen completions already sit in the unique caches: `promote_kv` gathers them into a packed shared level -- one launch per
layer, no forward pass -- and `HydragenLlamaForCausalLM.fork` makes that level the next one of the hierarchy.

    promote_kv / promote_kv_reference   the copy (HIP kernel / its definition in torch)
    gather_paths / gather_paths_reference   a survivor's whole path -- its parents' sequences in a chain of levels, then its
                                        unique rows -- into ONE packed level (`hyd_kv_gather_paths`): fork(merge_from=)
    check_fork_rows                     the host rule that keeps the hierarchy regular
    select_beams                        the `width` best rows per group, in the order check_fork_rows asks for
    stepwise_beam_search                a small driver: generate -> select_beams -> fork -> generate ...
"""

from __future__ import annotations

import ctypes as C
from typing import Callable, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from .kv_quant import FP8_DTYPE, dequantize_kv, is_fp8

_DST_DIMS = (64, 128, 256)


def _check_promote(k_src, v_src, rows, lens, k_dst, v_dst, k_scale, v_scale):
    """Shapes and dtypes both routes refuse.  -> (B, src_rows, Hkv, d_src, d_dst, n)."""
    if k_src.ndim != 4 or k_src.shape != v_src.shape or k_src.dtype != v_src.dtype:
        raise ValueError(f"k_src / v_src must be [B, rows, Hkv, d] caches of one shape and dtype, got {tuple(k_src.shape)} "
                         f"{k_src.dtype} and {tuple(v_src.shape)} {v_src.dtype}")
    if k_dst.ndim != 3 or k_dst.shape != v_dst.shape or k_dst.dtype != v_dst.dtype:
        raise ValueError(f"k_dst / v_dst must be packed [capacity, Hkv, D] levels of one shape and dtype, got {tuple(k_dst.shape)} "
                         f"{k_dst.dtype} and {tuple(v_dst.shape)} {v_dst.dtype}")
    if k_dst.dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"destination dtype {k_dst.dtype}: shared levels are float16 / bfloat16")
    if not is_fp8(k_src) and k_src.dtype != k_dst.dtype:
        raise ValueError(f"source dtype {k_src.dtype} differs from the destination's {k_dst.dtype}: a 16-bit source is copied as "
                         f"bytes ({FP8_DTYPE} sources are widened)")
    if not is_fp8(k_src) and (k_scale is not None or v_scale is not None):
        raise ValueError("k_scale / v_scale belong to fp8 sources")
    B, src_rows, Hkv, d_src = k_src.shape
    d_dst = k_dst.shape[2]
    if k_dst.shape[1] != Hkv:
        raise ValueError(f"destination has {k_dst.shape[1]} kv heads, the source {Hkv}")
    if d_src % 8:
        raise ValueError(f"head dim {d_src} must be a multiple of 8 (16-byte vectors)")
    if d_dst < d_src or (d_dst != d_src and d_dst not in _DST_DIMS):
        raise ValueError(f"destination head dim {d_dst}: {d_src} (the source's), or a wider one of 64 / 128 / 256")
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is not None and (s.dtype != torch.float32 or s.numel() != Hkv):
            raise ValueError(f"{name} must hold {Hkv} float32 scales, got {tuple(s.shape)} {s.dtype}")
    if rows.ndim != 1 or lens.shape != rows.shape or rows.numel() == 0:
        raise ValueError(f"rows / lens must be two [n] vectors, n >= 1, got {tuple(rows.shape)} and {tuple(lens.shape)}")
    if rows.dtype not in (torch.int32, torch.int64) or lens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"rows / lens must be int32 or int64, got {rows.dtype} and {lens.dtype}")
    return B, src_rows, Hkv, d_src, d_dst, rows.numel()


def promote_kv(k_src: Tensor, v_src: Tensor, rows: Tensor, lens: Tensor, k_dst: Tensor, v_dst: Tensor, *,
               k_scale: Optional[Tensor] = None, v_scale: Optional[Tensor] = None, max_len: Optional[int] = None) -> Tensor:
    """hyd_kv_promote: the first lens[i] tokens of unique sequence rows[i] become packed tokens [cu[i], cu[i + 1]) of the level.

    k_src / v_src [B, rows, Hkv, d] (views of the unique arena: any batch / token / head strides, d contiguous; float16,
    bfloat16, or float8_e4m3fn with per-kv-head float32 k_scale / v_scale, None = 1), k_dst / v_dst packed [capacity, Hkv, D]
    contiguous (float16 / bfloat16; D == d, or a wider 64 / 128 / 256 whose pad columns are written as zeros).  rows / lens: [n]
    device vectors.  Returns cu int32 [n + 1], computed on the device; one launch on the current stream, no synchronisation.
    A 16-bit source is a byte copy; an fp8 source is bit-identical to kv_quant.dequantize_kv.  The kernel skips a sequence whose
    row, length or offset would index outside the caches (nothing raises on the device): `promote_kv_reference` is the definition
    for valid arguments.  max_len: the host's bound on `lens`, if it has one -- the launch grid is sized by it (default: the
    source's rows); a longer sequence is skipped."""
    from .flash import _require_gpu, _stream

    B, src_rows, Hkv, d_src, d_dst, n = _check_promote(k_src, v_src, rows, lens, k_dst, v_dst, k_scale, v_scale)
    _require_gpu(k_src, v_src, rows, lens, k_dst, v_dst, k_scale, v_scale)
    if not (k_dst.is_contiguous() and v_dst.is_contiguous()):
        raise ValueError("k_dst / v_dst must be contiguous")
    if k_src.stride(3) != 1 or v_src.stride(3) != 1:
        raise ValueError("the head dim of k_src / v_src must be contiguous")
    if max_len is not None and not 1 <= int(max_len) <= src_rows:
        raise ValueError(f"max_len {max_len} outside [1, {src_rows}]")
    lib = _lib.load()
    rows32 = rows.to(torch.int32).contiguous()
    lens32 = lens.to(torch.int32).contiguous()
    cu = torch.zeros((n + 1,), dtype=torch.int32, device=lens.device)
    cu[1:] = lens32.cumsum(0, dtype=torch.int32)
    code = {torch.float16: _lib.HYD_F16, torch.bfloat16: _lib.HYD_BF16, FP8_DTYPE: _lib.HYD_FP8_E4M3}
    p = _lib.KvPromoteParams()
    p.k_src, p.v_src, p.k_dst, p.v_dst = k_src.data_ptr(), v_src.data_ptr(), k_dst.data_ptr(), v_dst.data_ptr()
    p.rows, p.lens, p.cu = rows32.data_ptr(), lens32.data_ptr(), cu.data_ptr()
    if k_scale is not None:
        k_scale = k_scale.contiguous()
        p.k_scale = k_scale.data_ptr()
    if v_scale is not None:
        v_scale = v_scale.contiguous()
        p.v_scale = v_scale.data_ptr()
    p.k_batch_stride, p.k_tok_stride, p.k_head_stride = k_src.stride(0), k_src.stride(1), k_src.stride(2)
    p.v_batch_stride, p.v_tok_stride, p.v_head_stride = v_src.stride(0), v_src.stride(1), v_src.stride(2)
    p.src_dtype, p.dst_dtype = code[k_src.dtype], code[k_dst.dtype]
    p.n, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst = n, B, src_rows, Hkv, d_src, d_dst
    p.capacity, p.max_len = k_dst.shape[0], 0 if max_len is None else int(max_len)
    _lib.check(lib.hyd_kv_promote(C.byref(p), _stream()))
    return cu


def promote_kv_reference(k_src: Tensor, v_src: Tensor, rows: Tensor, lens: Tensor, k_dst: Tensor, v_dst: Tensor, *,
                         k_scale: Optional[Tensor] = None, v_scale: Optional[Tensor] = None, max_len: Optional[int] = None) -> Tensor:
    """The definition of promote_kv in torch (any device; reads `lens` on the host): dequantize_kv for fp8 sources, index_select
    of the chosen rows, the first lens[i] tokens of each packed back to back into dst[: sum(lens)], pad columns zero.  Raises where
    the kernel would skip.  Returns cu int32 [n + 1]."""
    B, src_rows, Hkv, d_src, d_dst, n = _check_promote(k_src, v_src, rows, lens, k_dst, v_dst, k_scale, v_scale)
    rows_l, lens_l = [int(x) for x in rows.tolist()], [int(x) for x in lens.tolist()]
    total = sum(lens_l)
    if min(rows_l) < 0 or max(rows_l) >= B or min(lens_l) < 0 or max(lens_l) > src_rows or total > k_dst.shape[0]:
        raise ValueError(f"rows {rows_l} / lens {lens_l} outside a source of [{B}, {src_rows}] or a destination of {k_dst.shape[0]} tokens")
    if max_len is not None and max(lens_l) > max_len:
        raise ValueError(f"lens {lens_l} exceed max_len {max_len}")
    idx = rows.to(device=k_src.device, dtype=torch.int64)
    for src, dst, scale in ((k_src, k_dst, k_scale), (v_src, v_dst, v_scale)):
        if is_fp8(src):  # (the chosen rows first, as bytes: dequantize_kv is elementwise, the values are those of the whole cache)
            sel = dequantize_kv(src.view(torch.uint8).index_select(0, idx).view(FP8_DTYPE), scale, dst.dtype)
        else:
            sel = src.index_select(0, idx)
        if total:
            dst[:total, :, :d_src] = torch.cat([sel[i, : lens_l[i]] for i in range(n)], dim=0)
            dst[:total, :, d_src:] = 0
    cu = torch.zeros((n + 1,), dtype=torch.int32, device=lens.device)
    cu[1:] = lens.to(torch.int32).cumsum(0)
    return cu


def _byte_range(t: Tensor):
    """[first, past the last) byte address a tensor (any strides) can touch."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    span = sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


def _check_gather(levels, k_src, v_src, rows, lens, k_dst, v_dst, old_batch, k_scale, v_scale):
    """What both gather routes refuse: everything _check_promote refuses, chain levels that are no packed levels of the
    destination's geometry, and a destination that overlaps a source (by pointer range).  -> _check_promote's tuple + (divs,)."""
    dims = _check_promote(k_src, v_src, rows, lens, k_dst, v_dst, k_scale, v_scale)
    levels = list(levels)
    if len(levels) > _lib.HYD_MAX_LEVELS:
        raise ValueError(f"{len(levels)} chain levels: at most {_lib.HYD_MAX_LEVELS}")
    old_batch = int(old_batch)
    if old_batch <= 0:
        raise ValueError(f"old_batch {old_batch} must be positive")
    divs = []
    for j, (k, v, cu, s) in enumerate(levels):
        s = int(s)
        if k.ndim != 3 or k.shape != v.shape or k.dtype != k_dst.dtype or v.dtype != k_dst.dtype or k.shape[1:] != k_dst.shape[1:]:
            raise ValueError(f"chain level {j}: k / v must be packed [cap, {k_dst.shape[1]}, {k_dst.shape[2]}] {k_dst.dtype} levels, got "
                             f"{tuple(k.shape)} {k.dtype} and {tuple(v.shape)} {v.dtype}")
        if not (k.is_contiguous() and v.is_contiguous()):
            raise ValueError(f"chain level {j}: k / v must be contiguous")
        if s <= 0 or old_batch % s:
            raise ValueError(f"chain level {j}: {s} shared sequences do not divide the previous batch of {old_batch}")
        if cu.ndim != 1 or cu.dtype != torch.int32 or cu.numel() < s + 1 or not cu.is_contiguous():
            raise ValueError(f"chain level {j}: cu must be a contiguous int32 vector of at least {s + 1} offsets, got {tuple(cu.shape)} {cu.dtype}")
        divs.append(old_batch // s)
    sources = [("k_src", k_src), ("v_src", v_src)] + [(f"chain level {j} {n}", t) for j, lv in enumerate(levels) for n, t in zip("kv", lv[:2])]
    for dname, d in (("k_dst", k_dst), ("v_dst", v_dst)):
        d0, d1 = _byte_range(d)
        for sname, t in sources + ([("v_dst", v_dst)] if dname == "k_dst" else []):
            if t.device == d.device:
                s0, s1 = _byte_range(t)
                if d0 < s1 and s0 < d1:
                    raise ValueError(f"{dname} overlaps {sname}: the gather reads and writes in no order (gather into a staging buffer)")
    return dims + (divs,)


def _cu_dst(levels, divs, rows, lens):
    """Destination offsets [n + 1] int32 from device data, with torch ops (no host read): the parents' lengths plus lens."""
    path = lens.to(torch.int32)
    r = rows.to(device=lens.device, dtype=torch.int64)
    for (_, _, cu, s), div in zip(levels, divs):
        p = (r // div).clamp(0, int(s) - 1)  # (a row outside the batch: the kernel skips that sequence)
        c = cu.to(torch.int64) if cu.dtype != torch.int64 else cu
        path = path + (c[p + 1] - c[p]).to(torch.int32)
    cu_dst = torch.zeros((path.numel() + 1,), dtype=torch.int32, device=lens.device)
    cu_dst[1:] = path.cumsum(0, dtype=torch.int32)
    return cu_dst


def gather_paths(levels, k_src: Tensor, v_src: Tensor, rows: Tensor, lens: Tensor, k_dst: Tensor, v_dst: Tensor, *, old_batch: int,
                 k_scale: Optional[Tensor] = None, v_scale: Optional[Tensor] = None, max_len: Optional[int] = None,
                 max_path: Optional[int] = None) -> Tensor:
    """hyd_kv_gather_paths: destination sequence i becomes the whole path of survivor rows[i] -- for every chain level (k, v, cu, s)
    of `levels`, outermost first, the sequence rows[i] // (old_batch // s) of that level (packed [cap, Hkv, D] k / v of the
    destination's dtype and shape behind the first dim, cu int32 [>= s + 1] device offsets), copied as bytes, and then the first
    lens[i] tokens of unique sequence rows[i], written as promote_kv writes them (k_src / v_src, scales, D as documented there;
    lens[i] may be 0).  k_dst / v_dst: packed [capacity, Hkv, D] contiguous, overlapping no source.  Returns cu_dst int32 [n + 1],
    computed on the device with torch ops; one launch on the current stream, the host is not synchronised.  The kernel skips a
    sequence with a bad row, parent, offset or length (nothing raises on the device): `gather_paths_reference` is the definition
    for valid arguments.  max_len / max_path: the host's bounds on lens and on a path's tokens, if it has them -- the launch grid
    is sized by max_path (default: the destination's capacity); a longer path is skipped."""
    from .flash import _require_gpu, _stream

    levels = [tuple(lv) for lv in levels]
    B, src_rows, Hkv, d_src, d_dst, n, divs = _check_gather(levels, k_src, v_src, rows, lens, k_dst, v_dst, old_batch, k_scale, v_scale)
    _require_gpu(k_src, v_src, rows, lens, k_dst, v_dst, k_scale, v_scale, *[t for lv in levels for t in lv[:3]])
    if not (k_dst.is_contiguous() and v_dst.is_contiguous()):
        raise ValueError("k_dst / v_dst must be contiguous")
    if k_src.stride(3) != 1 or v_src.stride(3) != 1:
        raise ValueError("the head dim of k_src / v_src must be contiguous")
    if max_len is not None and not 1 <= int(max_len) <= src_rows:
        raise ValueError(f"max_len {max_len} outside [1, {src_rows}]")
    if max_path is not None and not 1 <= int(max_path) <= k_dst.shape[0]:
        raise ValueError(f"max_path {max_path} outside [1, capacity = {k_dst.shape[0]}]")
    lib = _lib.load()
    rows32 = rows.to(torch.int32).contiguous()
    lens32 = lens.to(torch.int32).contiguous()
    cu_dst = _cu_dst(levels, divs, rows32, lens32)
    code = {torch.float16: _lib.HYD_F16, torch.bfloat16: _lib.HYD_BF16, FP8_DTYPE: _lib.HYD_FP8_E4M3}
    p = _lib.KvGatherParams()
    for j, ((k, v, cu, s), div) in enumerate(zip(levels, divs)):
        p.level_k[j], p.level_v[j], p.level_cu[j] = k.data_ptr(), v.data_ptr(), cu.data_ptr()
        p.level_s[j], p.level_cap[j], p.level_div[j] = int(s), k.shape[0], div
    p.k_src, p.v_src, p.k_dst, p.v_dst = k_src.data_ptr(), v_src.data_ptr(), k_dst.data_ptr(), v_dst.data_ptr()
    p.rows, p.lens, p.cu_dst = rows32.data_ptr(), lens32.data_ptr(), cu_dst.data_ptr()
    if k_scale is not None:
        k_scale = k_scale.contiguous()
        p.k_scale = k_scale.data_ptr()
    if v_scale is not None:
        v_scale = v_scale.contiguous()
        p.v_scale = v_scale.data_ptr()
    p.k_batch_stride, p.k_tok_stride, p.k_head_stride = k_src.stride(0), k_src.stride(1), k_src.stride(2)
    p.v_batch_stride, p.v_tok_stride, p.v_head_stride = v_src.stride(0), v_src.stride(1), v_src.stride(2)
    p.src_dtype, p.dst_dtype = code[k_src.dtype], code[k_dst.dtype]
    p.n, p.n_levels, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst = n, len(levels), B, src_rows, Hkv, d_src, d_dst
    p.capacity, p.max_len, p.max_path = k_dst.shape[0], 0 if max_len is None else int(max_len), 0 if max_path is None else int(max_path)
    _lib.check(lib.hyd_kv_gather_paths(C.byref(p), _stream()))
    return cu_dst


def gather_paths_reference(levels, k_src: Tensor, v_src: Tensor, rows: Tensor, lens: Tensor, k_dst: Tensor, v_dst: Tensor, *,
                           old_batch: int, k_scale: Optional[Tensor] = None, v_scale: Optional[Tensor] = None,
                           max_len: Optional[int] = None, max_path: Optional[int] = None) -> Tensor:
    """The definition of gather_paths in torch (any device; reads rows, lens and the levels' offsets on the host): per survivor,
    the slices of its parents' sequences in the chain levels, then its unique rows as promote_kv_reference writes them
    (dequantize_kv for fp8 sources, pad columns zero), concatenated and packed back to back into dst[: total].  Raises where the
    kernel would skip.  Returns cu_dst int32 [n + 1]."""
    levels = [tuple(lv) for lv in levels]
    B, src_rows, Hkv, d_src, d_dst, n, divs = _check_gather(levels, k_src, v_src, rows, lens, k_dst, v_dst, old_batch, k_scale, v_scale)
    rows_l, lens_l = [int(x) for x in rows.tolist()], [int(x) for x in lens.tolist()]
    if min(rows_l) < 0 or max(rows_l) >= B or min(lens_l) < 0 or max(lens_l) > src_rows:
        raise ValueError(f"rows {rows_l} / lens {lens_l} outside a source of [{B}, {src_rows}]")
    if max_len is not None and max(lens_l) > max_len:
        raise ValueError(f"lens {lens_l} exceed max_len {max_len}")
    segs = [[] for _ in range(n)]  # per survivor: (level index, first token, past the last token)
    for j, ((k, _, cu, s), div) in enumerate(zip(levels, divs)):
        cu_l = [int(x) for x in cu[: int(s) + 1].tolist()]
        for i, r in enumerate(rows_l):
            p = r // div
            if p >= int(s):
                raise ValueError(f"rows[{i}] = {r}: parent {p} outside chain level {j} of {s} sequences")
            lo, hi = cu_l[p], cu_l[p + 1]
            if lo < 0 or hi < lo or hi > k.shape[0]:
                raise ValueError(f"chain level {j}: sequence {p} spans [{lo}, {hi}) of {k.shape[0]} tokens")
            segs[i].append((j, lo, hi))
    path = [sum(hi - lo for _, lo, hi in segs[i]) + lens_l[i] for i in range(n)]
    total = sum(path)
    if total > k_dst.shape[0] or (max_path is not None and max(path) > max_path):
        raise ValueError(f"paths of {path} tokens exceed the destination's {k_dst.shape[0]} tokens or max_path {max_path}")
    idx = rows.to(device=k_src.device, dtype=torch.int64)
    for which, (src, dst, scale) in enumerate(((k_src, k_dst, k_scale), (v_src, v_dst, v_scale))):
        if is_fp8(src):  # (the chosen rows first, as bytes: dequantize_kv is elementwise, the values are those of the whole cache)
            sel = dequantize_kv(src.view(torch.uint8).index_select(0, idx).view(FP8_DTYPE), scale, dst.dtype)
        else:
            sel = src.index_select(0, idx)
        pieces = []
        for i in range(n):
            pieces += [levels[j][which][lo:hi].to(dst.device) for j, lo, hi in segs[i]]
            pieces.append(torch.nn.functional.pad(sel[i, : lens_l[i]], (0, d_dst - d_src)).to(dst.device))
        if total:
            dst[:total] = torch.cat(pieces, dim=0)
    cu_dst = torch.zeros((n + 1,), dtype=torch.int32, device=lens.device)
    cu_dst[1:] = torch.tensor(path, dtype=torch.int32).cumsum(0).to(torch.int32)
    return cu_dst


def check_fork_rows(rows: Sequence[int], old_batch: int, level_batch_sizes: Sequence[int]) -> None:
    """The host rule that keeps the hierarchy regular after a fork.  Sequence i of a batch reads shared sequence i // (batch / sb)
    of a level of sb sequences, before and after: with k = len(rows), every level in use with s sequences needs k % s == 0 and
    rows[i] // (old_batch // s) == i // (k // s) for every i -- the same number of survivors in every group of every level, listed
    in group order, in any order within a group.  Rows are distinct and inside [0, old_batch).  Raises ValueError naming the level
    and the index."""
    rows = [int(r) for r in rows]
    k, old_batch = len(rows), int(old_batch)
    if k == 0:
        raise ValueError("fork of no rows")
    if old_batch <= 0:
        raise ValueError(f"old_batch {old_batch} must be positive")
    seen = {}
    for i, r in enumerate(rows):
        if not 0 <= r < old_batch:
            raise ValueError(f"rows[{i}] = {r} is outside the previous batch of {old_batch}")
        if r in seen:
            raise ValueError(f"rows[{i}] = {r} repeats rows[{seen[r]}]: a completion is promoted once (sample it several times instead)")
        seen[r] = i
    for lvl, s in enumerate(int(x) for x in level_batch_sizes):
        if s <= 0 or old_batch % s:
            raise ValueError(f"level {lvl}: {s} shared sequences do not divide the previous batch of {old_batch}")
        if k % s:
            raise ValueError(f"level {lvl}: {k} rows are no multiple of its {s} shared sequences (the same number of survivors per group)")
        per_old, per_new = old_batch // s, k // s
        for i, r in enumerate(rows):
            if r // per_old != i // per_new:
                raise ValueError(f"level {lvl}: rows[{i}] = {r} hangs off shared sequence {r // per_old} but position {i} of {k} reads "
                                 f"sequence {i // per_new} ({per_new} survivors per group, listed in group order)")


def select_beams(scores, group_size: int, width: int) -> Tensor:
    """Row indices [G * width] (int64, on the scores' device) of the `width` best of every group of `group_size` consecutive scores
    [G * group_size] (host or device): listed in group order and, within a group, by descending score, ties to the lower row index.
    The result passes check_fork_rows for any levels whose groups are unions of these groups."""
    s = torch.as_tensor(scores)
    group_size, width = int(group_size), int(width)
    if s.ndim != 1 or group_size <= 0 or s.numel() == 0 or s.numel() % group_size:
        raise ValueError(f"scores must be [G * group_size], got {tuple(s.shape)} for group_size {group_size}")
    if not 1 <= width <= group_size:
        raise ValueError(f"width {width} outside [1, group_size = {group_size}]")
    G = s.numel() // group_size
    order = torch.sort(s.reshape(G, group_size), dim=1, descending=True, stable=True).indices[:, :width]
    return (order + torch.arange(G, device=s.device)[:, None] * group_size).reshape(-1)


@torch.no_grad()
def stepwise_beam_search(model, input_ids, *, width: int, expand: int, step_tokens: int, steps: int,
                         score_fn: Optional[Callable[[Tensor, Tensor], Tensor]] = None, return_trace: bool = False,
                         select: str = "path", **sampling):
    """Step-level search over a forked hierarchy: `steps` rounds of `step_tokens` tokens each, `width` paths per prompt.

    input_ids: generate()'s prompt levels, all shared (a tensor [G, P] or a list of levels, the last one [G, p]); G prompts.
    Round 0 samples width * expand candidates per prompt and keeps the `width` best of each prompt.  Every later round samples
    `expand` children per kept path; which of them survive is `select`:
      "path"    the best child of EACH path: a plain fork must leave the same number of survivors under every sequence of every
                level in use (check_fork_rows), and the level promoted by the round before has one sequence per path -- `width`
                independent chains after round 0.  One shared level per round but the last: the caches need steps - 1 free
                levels of G * width sequences and step_tokens tokens behind the prompt's levels.
      "prompt"  beam search: select_beams(scores, width * expand, width) in every round, the global top-`width` of the children of
                ALL paths of a prompt -- two children of a strong path and none of a weak one is a valid outcome.  From round 1
                on the fork merges (model.fork(merge_from= the index of the path level)): every survivor's whole path since the
                prompt is gathered into the one level behind the prompt's, whatever its parent, so the hierarchy stays at
                prompt levels + 1 however many rounds run.  The caches need ONE level of G * width sequences of up to
                (steps - 1) * step_tokens tokens behind the prompt's levels (a merged fork copies the path: its cost grows with
                the round, profiles/fork_merge.md).
    Per round: generate(..., return_logprobs=True, shared_cache_op="extend"), select_beams, model.fork, then the next round with
    each survivor's first uncached token as a one-token unique prompt.

    A candidate's score is the cumulative log-prob of its path (the log-probs generate() returns), or score_fn(tokens, logprobs)
    of the candidates' paths so far ([rows, tokens so far] each) -> [rows].  **sampling goes to generate() (temperature, top_k,
    top_p, min_p, penalties ...).  Returns (tokens [G * width, steps * step_tokens], scores [G * width]); with return_trace also a
    list with one dict per round: candidate_scores [rows] (CPU), group_size, width (what select_beams was called with), rows (the
    chosen candidates, CPU), parents (the kept path -- round 0: the prompt -- each one continues), tokens / logprobs [G * width, step_tokens] of the kept
    paths' new step.  The number of shared levels in use is restored when the call returns or raises.
    No EOS or stop handling in this version: every path runs steps * step_tokens tokens."""
    width, expand, step_tokens, steps = int(width), int(expand), int(step_tokens), int(steps)
    if width < 1 or expand < 1 or steps < 1:
        raise ValueError(f"width {width}, expand {expand} and steps {steps} must be >= 1")
    if select not in ("path", "prompt"):
        raise ValueError(f'select {select!r}: "path" (the best child of each path) or "prompt" (the global top-width per prompt)')
    if step_tokens < 2:
        raise ValueError(f"step_tokens {step_tokens}: a round caches step_tokens - 1 tokens per path, a fork promotes at least one")
    for name in ("num_return_sequences", "max_new_tokens", "return_logprobs", "shared_cache_op", "return_logits", "token_overrides",
                 "stop", "return_finish", "seq_lens"):
        if name in sampling:
            raise ValueError(f"{name} is set by stepwise_beam_search")
    levels = [input_ids] if isinstance(input_ids, Tensor) else list(input_ids)
    G = levels[-1].shape[0]
    T = step_tokens
    levels_before = model.get_num_used_shared_caches()
    trace = []
    try:
        paths = path_lp = last = None
        for rnd in range(steps):
            if rnd == 0:
                new, lp = model.generate(input_ids=levels, num_return_sequences=width * expand, max_new_tokens=T,
                                         return_logprobs=True, shared_cache_op="extend", **sampling)
                group, keep = width * expand, width
                cand, cand_lp = new, lp
            else:
                new, lp = model.generate(input_ids=last.repeat_interleave(expand, 0)[:, None], num_return_sequences=1,
                                         max_new_tokens=T, return_logprobs=True, shared_cache_op="extend", **sampling)
                group, keep = (expand, 1) if select == "path" else (width * expand, width)
                cand = torch.cat([paths.repeat_interleave(expand, 0), new], dim=1)
                cand_lp = torch.cat([path_lp.repeat_interleave(expand, 0), lp], dim=1)
            scores = cand_lp.sum(1) if score_fn is None else torch.as_tensor(score_fn(cand, cand_lp)).to(cand_lp.device).reshape(-1)
            if scores.numel() != cand.shape[0]:
                raise ValueError(f"score_fn returned {scores.numel()} scores for {cand.shape[0]} candidates")
            rows = select_beams(scores, group, keep)
            # the kept path (round 0: the prompt) each chosen candidate continues
            parents = rows // (group if rnd == 0 or select == "path" else expand)
            old_batch = cand.shape[0]
            if rnd + 1 < steps:
                # cached per candidate: its one-token prompt (rounds >= 1) and the step's tokens but the last, which was never fed
                fed = new[rows, : T - 1] if rnd == 0 else torch.cat([last[parents][:, None], new[rows, : T - 1]], dim=1)
                # "prompt", rounds >= 1: the level the round before left behind the prompt's levels is the path level
                merge = model.get_num_used_shared_caches() - 1 if (select == "prompt" and rnd > 0) else None
                model.fork(rows, torch.full((rows.numel(),), fed.shape[1], dtype=torch.int32, device=rows.device), fed, old_batch,
                           merge_from=merge)
            paths, path_lp, last, best = cand[rows], cand_lp[rows], new[rows, T - 1], scores[rows]
            if return_trace:
                trace.append(dict(candidate_scores=scores.detach().cpu(), group_size=group, width=keep, rows=rows.cpu(),
                                  parents=parents.cpu(), tokens=new[rows].cpu(), logprobs=lp[rows].cpu()))
        return (paths, best, trace) if return_trace else (paths, best)
    finally:
        model.truncate_shared_caches(levels_before)
