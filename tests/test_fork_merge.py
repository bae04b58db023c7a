"""-m "not gpu": fork with merged levels (hydragen_amd/fork.py gather_paths, hyd_kv_gather_paths) -- the ABI bookkeeping of the entry
point, its refusals (they run before any launch, so they need no device), the torch definition of the gather against a plain
Python loop, the host rule on the levels below the merge, the merged level's bookkeeping on CPU tensors, and the register
metadata of the new kernel next to kv_promote_kernel's."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd.fork import check_fork_rows, gather_paths_reference, select_beams
from hydragen_amd.kv_quant import FP8_DTYPE, dequantize_kv

REPO = Path(__file__).resolve().parent.parent
PTR = 0x7F0000001000  # never dereferenced on the host: the entry point only checks null / alignment


def test_header_exports_and_library_agree_on_the_entry_point():
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    assert re.search(r"HYD_API int hyd_kv_gather_paths\(const hyd_kv_gather_params\* p, void\* stream\);", header)
    assert "typedef struct hyd_kv_gather_params" in header
    assert "MUST NOT\n * OVERLAP ANY SOURCE" in header or "MUST NOT OVERLAP ANY SOURCE" in header.replace("\n *", "")
    assert "hyd_kv_gather_paths" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "hyd_kv_gather_paths")
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(_lib.lib_path())], text=True)
    assert any(ln.split()[-1] == "hyd_kv_gather_paths" and " T " in ln for ln in out.splitlines())
    assert lib.hyd_version() == 500  # a new symbol only: no existing struct changed
    assert "kv_gather.hip" in (REPO / "hydragen_amd" / "csrc" / "build.py").read_text()
    # the widening helpers live in one header that both copy kernels include
    for src in ("kv_promote.hip", "kv_gather.hip"):
        text = (REPO / "hydragen_amd" / "csrc" / src).read_text()
        assert '#include "kv_widen.h"' in text and "widen8(const" not in text and "cvt1(float" not in text, src


def test_struct_layout_matches_c():
    """The ctypes mirror has the size gcc gives the C struct, and the fields sit where gcc puts them."""
    names = [n for n, _ in _lib.KvGatherParams._fields_]
    offs = "".join(f'printf("%zu ", offsetof(hyd_kv_gather_params, {n}));' for n in names)
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu ", sizeof(hyd_kv_gather_params));'
           + offs + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got[0] == C.sizeof(_lib.KvGatherParams)
    assert got[1:] == [getattr(_lib.KvGatherParams, n).offset for n in names]
    assert len(_lib.KvGatherParams().level_k) == _lib.HYD_MAX_LEVELS == 8


def _params(levels=2, **kw):
    p = _lib.KvGatherParams()
    p.k_src = p.v_src = p.k_dst = p.v_dst = p.rows = p.lens = p.cu_dst = PTR
    p.k_batch_stride = p.v_batch_stride = 2 * 48 * 8 * 128
    p.k_tok_stride = p.v_tok_stride = 8 * 128
    p.k_head_stride = p.v_head_stride = 128
    p.src_dtype = p.dst_dtype = _lib.HYD_BF16
    p.n, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst, p.capacity = 4, 12, 48, 8, 128, 128, 4 * 96
    p.n_levels = levels
    for j, s in enumerate((4, 2, 1, 1, 1, 1, 1, 1)[: min(max(levels, 0), 8)]):
        p.level_k[j] = p.level_v[j] = p.level_cu[j] = PTR
        p.level_s[j], p.level_cap[j], p.level_div[j] = s, 17 * s, 12 // s
    for k, v in kw.items():
        if isinstance(v, tuple):  # (index, value) of a per-level array
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,code,frag", [
    # what hyd_kv_promote refuses
    (dict(dst_dtype=_lib.HYD_FP8_E4M3, src_dtype=_lib.HYD_FP8_E4M3), -2, "dst_dtype"),
    (dict(dst_dtype=_lib.HYD_F32), -2, "dst_dtype"),
    (dict(d_src=128, d_dst=64), -1, "d_dst"),
    (dict(d_src=100, d_dst=128), -1, "d_src"),
    (dict(d_src=4, d_dst=64), -1, "d_src"),
    (dict(n=0), -1, "n 0"),
    (dict(n=-3), -1, "n -3"),
    (dict(Hkv=0), -1, "Hkv"),
    (dict(k_src=None), -1, "k_src"),
    (dict(v_src=None), -1, "v_src"),
    (dict(k_dst=None), -1, "k_dst"),
    (dict(v_dst=None), -1, "v_dst"),
    (dict(rows=None), -1, "rows"),
    (dict(lens=None), -1, "lens"),
    (dict(cu_dst=None), -1, "cu_dst"),
    (dict(src_dtype=_lib.HYD_F16), -1, "src_dtype"),
    (dict(src_dtype=_lib.HYD_F32), -2, "src_dtype"),
    (dict(d_src=80, d_dst=96), -2, "d_dst"),
    (dict(k_tok_stride=8 * 128 + 4), -1, "k_tok_stride"),
    (dict(v_src=PTR + 8), -1, "v_src"),
    (dict(max_len=49), -1, "max_len"),
    (dict(n=70000), -2, "n 70000"),
    # and the chain's own
    (dict(levels=-1), -1, "n_levels -1"),
    (dict(levels=9), -1, "n_levels 9"),
    (dict(level_k=(1, None)), -1, "level_k[1]"),
    (dict(level_v=(0, None)), -1, "level_v[0]"),
    (dict(level_v=(1, PTR + 4)), -1, "level_v[1]"),
    (dict(level_cu=(1, None)), -1, "level_cu[1]"),
    (dict(level_div=(0, 0)), -1, "level_div[0]"),
    (dict(level_div=(1, -6)), -1, "level_div[1]"),
    (dict(level_s=(1, 0)), -1, "level_s[1]"),
    (dict(level_cap=(0, -1)), -1, "level_cap[0]"),
    (dict(max_path=4 * 96 + 1), -1, "max_path"),
    (dict(max_path=-1), -1, "max_path"),
    (dict(capacity=2**31 - 1, max_path=2**31 - 1), -2, "max_path"),   # x Hkv 8 x d_dst 128 / 8 >= 2^31 vectors
    (dict(capacity=2**24), -2, "max_path"),                           # the default bound is the capacity
])
def test_refusals_come_before_any_launch_and_name_the_field(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_kv_gather_paths(C.byref(_params(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode(), lib.hyd_last_error_string().decode()


def test_null_params_and_valid_parameters_without_a_device():
    lib = _lib.load()
    assert lib.hyd_kv_gather_paths(None, None) == -1
    if torch.cuda.is_available():
        return  # a device is present: a launch on made-up pointers is not issued
    # every accepted form reaches the launch, which fails cleanly without a device (HYD_ERR_LAUNCH), it does not crash
    for kw in (dict(), dict(levels=0), dict(levels=1), dict(levels=8), dict(d_src=80, d_dst=128), dict(src_dtype=_lib.HYD_FP8_E4M3),
               dict(src_dtype=_lib.HYD_FP8_E4M3, dst_dtype=_lib.HYD_F16, k_scale=PTR, v_scale=PTR), dict(max_len=17, max_path=60),
               dict(src_dtype=_lib.HYD_F16, dst_dtype=_lib.HYD_F16, Hkv=1, d_src=64, d_dst=64),
               dict(levels=1, level_k=(5, None))):  # (a level past n_levels is not looked at)
        assert lib.hyd_kv_gather_paths(C.byref(_params(**kw)), None) == -4, kw
        assert "kv_gather" in lib.hyd_last_error_string().decode()


# ---- gather_paths_reference against a plain Python loop --------------------------------------------------------------------
def _arena(B, rows, Hkv, d, dtype, seed):
    from hydragen_amd import placement

    arena = placement.kv_arena((B, rows, Hkv, d), dtype, "cpu", zero=True)
    g = torch.Generator().manual_seed(seed)
    if dtype == FP8_DTYPE:
        arena.view(torch.uint8).copy_(torch.randint(0, 256, tuple(arena.shape), dtype=torch.uint8, generator=g))
    else:
        arena.copy_(torch.randn(tuple(arena.shape), generator=g).to(dtype))
    return arena[0], arena[1]


def _chain(sizes, Hkv, D, dtype, seed, slack=3):
    """Packed chain levels [(k, v, cu, s)] with ragged lengths from {1, 15, 16, 17} and `slack` unused tokens behind them."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in sizes:
        lens = torch.tensor([1, 15, 16, 17])[torch.randint(0, 4, (s,), generator=g)]
        cu = torch.zeros(s + 1, dtype=torch.int32)
        cu[1:] = lens.cumsum(0)
        cap = int(cu[-1]) + slack
        out.append((torch.randn(cap, Hkv, D, generator=g).to(dtype), torch.randn(cap, Hkv, D, generator=g).to(dtype), cu, s))
    return out


def _loop_expect(levels, src, which, rows, lens, old_batch, scale, dtype, D):
    """Token by token: the path of every survivor as a list of [Hkv, D] rows."""
    x = src if src.dtype != FP8_DTYPE else dequantize_kv(src, scale, dtype)
    toks = []
    for r, n in zip(rows, lens):
        for lv in levels:
            p = r // (old_batch // lv[3])
            for t in range(int(lv[2][p]), int(lv[2][p + 1])):
                toks.append(lv[which][t])
        for t in range(n):
            row = torch.zeros(x.shape[2], D, dtype=dtype)
            row[:, : x.shape[3]] = x[r, t]
            toks.append(row)
    return torch.stack(toks) if toks else torch.zeros(0, x.shape[2], D, dtype=dtype)


@pytest.mark.parametrize("dtype,src_dtype,Hkv,d,D", [
    (torch.bfloat16, torch.bfloat16, 4, 64, 64),
    (torch.float16, torch.float16, 2, 128, 128),
    (torch.bfloat16, torch.bfloat16, 8, 80, 128),     # a narrow unique source
    (torch.bfloat16, FP8_DTYPE, 8, 64, 64),
    (torch.float16, FP8_DTYPE, 8, 128, 128),
])
@pytest.mark.parametrize("sizes", [(), (4,), (1, 4, 2)], ids=lambda s: f"levels{len(s)}")
def test_gather_paths_reference_against_a_python_loop(dtype, src_dtype, Hkv, d, D, sizes):
    B, R = 12, 48
    rows, lens = [7, 6, 8, 2, 11], [15, 0, 48, 1, 17]     # three children of parent 2 of 4 (rows 6..8), none of parent 1, not monotone
    k, v = _arena(B, R, Hkv, d, src_dtype, 3)
    fp8 = src_dtype == FP8_DTYPE
    ks = (torch.arange(Hkv).float() * 0.37 + 0.11) if fp8 else None
    vs = (torch.arange(Hkv).float() * 0.05 + 1.3) if fp8 else None
    kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    levels = _chain(sizes, Hkv, D, dtype, seed=len(sizes) + Hkv)
    want_k = _loop_expect(levels, k, 0, rows, lens, B, ks, dtype, D)
    want_v = _loop_expect(levels, v, 1, rows, lens, B, vs, dtype, D)
    total = want_k.shape[0]
    sentinel = torch.full((total + 5, Hkv, D), 7.0, dtype=dtype)
    kd, vd = sentinel.clone(), sentinel.clone()
    cu = gather_paths_reference(levels, k, v, torch.tensor(rows), torch.tensor(lens), kd, vd, old_batch=B, **kw)
    paths = [sum(int(lv[2][r // (B // lv[3]) + 1] - lv[2][r // (B // lv[3])]) for lv in levels) + n for r, n in zip(rows, lens)]
    assert cu.dtype == torch.int32 and cu.tolist() == [0] + torch.tensor(paths).cumsum(0).tolist() and cu[-1] == total
    bits = lambda t: t.view(torch.int16)
    for dst, want in ((kd, want_k), (vd, want_v)):
        nan = want.isnan()
        assert torch.equal(dst[:total].isnan(), nan)
        assert torch.equal(bits(dst[:total])[~nan], bits(want)[~nan])
        assert torch.equal(dst[total:], sentinel[total:])          # tokens past cu_dst[n] are untouched
    # it raises where the kernel would skip
    t = torch.tensor
    with pytest.raises(ValueError):
        gather_paths_reference(levels, k, v, t([0, 12]), t([1, 1]), kd, vd, old_batch=B, **kw)
    with pytest.raises(ValueError):
        gather_paths_reference(levels, k, v, t([0, 1]), t([1, R + 1]), kd, vd, old_batch=B, **kw)
    with pytest.raises(ValueError):
        gather_paths_reference(levels, k, v, t(rows), t(lens), kd[: total - 1], vd[: total - 1], old_batch=B, **kw)
    with pytest.raises(ValueError, match="max_path"):
        gather_paths_reference(levels, k, v, t(rows), t(lens), kd, vd, old_batch=B, max_path=max(paths) - 1, **kw)
    if sizes:
        bad = [tuple(lv) for lv in levels]
        cu_bad = bad[-1][2].clone()
        cu_bad[-1] = bad[-1][0].shape[0] + 1                      # the last sequence runs past the level
        bad[-1] = bad[-1][:2] + (cu_bad,) + bad[-1][3:]
        with pytest.raises(ValueError, match="chain level"):
            gather_paths_reference(bad, k, v, t([B - 1]), t([1]), kd, vd, old_batch=B, **kw)
        with pytest.raises(ValueError, match="do not divide"):
            gather_paths_reference(levels, k, v, t(rows), t(lens), kd, vd, old_batch=B + 1, **kw)
        with pytest.raises(ValueError, match="overlaps chain level 0 k"):   # a destination that is a source
            gather_paths_reference(levels, k, v, t(rows), t(lens), levels[0][0], vd[: levels[0][0].shape[0]], old_batch=B, **kw)
    if not fp8 and d == D:
        with pytest.raises(ValueError, match="overlaps k_src"):
            gather_paths_reference(levels, k, v, t([0]), t([1]), k[0], vd[:R], old_batch=B)
        with pytest.raises(ValueError, match="dtype"):
            other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
            gather_paths_reference(levels, k, v, t(rows), t(lens), kd.to(other), vd.to(other), old_batch=B)


def test_gather_routes_refuse_what_promote_refuses_and_need_a_gpu():
    from hydragen_amd.fork import gather_paths

    k, v = _arena(4, 8, 2, 64, torch.bfloat16, 1)
    kd, vd = torch.zeros(16, 2, 64, dtype=torch.bfloat16), torch.zeros(16, 2, 64, dtype=torch.bfloat16)
    t = torch.tensor
    for fn in (gather_paths, gather_paths_reference):
        with pytest.raises(ValueError, match="rows / lens"):
            fn([], k, v, t([], dtype=torch.int64), t([], dtype=torch.int64), kd, vd, old_batch=4)
        with pytest.raises(ValueError, match="kv heads"):
            fn([], k, v, t([0]), t([1]), kd[:, :1], vd[:, :1], old_batch=4)
        with pytest.raises(ValueError, match="chain level 0"):
            fn([(kd[:, :, :32], vd[:, :, :32], torch.zeros(2, dtype=torch.int32), 1)], k, v, t([0]), t([1]), kd, vd, old_batch=4)
        with pytest.raises(ValueError, match="old_batch"):
            fn([], k, v, t([0]), t([1]), kd, vd, old_batch=0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        gather_paths([], k, v, t([0]), t([1]), kd, vd, old_batch=4)


# ---- the host rule on the levels below the merge ------------------------------------------------------------------------------
def test_check_fork_rows_below_the_merge_accepts_uneven_parents():
    """G = 2 prompts, width 2, expand 3: 12 candidates, prompt levels of 1 and 2 sequences, a path level of 4.  The global top-2
    per prompt may take both survivors of a prompt from ONE path: the path level refuses that, the prompt levels do not -- and a
    merged fork checks only those.  A row that crosses a prompt group is refused by the prompt levels themselves."""
    old, prompt, path = 12, [1, 2], [1, 2, 4]
    for rows in ([0, 2, 9, 11], [1, 0, 10, 11], [3, 5, 6, 7], [2, 4, 8, 6]):   # (0, 0 | 3, 3), (0, 0 | 3, 3), (1, 1 | 2, 2), (0, 1 | 2, 2)
        check_fork_rows(rows, old, prompt)
    for rows in ([0, 2, 9, 11], [1, 0, 10, 11], [3, 5, 6, 7]):
        with pytest.raises(ValueError, match="level 2"):
            check_fork_rows(rows, old, path)
    scores = torch.tensor([9., 8., 7., 0., 0., 0., 0., 0., 0., 5., 4., 6.])     # prompt 0: all of path 0; prompt 1: all of path 3
    rows = select_beams(scores, 6, 2).tolist()
    assert rows == [0, 1, 11, 9] and [r // 3 for r in rows] == [0, 0, 3, 3]
    check_fork_rows(rows, old, prompt)
    for rows, frag in (([0, 6, 7, 8], r"level 1: rows\[1\] = 6"), ([0, 1, 2, 6], r"level 1: rows\[2\] = 2"), ([7, 8, 0, 1], r"level 1: rows\[0\] = 7")):
        with pytest.raises(ValueError, match=frag):
            check_fork_rows(rows, old, prompt)
    with pytest.raises(ValueError, match="repeats"):
        check_fork_rows([0, 0, 6, 7], old, prompt)


# ---- the merged level's bookkeeping -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_dim", [64, 80])
def test_promote_unique_merged_leaves_the_level_as_fill_would(head_dim):
    """PerLayerKVCache.promote_unique_merged through the torch route on CPU: slot `base` holds exactly what SharedCache.fill leaves
    for the concatenated paths on a cache with the same history, the levels behind it are dropped, and fill's errors are raised
    before anything is written."""
    from hydragen_amd.llama import PerLayerKVCache

    H, B = 8, 12
    bf = torch.bfloat16

    def cache():
        c = PerLayerKVCache(B, 16, [1, 6, 4], [8, 40, 12], H, head_dim, "cpu", bf)
        g = torch.Generator().manual_seed(1)
        rnd = lambda *s: torch.randn(*s, generator=g).to(bf)
        c.per_completion_k_cache.copy_(rnd(B, 16, H, head_dim))
        c.per_completion_v_cache.copy_(rnd(B, 16, H, head_dim))
        c.append_shared(rnd(1, 8, H, head_dim), rnd(1, 8, H, head_dim), torch.tensor([8]))
        c.append_shared(rnd(4, 9, H, head_dim), rnd(4, 9, H, head_dim), torch.tensor([9, 3, 1, 7]))     # the chain: 4 paths ...
        c.append_shared(rnd(2, 12, H, head_dim), rnd(2, 12, H, head_dim), torch.tensor([12, 5]))        # ... and a level of 2
        return c

    D = cache().kernel_head_dim
    assert D == (128 if head_dim == 80 else 64)
    t32 = lambda x: torch.tensor(x, dtype=torch.int32)
    for rows, lens in (([7, 6, 8, 2, 11], [5, 0, 12, 1, 7]), ([0, 1], [3, 3]), ([9, 10, 11], [2, 2, 2])):
        a, b = cache(), cache()
        A, Bl = a.shared_caches[1], a.shared_caches[2]
        cuA, cuB = A.cumsum_lengths.tolist(), Bl.cumsum_lengths.tolist()
        paths_k, paths_v, plen = [], [], []
        for r, n in zip(rows, lens):
            pa, pb = r // 3, r // 6
            pad = lambda x: torch.nn.functional.pad(x, (0, D - head_dim))
            paths_k.append(torch.cat([A.k_cache[cuA[pa] : cuA[pa + 1]], Bl.k_cache[cuB[pb] : cuB[pb + 1]], pad(a.per_completion_k_cache[r, :n])]))
            paths_v.append(torch.cat([A.v_cache[cuA[pa] : cuA[pa + 1]], Bl.v_cache[cuB[pb] : cuB[pb + 1]], pad(a.per_completion_v_cache[r, :n])]))
            plen.append(paths_k[-1].shape[0])
        a.promote_unique_merged(1, t32(rows), t32(lens), plen, old_batch=B, use_kernel=False)
        stack = lambda ps: torch.stack([torch.nn.functional.pad(p, (0, 0, 0, 0, 0, max(plen) - p.shape[0])) for p in ps])
        b.truncate_shared_caches(1)
        b.append_shared(stack(paths_k), stack(paths_v), torch.tensor(plen))
        sa, sb = a.shared_caches[1], b.shared_caches[1]
        assert a.num_used_shared_caches == b.num_used_shared_caches == 2
        for name in ("k_cache", "v_cache", "seq_lens", "cumsum_lengths"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), (rows, name)
        assert (sa.use_varlen, sa.sliced_sequence_length, sa.current_batch_size) == (sb.use_varlen, sb.sliced_sequence_length, sb.current_batch_size)
        assert sa.current_batch_size == len(rows) and sa.use_varlen == (len(set(plen)) > 1)
    # merging from the end of the chain is the plain promote
    a, b = cache(), cache()
    a.truncate_shared_caches(2), b.truncate_shared_caches(2)
    a.promote_unique_merged(2, t32([5, 0, 3]), t32([5, 12, 7]), [5, 12, 7], old_batch=B, use_kernel=False)
    b.promote_unique(t32([5, 0, 3]), t32([5, 12, 7]), [5, 12, 7], use_kernel=False)
    for name in ("k_cache", "v_cache", "seq_lens", "cumsum_lengths"):
        assert torch.equal(getattr(a.shared_caches[2], name), getattr(b.shared_caches[2], name)), name
    assert a.num_used_shared_caches == b.num_used_shared_caches == 3
    # refusals: nothing moves
    c = cache()
    snap = [x.clone() for s in c.shared_caches for x in (s.k_cache, s.v_cache, s.seq_lens, s.cumsum_lengths)]
    for args, frag in (((1, t32(list(range(7))), t32([1] * 7), [11] * 7), "Batch size 7 exceeds"),
                       ((1, t32([0, 1]), t32([16, 1]), [41, 22]), "Sequence length 41 exceeds"),
                       ((2, t32([0, 1, 2, 3]), t32([1] * 4), [13] * 4), "Sequence length 13 exceeds"),
                       ((4, t32([0]), t32([1]), [1]), "merge_from 4"),
                       ((-1, t32([0]), t32([1]), [1]), "merge_from -1")):
        with pytest.raises(ValueError, match=frag):
            c.promote_unique_merged(*args, old_batch=B, use_kernel=False)
        assert c.num_used_shared_caches == 3
        now = [x for s in c.shared_caches for x in (s.k_cache, s.v_cache, s.seq_lens, s.cumsum_lengths)]
        assert all(torch.equal(x, y) for x, y in zip(now, snap)), frag
    with pytest.raises(ValueError, match="No more available shared caches"):
        c.promote_unique_merged(3, t32([0]), t32([1]), [1], old_batch=B, use_kernel=False)


# ---- the kernel's build ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")
def test_gather_kernel_has_no_scratch_and_no_more_registers_than_promote():
    """Every instantiation (16-bit byte copy, fp8 -> f16, fp8 -> bf16): private segment size 0, nothing spilled, and a VGPR count
    no higher than the same instantiation of kv_promote_kernel in the same build (the occupancy the copy was measured at);
    16-byte vector loads and stores, no LDS, no hand-written assembly in the source."""
    from tests.test_build_quality import _device_asm, _metadata

    _, gather = _metadata("kv_gather.hip")
    _, promote = _metadata("kv_promote.hip")
    mode = lambda k: re.search(r"ILi(\d)E", k["name"]).group(1)
    assert len(gather) == 3 and all("kv_gather_paths_kernel" in k["name"] for k in gather), [k["name"] for k in gather]
    budget = {mode(k): k["vgpr"] for k in promote if "kv_promote_kernel" in k["name"]}
    assert sorted(budget) == ["0", "1", "2"]
    for k in gather:
        assert k["scratch"] == 0 and k["spill"] == 0 and k["sspill"] == 0, k
        assert k["vgpr"] <= budget[mode(k)], (k, budget)
    asm = _device_asm("kv_gather.hip")
    src = (REPO / "hydragen_amd" / "csrc" / "kv_gather.hip").read_text() + (REPO / "hydragen_amd" / "csrc" / "kv_widen.h").read_text()
    assert ";;#ASMSTART" not in asm and "asm" not in src.replace("assembly", "")
    assert "global_load_dwordx4" in asm and "global_store_dwordx4" in asm and "global_load_dwordx2" in asm
    assert "ds_write" not in asm and "ds_read" not in asm and "scratch_" not in asm  # no LDS, no scratch
