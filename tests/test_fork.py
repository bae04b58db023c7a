"""-m "not gpu": fork completions (hydragen_amd/fork.py, hyd_kv_promote) -- the ABI bookkeeping of the new entry point, its refusals
(they run before any launch, so they need no device), the host rules (check_fork_rows, select_beams), the torch definition of the
copy on CPU tensors, and the register metadata of the new kernel."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd.fork import check_fork_rows, promote_kv_reference, select_beams
from hydragen_amd.kv_quant import FP8_DTYPE, dequantize_kv

REPO = Path(__file__).resolve().parent.parent
PTR = 0x7F0000001000  # never dereferenced on the host: the entry point only checks null / alignment


def test_header_exports_and_library_agree_on_the_entry_point():
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    assert re.search(r"HYD_API int hyd_kv_promote\(const hyd_kv_promote_params\* p, void\* stream\);", header)
    assert "typedef struct hyd_kv_promote_params" in header
    assert "hyd_kv_promote" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "hyd_kv_promote")
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(_lib.lib_path())], text=True)
    assert any(ln.split()[-1] == "hyd_kv_promote" and " T " in ln for ln in out.splitlines())
    assert lib.hyd_version() == 500  # new symbols only: no existing struct changed
    assert "kv_promote.hip" in (REPO / "hydragen_amd" / "csrc" / "build.py").read_text()


def test_struct_layout_matches_c():
    """The ctypes mirror has the size gcc gives the C struct, and the fields sit where gcc puts them."""
    names = [n for n, _ in _lib.KvPromoteParams._fields_]
    offs = "".join(f'printf("%zu ", offsetof(hyd_kv_promote_params, {n}));' for n in names)
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu ", sizeof(hyd_kv_promote_params));'
           + offs + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got[0] == C.sizeof(_lib.KvPromoteParams)
    assert got[1:] == [getattr(_lib.KvPromoteParams, n).offset for n in names]


def _params(**kw):
    p = _lib.KvPromoteParams()
    p.k_src = p.v_src = p.k_dst = p.v_dst = p.rows = p.lens = p.cu = PTR
    p.k_batch_stride = p.v_batch_stride = 2 * 48 * 8 * 128
    p.k_tok_stride = p.v_tok_stride = 8 * 128
    p.k_head_stride = p.v_head_stride = 128
    p.src_dtype = p.dst_dtype = _lib.HYD_BF16
    p.n, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst, p.capacity = 4, 6, 48, 8, 128, 128, 4 * 48
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,code,frag", [
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
    (dict(cu=None), -1, "cu"),
    (dict(src_dtype=_lib.HYD_F16), -1, "src_dtype"),
    (dict(src_dtype=_lib.HYD_F32), -2, "src_dtype"),
    (dict(d_src=80, d_dst=96), -2, "d_dst"),
    (dict(k_tok_stride=8 * 128 + 4), -1, "k_tok_stride"),
    (dict(v_src=PTR + 8), -1, "v_src"),
    (dict(max_len=49), -1, "max_len"),
    (dict(n=70000), -2, "n 70000"),
])
def test_refusals_come_before_any_launch_and_name_the_field(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_kv_promote(C.byref(_params(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode(), lib.hyd_last_error_string().decode()


def test_null_params_and_valid_parameters_without_a_device():
    lib = _lib.load()
    assert lib.hyd_kv_promote(None, None) == -1
    if torch.cuda.is_available():
        return  # a device is present: a launch on made-up pointers is not issued
    # every accepted form reaches the launch, which fails cleanly without a device (HYD_ERR_LAUNCH), it does not crash
    for kw in (dict(), dict(d_src=80, d_dst=128), dict(d_src=80, d_dst=80), dict(src_dtype=_lib.HYD_FP8_E4M3),
               dict(src_dtype=_lib.HYD_FP8_E4M3, dst_dtype=_lib.HYD_F16, k_scale=PTR, v_scale=PTR), dict(max_len=17),
               dict(src_dtype=_lib.HYD_F16, dst_dtype=_lib.HYD_F16, Hkv=1, d_src=64, d_dst=64)):
        assert lib.hyd_kv_promote(C.byref(_params(**kw)), None) == -4, kw
        assert "kv_promote" in lib.hyd_last_error_string().decode()


# ---- check_fork_rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,old,levels", [
    ([3, 0, 2], 4, []),                       # no level: any distinct rows
    ([5, 0, 3], 6, [1]),                      # one level of 1: any distinct rows
    ([1, 3, 4, 6], 8, [1, 2]),
    ([3, 1, 6, 4], 8, [1, 2]),                # any order within a group
    ([0, 1, 2, 3, 4, 5, 6, 7], 8, [1, 2, 4]),
    ([1, 2, 5, 6], 8, [1, 2, 4]),
])
def test_check_fork_rows_accepts_regular_forks(rows, old, levels):
    check_fork_rows(rows, old, levels)
    check_fork_rows(torch.tensor(rows), old, levels)


@pytest.mark.parametrize("rows,old,levels,frag", [
    ([1, 2, 3, 6], 8, [1, 2], r"level 1: rows\[2\] = 3"),       # 3 + 1 survivors per group
    ([4, 6, 1, 3], 8, [1, 2], r"level 1: rows\[0\] = 4"),       # group order
    ([1, 4, 6], 8, [1, 2], r"level 1: 3 rows"),                 # k no multiple of the level's batch
    ([1, 3, 3, 6], 8, [1, 2], r"rows\[2\] = 3 repeats rows\[1\]"),
    ([1, 8], 8, [1], r"rows\[1\] = 8"),
    ([-1, 2], 8, [1], r"rows\[0\] = -1"),
    ([0, 1], 8, [3], r"level 0: 3 shared sequences"),
    ([], 8, [1], "no rows"),
])
def test_check_fork_rows_refuses_and_names_level_and_index(rows, old, levels, frag):
    with pytest.raises(ValueError, match=frag):
        check_fork_rows(rows, old, levels)


# ---- select_beams ------------------------------------------------------------------------------------
def _brute_beams(scores, group_size, width):
    out = []
    for g in range(len(scores) // group_size):
        idx = list(range(g * group_size, (g + 1) * group_size))
        idx.sort(key=lambda i: (-scores[i], i))  # descending score, ties to the lower row index
        out += idx[:width]
    return out


@pytest.mark.parametrize("G,group,width", [(1, 6, 2), (2, 6, 2), (3, 5, 5), (4, 7, 1), (2, 1, 1)])
def test_select_beams_matches_brute_force(G, group, width):
    g = torch.Generator().manual_seed(G * 100 + group)
    for ties in (False, True):
        s = torch.randn(G * group, generator=g)
        if ties:
            s = torch.randint(0, 3, (G * group,), generator=g).float()  # three values: many ties in every group
        rows = select_beams(s, group, width)
        assert rows.dtype == torch.int64 and rows.tolist() == _brute_beams(s.tolist(), group, width)
        assert select_beams(s.tolist(), group, width).tolist() == rows.tolist()  # host scores
        check_fork_rows(rows.tolist(), G * group, [1, G])
    with pytest.raises(ValueError, match="width"):
        select_beams(torch.zeros(G * group), group, group + 1)
    with pytest.raises(ValueError, match="group_size"):
        select_beams(torch.zeros(7), 3, 1)


# ---- promote_kv_reference on CPU tensors --------------------------------------------------------------
def _arena(B, rows, Hkv, d, dtype, seed):
    from hydragen_amd import placement

    arena = placement.kv_arena((B, rows, Hkv, d), dtype, "cpu", zero=True)
    g = torch.Generator().manual_seed(seed)
    if dtype == FP8_DTYPE:
        arena.view(torch.uint8).copy_(torch.randint(0, 256, tuple(arena.shape), dtype=torch.uint8, generator=g))
    else:
        arena.copy_(torch.randn(tuple(arena.shape), generator=g).to(dtype))
    return arena[0], arena[1]


def _expect(src, rows, lens, scale, dtype, D):
    x = src if src.dtype != FP8_DTYPE else dequantize_kv(src, scale, dtype)
    tok = torch.cat([x[r, :n] for r, n in zip(rows, lens)], dim=0)
    return torch.nn.functional.pad(tok, (0, D - tok.shape[-1]))


@pytest.mark.parametrize("dtype,src_dtype,Hkv,d,D,lens", [
    (torch.bfloat16, torch.bfloat16, 4, 64, 64, [1, 15, 16, 17]),
    (torch.float16, torch.float16, 2, 128, 128, [48, 1, 17, 16]),
    (torch.bfloat16, torch.bfloat16, 8, 80, 128, [17, 17, 17, 17]),   # the narrow widening, all lengths equal
    (torch.bfloat16, torch.bfloat16, 8, 80, 128, [15, 48, 1, 16]),
    (torch.bfloat16, FP8_DTYPE, 8, 64, 64, [16, 1, 48, 15]),
    (torch.float16, FP8_DTYPE, 8, 128, 128, [17, 15, 1, 16]),
])
def test_promote_kv_reference_on_cpu(dtype, src_dtype, Hkv, d, D, lens):
    B, R, rows = 6, 48, [4, 0, 5, 2]   # a permuted subset of the rows
    k, v = _arena(B, R, Hkv, d, src_dtype, 3)
    assert k.stride(0) == 2 * R * Hkv * d   # views of the arena: the batch stride is not rows * Hkv * d
    fp8 = src_dtype == FP8_DTYPE
    ks = (torch.arange(Hkv).float() * 0.37 + 0.11) if fp8 else None
    vs = (torch.arange(Hkv).float() * 0.05 + 1.3) if fp8 else None
    cap = sum(lens) + 5
    sentinel = torch.full((cap, Hkv, D), 7.0, dtype=dtype)
    kd, vd = sentinel.clone(), sentinel.clone()
    cu = promote_kv_reference(k, v, torch.tensor(rows), torch.tensor(lens), kd, vd, **(dict(k_scale=ks, v_scale=vs) if fp8 else {}))
    assert cu.dtype == torch.int32 and cu.tolist() == [0] + torch.tensor(lens).cumsum(0).tolist()
    total = sum(lens)
    as_bits = lambda t: t.view(torch.int16)
    for src, dst, scale in ((k, kd, ks), (v, vd, vs)):
        want = _expect(src, rows, lens, scale, dtype, D)
        nan = want.isnan()
        assert torch.equal(dst[:total].isnan(), nan)
        assert torch.equal(as_bits(dst[:total])[~nan], as_bits(want)[~nan])
        assert not dst[:total, :, d:].any()                       # pad columns are zero
        assert torch.equal(dst[total:], sentinel[total:])          # rows past the total are untouched
    with pytest.raises(ValueError):
        promote_kv_reference(k, v, torch.tensor([0, 6]), torch.tensor([1, 1]), kd, vd)
    with pytest.raises(ValueError):
        promote_kv_reference(k, v, torch.tensor([0, 1]), torch.tensor([1, R + 1]), kd, vd)
    if not fp8:
        with pytest.raises(ValueError, match="dtype"):
            other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
            promote_kv_reference(k, v, torch.tensor(rows), torch.tensor(lens), kd.to(other), vd.to(other))


def test_promote_unique_leaves_the_level_as_fill_would():
    """PerLayerKVCache.promote_unique through the torch route on CPU: the level's buffers and flags equal those SharedCache.fill
    leaves for the same data, and its errors are fill's / append_shared's."""
    from hydragen_amd.llama import PerLayerKVCache

    def cache():
        c = PerLayerKVCache(6, 16, [1, 3], [8, 12], 8, 80, "cpu", torch.bfloat16)
        g = torch.Generator().manual_seed(1)
        c.per_completion_k_cache.copy_(torch.randn(6, 16, 8, 80, generator=g).to(torch.bfloat16))
        c.per_completion_v_cache.copy_(torch.randn(6, 16, 8, 80, generator=g).to(torch.bfloat16))
        c.append_shared(torch.zeros(1, 8, 8, 80, dtype=torch.bfloat16), torch.zeros(1, 8, 8, 80, dtype=torch.bfloat16), torch.tensor([8]))
        return c

    for lens in ([5, 12, 7], [9, 9, 9]):
        a, b = cache(), cache()
        rows = [5, 0, 3]
        a.promote_unique(torch.tensor(rows, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32), lens, use_kernel=False)
        b.append_shared(b.per_completion_k_cache[rows, :12], b.per_completion_v_cache[rows, :12], torch.tensor(lens))
        sa, sb = a.shared_caches[1], b.shared_caches[1]
        assert a.num_used_shared_caches == b.num_used_shared_caches == 2
        for name in ("k_cache", "v_cache", "seq_lens", "cumsum_lengths"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), name
        assert (sa.use_varlen, sa.sliced_sequence_length, sa.current_batch_size) == (sb.use_varlen, sb.sliced_sequence_length, sb.current_batch_size)
    c = cache()
    t = lambda x: torch.tensor(x, dtype=torch.int32)
    with pytest.raises(ValueError, match="Batch size 4 exceeds"):
        c.promote_unique(t([0, 1, 2, 3]), t([1, 1, 1, 1]), [1, 1, 1, 1], use_kernel=False)
    with pytest.raises(ValueError, match="Sequence length 13 exceeds"):
        c.promote_unique(t([0, 1, 2]), t([1, 13, 1]), [1, 13, 1], use_kernel=False)
    assert c.num_used_shared_caches == 1
    c.promote_unique(t([0, 1, 2]), t([1, 2, 3]), [1, 2, 3], use_kernel=False)
    with pytest.raises(ValueError, match="No more available shared caches"):
        c.promote_unique(t([0, 1, 2]), t([1, 2, 3]), [1, 2, 3], use_kernel=False)


@pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")
def test_promote_kernel_has_no_scratch_and_names_no_register_by_hand():
    """Every instantiation (16-bit byte copy, fp8 -> f16, fp8 -> bf16): private segment size 0, nothing spilled; 16-byte vector
    loads and stores; and no hand-written assembly in the source."""
    from tests.test_build_quality import _device_asm, _metadata

    _, kernels = _metadata("kv_promote.hip")
    assert len(kernels) == 3 and all("kv_promote_kernel" in k["name"] for k in kernels), [k["name"] for k in kernels]
    for k in kernels:
        assert k["scratch"] == 0 and k["spill"] == 0 and k["sspill"] == 0 and k["vgpr"] <= 128, k
    asm = _device_asm("kv_promote.hip")
    assert ";;#ASMSTART" not in asm and "asm" not in (REPO / "hydragen_amd" / "csrc" / "kv_promote.hip").read_text().replace("assembly", "")
    assert "global_load_dwordx4" in asm and "global_store_dwordx4" in asm and "global_load_dwordx2" in asm
    assert "ds_write" not in asm and "ds_read" not in asm  # no LDS
