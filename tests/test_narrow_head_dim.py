"""-m "not gpu": narrow unique K/V caches (head dims 80 / 96 / 192 ... kept at their true width, include/hydragen_hip.h:
hyd_suffix_params.kv_dim, hyd_rope_params.head_dim, hyd_narrow_kv_supported) -- the host side: the export, the shapes-only
answers, the refusals with their messages, the register budget of the new kernel instantiations, and the cache layout the model
shell chooses.  No compute calls."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd._lib import DecodeParams, KvQuant, RopeParams, SuffixParams

REPO = Path(__file__).resolve().parent.parent
PTR = 0x10000


def _suffix(d, D, Hq, Hkv, nq, rows=32, B=4):
    p = SuffixParams()
    p.dtype, p.B, p.nq, p.Hq, p.Hkv, p.D, p.kv_len = _lib.HYD_BF16, B, nq, Hq, Hkv, D, rows
    p.kv_dim = d
    p.k_head_stride = p.v_head_stride = d
    p.k_tok_stride = p.v_tok_stride = Hkv * d
    p.k_batch_stride = p.v_batch_stride = rows * Hkv * d
    p.q = p.k = p.v = p.out = PTR
    return p


def test_export_and_struct_layout():
    lib = _lib.load()
    assert "hyd_narrow_kv_supported" in _lib.EXPORTS and hasattr(lib, "hyd_narrow_kv_supported")
    assert lib.hyd_version() == 500
    # kv_dim / head_dim took the place of the reserved words: same offsets, same sizes as the C compiler's
    src = ('#include "hydragen_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n", '
           'sizeof(hyd_suffix_params), sizeof(hyd_rope_params), sizeof(hyd_decode_params), offsetof(hyd_suffix_params, kv_dim), '
           'offsetof(hyd_rope_params, head_dim));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got == [C.sizeof(SuffixParams), C.sizeof(RopeParams), C.sizeof(DecodeParams), SuffixParams.kv_dim.offset,
                   RopeParams.head_dim.offset]
    # ... and as before the fields had names: 8 pointers, 6 strides, 10 words, 8 partials of 24 bytes; 11 pointers, 11 strides, 8 words
    assert C.sizeof(SuffixParams) == 8 * 8 + 6 * 8 + 10 * 4 + 8 * 24 and C.sizeof(RopeParams) == 11 * 8 + 11 * 8 + 8 * 4


YES = [(96, 128, 8, 8, 1), (80, 128, 4, 4, 1), (48, 64, 8, 8, 1), (192, 256, 2, 2, 1)]
NO = [(96, 128, 8, 2, 1), (96, 128, 8, 8, 2), (96, 128, 6, 6, 1), (72, 128, 8, 8, 1)]


@pytest.mark.parametrize("shape", YES + NO)
def test_narrow_kv_supported_answers(shape):
    """(d, D, Hq, Hkv, nq): yes exactly for one query row, Hq == Hkv, whole lane groups (64 / (D / 8) heads) and d % 16 == 0; the
    launch entry points refuse what the query refuses, before touching the device."""
    lib = _lib.load()
    p = _suffix(*shape)
    want = 1 if shape in YES else 0
    assert lib.hyd_narrow_kv_supported(C.byref(p)) == want
    if not want:
        code = -1 if shape[0] % 16 else -2  # a bad kv_dim is a bad argument, a shape without a narrow kernel is unsupported
        assert lib.hyd_suffix_attn_fwd(C.byref(p), None) == code
        assert "kv_dim" in lib.hyd_last_error_string().decode()
        d = DecodeParams()
        d.suffix = p
        d.n_levels = 1
        d.levels[0].sb, d.levels[0].kv_len = 1, 64
        d.levels[0].k = d.levels[0].v = PTR
        assert lib.hyd_decode_attn_fused(C.byref(d), None) == code
        assert "kv_dim" in lib.hyd_last_error_string().decode()
    # kv_dim 0 and kv_dim == D are the existing call: always taken
    for same in (0, shape[1]):
        p.kv_dim = same
        assert lib.hyd_narrow_kv_supported(C.byref(p)) == 1


def test_fp8_caches_have_no_narrow_form():
    lib = _lib.load()
    p = _suffix(96, 128, 8, 8, 1)
    kq = KvQuant()
    kq.kv_dtype, kq.flags = _lib.HYD_FP8_E4M3, _lib.HYD_KVQ_GQA
    assert lib.hyd_kv_quant_supported(C.byref(p), C.byref(kq)) == 0
    assert lib.hyd_suffix_attn_fwd_kvq(C.byref(p), C.byref(kq), None) == -2
    assert "fp8" in lib.hyd_last_error_string().decode() and "kv_dim" in lib.hyd_last_error_string().decode()
    d = DecodeParams()
    d.suffix = p
    d.n_levels = 1
    d.levels[0].sb, d.levels[0].kv_len = 1, 64
    d.levels[0].k = d.levels[0].v = PTR
    assert lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(kq)) == 0
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(kq), None) == -2
    r = _rope(96, 128)
    assert lib.hyd_rope_append_decode_kvq(C.byref(r), C.byref(kq), None) == -2
    assert "fp8" in lib.hyd_last_error_string().decode()


def _rope(head_dim, D):
    r = RopeParams()
    r.q = r.k = r.v = r.q_out = r.k_cache = r.v_cache = r.cos = r.sin = r.position_ids = r.seq_lens = PTR
    r.dtype, r.B, r.Hq, r.Hkv, r.D, r.cache_len, r.max_pos = _lib.HYD_BF16, 2, 8, 8, D, 16, 64
    r.head_dim = head_dim
    r.cs_stride = head_dim or D
    return r


@pytest.mark.parametrize("bad", [8, 100, 144, 256, -16])
def test_bad_narrow_dims_are_bad_arguments_that_name_the_field(bad):
    """kv_dim / head_dim: 0 or D, or a multiple of 16 in [16, D) (D = 128 here: 8 is too small, 100 no multiple of 16, 144 and 256
    are beyond D)."""
    lib = _lib.load()
    p = _suffix(bad, 128, 8, 8, 1)
    assert lib.hyd_narrow_kv_supported(C.byref(p)) == 0
    assert lib.hyd_suffix_attn_fwd(C.byref(p), None) == -1
    msg = lib.hyd_last_error_string().decode()
    assert "kv_dim" in msg and str(bad) in msg
    d = DecodeParams()
    d.suffix = p
    assert lib.hyd_decode_attn_fused(C.byref(d), None) == -1 and "kv_dim" in lib.hyd_last_error_string().decode()
    assert lib.hyd_rope_append_decode(C.byref(_rope(bad, 128)), None) == -1
    msg = lib.hyd_last_error_string().decode()
    assert "head_dim" in msg and str(bad) in msg


@pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")
def test_new_instantiations_keep_the_register_budget():
    """The narrow token-row instantiations (the template's last argument true) and the narrow RoPE + append kernel: at most 128
    VGPRs (4 waves per SIMD, the D-wide kernel's occupancy), nothing spilled, no scratch -- read from the assembly's metadata the
    way tests/test_build_quality.py reads it (the same per-session compile)."""
    from tests.test_build_quality import _metadata

    _, kernels = _metadata("suffix_attn.hip")
    narrow = [k for k in kernels if "suffix_attn_rows_kernel" in k["name"] and k["name"].endswith("Lb1EEEvNS_10SuffixArgsE")]
    # {f16, bf16} x {64, 128, 256} x {(NPRE, TS) = (1, 1), (1, 2), (1, 4), (2, 1)}
    assert len(narrow) == 24, [k["name"] for k in narrow]
    wide = [k for k in kernels if "suffix_attn_rows_kernel" in k["name"] and k["name"].endswith("Lb0EEEvNS_10SuffixArgsE")]
    assert len(wide) == 24
    _, rope = _metadata("rope_append.hip")
    rope_narrow = [k for k in rope if "rope_append_narrow_kernel" in k["name"]]
    assert len(rope_narrow) == 2, [k["name"] for k in rope]
    for k in narrow + rope_narrow:
        assert k["vgpr"] <= 128 and k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k


def test_cache_widths_of_the_model_shell():
    """Unique rows at the true head dim, shared caches (zero-initialised) at the kernels' -- only where the shapes qualify."""
    from hydragen_amd.llama import PerLayerKVCache, narrow_kv_head_dim

    c = PerLayerKVCache(4, 16, [1, 2], [16, 8], 4, 96, "cpu", torch.bfloat16)
    assert c.narrow and c.per_completion_k_cache.shape == (4, 16, 4, 96) and c.per_completion_v_cache.shape[-1] == 96
    for sc in c.shared_caches:
        assert sc.k_cache.shape[-1] == 128 and sc.v_cache.shape[-1] == 128 and not sc.k_cache.any()
    # fill writes the leading columns, the pad columns stay zero; copy_shared_to_unique reads them back
    k = torch.randn(1, 16, 4, 96).to(torch.bfloat16)
    c.append_shared(k, -k, torch.tensor([16]))
    sc = c.shared_caches[0]
    assert torch.equal(sc.k_cache[:16, :, :96], k[0]) and torch.equal(sc.v_cache[:16, :, :96], -k[0]) and not sc.k_cache[..., 96:].any()
    c.copy_shared_to_unique(4)
    assert torch.equal(c.per_completion_k_cache[3], k[0]) and torch.equal(c.per_completion_v_cache[0], -k[0])
    # shapes that do not qualify keep every tensor at the model's head dim, as always
    for kw, args in ((dict(), (2, 96)), (dict(n_q_heads=8), (4, 96)), (dict(), (4, 72)), (dict(), (4, 128)),
                     (dict(kv_cache_dtype=torch.float8_e4m3fn), (4, 96))):
        o = PerLayerKVCache(4, 16, [1], [16], *args, "cpu", torch.bfloat16, **kw)
        assert not o.narrow and o.shared_caches[0].k_cache.shape[-1] == args[1] and o.per_completion_k_cache.shape[-1] == args[1]
    assert [narrow_kv_head_dim(d, h) for d, h in ((96, 4), (80, 32), (48, 8), (192, 2), (192, 3), (96, 6), (100, 4), (128, 4))] == \
        [128, 128, 64, 256, 0, 0, 0, 0]
