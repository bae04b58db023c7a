"""-m "not gpu": fp8 (e4m3fn) unique K/V caches -- the additive C ABI (hyd_kv_quant, hyd_*_kvq, hyd_kv_quant_supported), the
quantizer every kernel matches (hydragen_amd/kv_quant.py) against an independent numpy rounding, the error the quantization
costs attention (float64 oracle), and the register budget of the new kernels."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd._lib import KvQuant, SuffixParams
from hydragen_amd.kv_quant import dequantize_kv, quantize_kv
from oracle import hydragen_oracle as O

REPO = Path(__file__).resolve().parent.parent
NEW = {"hyd_suffix_attn_fwd_kvq", "hyd_decode_attn_fused_kvq", "hyd_rope_append_decode_kvq", "hyd_kv_quant_supported"}


def test_new_symbols_exported_and_declared():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name)
    assert "HYD_FP8_E4M3 = 3" in header and _lib.HYD_FP8_E4M3 == 3
    assert lib.hyd_version() == 500  # additive: the version stays


def test_struct_sizes_gcc_vs_ctypes_and_unchanged():
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
           'sizeof(hyd_kv_quant), sizeof(hyd_prefix_params), sizeof(hyd_partial), sizeof(hyd_suffix_params), sizeof(hyd_level),'
           'sizeof(hyd_decode_params), sizeof(hyd_rope_params), sizeof(hyd_add_rmsnorm_params), sizeof(hyd_swiglu_params),'
           'sizeof(hyd_sample_params));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        sizes = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert sizes[0] == C.sizeof(KvQuant) == 24
    # the nine existing structs keep the sizes of ABI 0.5.0
    assert sizes[1:] == [176, 24, 344, 80, 1024, 208, 96, 64, 56]


def _sp(B=1024, nq=1, Hq=32, Hkv=32, D=128, S=64, dtype=_lib.HYD_BF16):
    p = SuffixParams()
    p.dtype, p.B, p.nq, p.Hq, p.Hkv, p.D, p.kv_len = dtype, B, nq, Hq, Hkv, D, S
    p.k_head_stride = p.v_head_stride = D
    p.k_tok_stride = p.v_tok_stride = Hkv * D
    p.k_batch_stride = p.v_batch_stride = S * Hkv * D
    return p


def _kq(kv_dtype=_lib.HYD_FP8_E4M3):
    kq = KvQuant()
    kq.kv_dtype = kv_dtype
    return kq


@pytest.mark.parametrize("shape, native", [
    (dict(Hq=32, Hkv=32, D=128), True),   # C2
    (dict(Hq=4, Hkv=4, D=128), True),     # the heads of one wave instruction (token split), TP = 8 shard
    (dict(Hq=8, Hkv=8, D=64), True),
    (dict(Hq=16, Hkv=16, D=64), True),
    (dict(Hq=2, Hkv=2, D=256), True),
    (dict(Hq=32, Hkv=32, D=256), True),
    (dict(Hq=32, Hkv=8, D=128), False),   # grouped-query heads
    (dict(Hq=32, Hkv=32, D=128, nq=2), False),
    (dict(Hq=32, Hkv=32, D=96), False),
    (dict(Hq=2, Hkv=2, D=128), False),    # fewer heads than one wave instruction covers
    (dict(Hq=6, Hkv=6, D=128), False),
])
def test_kv_quant_supported_truth_table(shape, native):
    lib = _lib.load()
    p = _sp(**shape)
    assert lib.hyd_kv_quant_supported(C.byref(p), C.byref(_kq())) == int(native)
    # no quantization: always "supported" (the existing entry point decides)
    assert lib.hyd_kv_quant_supported(C.byref(p), None) == 1
    assert lib.hyd_kv_quant_supported(C.byref(p), C.byref(_kq(p.dtype))) == 1


def test_kv_quant_supported_counts_one_byte_elements():
    lib = _lib.load()
    # a sequence spanning 1.5 GiB of fp8 (3 GiB as 16-bit) stays native: offsets are counted in bytes
    S = (3 << 29) // (32 * 128)
    assert lib.hyd_kv_quant_supported(C.byref(_sp(B=2, S=S)), C.byref(_kq())) == 1
    assert lib.hyd_kv_quant_supported(C.byref(_sp(B=2, S=2 * S)), C.byref(_kq())) == 0


def test_kvq_argument_validation():
    lib = _lib.load()
    err = lambda: lib.hyd_last_error_string().decode()  # noqa: E731
    p = _sp()
    p.q = p.out = p.k = p.v = 4096  # never dereferenced: validation fails first
    assert lib.hyd_suffix_attn_fwd_kvq(C.byref(p), C.byref(_kq(7)), None) == -2 and "kv_dtype 7" in err()
    assert lib.hyd_rope_append_decode_kvq(C.byref(_lib.RopeParams(dtype=1, B=1, Hq=4, Hkv=4, D=128)), C.byref(_kq(7)), None) == -2
    assert "kv_dtype 7" in err()
    d = _lib.DecodeParams()
    d.suffix = p
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(_kq(9)), None) == -2 and "kv_dtype 9" in err()
    # fp8 queries are not a thing: q stays 16-bit
    p8 = _sp(dtype=_lib.HYD_FP8_E4M3)
    p8.q = p8.out = p8.k = p8.v = 4096
    assert lib.hyd_suffix_attn_fwd_kvq(C.byref(p8), C.byref(_kq()), None) == -2 and "dtype 3" in err()
    # non-native shapes are refused before any launch
    g = _sp(Hkv=8)
    g.q = g.out = g.k = g.v = 4096
    assert lib.hyd_suffix_attn_fwd_kvq(C.byref(g), C.byref(_kq()), None) == -2 and "not native" in err()
    d.suffix = g
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(_kq()), None) == -2 and "not native" in err()


@pytest.mark.parametrize("kq", [None, "same"])
def test_kvq_without_quantization_is_the_existing_entry_point(kq):
    lib = _lib.load()
    p = _sp(D=96)  # rejected by the existing entry point's validation: same code, same message
    p.q = p.out = p.k = p.v = 4096
    k = None if kq is None else C.byref(_kq(p.dtype))
    rc0 = lib.hyd_suffix_attn_fwd(C.byref(p), None)
    m0 = lib.hyd_last_error_string().decode()
    assert lib.hyd_suffix_attn_fwd_kvq(C.byref(p), k, None) == rc0 == -2
    assert lib.hyd_last_error_string().decode() == m0
    d = _lib.DecodeParams()
    d.suffix = p
    rc0 = lib.hyd_decode_attn_fused(C.byref(d), None)
    m0 = lib.hyd_last_error_string().decode()
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), k, None) == rc0 and lib.hyd_last_error_string().decode() == m0
    r = _lib.RopeParams(dtype=1, B=1, Hq=4, Hkv=4, D=128)  # null pointers
    rc0 = lib.hyd_rope_append_decode(C.byref(r), None)
    m0 = lib.hyd_last_error_string().decode()
    assert lib.hyd_rope_append_decode_kvq(C.byref(r), k, None) == rc0 == -1 and lib.hyd_last_error_string().decode() == m0


# ---- the quantizer against an independent rounding ----------------------------------------------------------------------
def _e4m3_values():
    """The 127 non-negative finite e4m3fn values, by code (0x00 .. 0x7e)."""
    vals = []
    for c in range(0x7F):
        e, m = c >> 3, c & 7
        vals.append(m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return np.array(vals)


def _np_quant_bits(x):
    """Round-to-nearest, ties to even code (= even mantissa), saturating at 448; NaN -> 0x7f | sign."""
    vals = _e4m3_values()
    x = np.asarray(x, dtype=np.float64)
    sign = np.signbit(x).astype(np.uint8) << 7
    a = np.minimum(np.abs(x), 448.0)
    i = np.clip(np.searchsorted(vals, a), 1, 126)
    lo, hi = vals[i - 1], vals[i]
    pick_hi = (hi - a < a - lo) | ((hi - a == a - lo) & (i % 2 == 0))
    code = np.where(a >= vals[126], 126, np.where(a <= 0, 0, np.where(pick_hi, i, i - 1)))
    code = np.where(np.isnan(x), 0x7F, code)
    return (code.astype(np.uint8) | sign).astype(np.uint8)


def _bits(t):
    return t.view(torch.uint8).numpy()


def test_quantize_matches_independent_rounding():
    rng = np.random.default_rng(0)
    vals = _e4m3_values()
    mids = (vals[1:] + vals[:-1]) / 2  # exact ties between neighbours: half to the even code
    x = np.concatenate([rng.standard_normal(20000) * s for s in (1e-3, 0.1, 1, 30, 300)] +
                       [vals, -vals, mids, -mids, [447, 449, 464, 500, 1e6, -1e6, np.inf, -np.inf]]).astype(np.float32)
    got = _bits(quantize_kv(torch.from_numpy(x).reshape(-1, 1, 1)).reshape(-1))
    want = _np_quant_bits(x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


def test_quantize_saturates_per_head_scale_and_round_trips():
    scale = torch.tensor([1.0, 0.5, 4.0], dtype=torch.float32)
    x = torch.tensor([[448.0, 2000.0, -2000.0], [224.0, 300.0, -300.0], [1792.0, 1e9, -1e9]]).reshape(1, 3, 3)  # [1, H, D]
    q8 = quantize_kv(x, scale)
    back = dequantize_kv(q8, scale, torch.float32)
    # saturation at +-448 * scale[h]; 448 * scale[h] itself is exact
    assert torch.equal(back[0, :, 1], 448 * scale) and torch.equal(back[0, :, 2], -448 * scale)
    assert torch.equal(back[0, :, 0], 448 * scale)
    # every representable value (times its head's scale) survives a round trip exactly, in bf16 and f16
    vals = torch.from_numpy(np.concatenate([_e4m3_values(), -_e4m3_values()[1:]])).float()
    for dt in (torch.bfloat16, torch.float16):
        y = (vals[:, None] * scale[None, :]).reshape(-1, 3, 1).to(dt)
        assert torch.equal(dequantize_kv(quantize_kv(y, scale), scale, dt), y)
    # NaN passes through (the clamp keeps it)
    n = quantize_kv(torch.tensor([float("nan"), 1.0]).reshape(2, 1, 1))
    assert torch.isnan(n.float()[0]).all() and n.float()[1].item() == 1.0
    with pytest.raises(ValueError):
        quantize_kv(x, torch.ones(2))


# ---- the error the quantization costs attention ---------------------------------------------------------------------------
# relative L2 of attention on fp8 K / V (scale 1) against float64 attention on the raw (unit-normal) inputs.  Measured with this
# test's seeds: 3.4-4.0e-2 over D 64 / 128 / 256 and S 8 ... 1024; K std 3 (sharper softmax): 4.3-7.0e-2.  The bound tells
# users what they trade: 8e-2.
FP8_REL_L2_BOUND = 8e-2


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("S", [8, 128, 1024])
@pytest.mark.parametrize("kstd", [1.0, 3.0])
def test_quantization_error_budget(D, S, kstd):
    rng = np.random.default_rng(D * 7 + S + int(kstd))
    B, H = 2, 2
    q = rng.standard_normal((B, 1, H, D)).astype(np.float32)
    k = (rng.standard_normal((B, S, H, D)) * kstd).astype(np.float32)
    v = rng.standard_normal((B, S, H, D)).astype(np.float32)
    k8 = quantize_kv(torch.from_numpy(k)).float().numpy()
    v8 = quantize_kv(torch.from_numpy(v)).float().numpy()
    want, _ = O.flash_attention_seqlen(q, k, v, None)
    got, _ = O.flash_attention_seqlen(q, k8, v8, None)
    l2 = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert 1e-3 < l2 <= FP8_REL_L2_BOUND, l2


# ---- the new kernels' registers ---------------------------------------------------------------------------------------------
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
@pytest.mark.parametrize("src, pat, count", [("suffix_attn_fp8.hip", r"suffix_attn_rows_fp8_kernel", 24),
                                             ("rope_append.hip", r"rope_append_fp8_kernel", 6)])
def test_fp8_kernels_have_no_scratch_and_keep_four_waves(src, pat, count):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                          str(REPO / "hydragen_amd" / "csrc" / src), "-o", "-"], capture_output=True, text=True, check=True).stdout
    seen = 0
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if not re.search(pat, name):
            continue
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spill == 0 and scratch == 0 and vgpr <= 128, (name, vgpr, spill, scratch)
    assert seen == count  # {bf16, f16} x D {64, 128, 256} x (suffix: NPRE 2, token split 4 / 2 / 1)
    # the K / V bytes arrive as 8-byte requests and are widened by the native gfx950 conversions
    if src == "suffix_attn_fp8.hip":
        for ins in ("global_load_dwordx2", "v_cvt_pk_f32_fp8", "v_cvt_scalef32_pk_bf16_fp8", "v_cvt_scalef32_pk_f16_fp8"):
            assert ins in out, ins
    else:
        assert "v_cvt_pk_fp8_f32" in out
