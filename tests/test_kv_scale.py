"""-m "not gpu": calibrated fp8 K/V scales -- the additive C ABI (hyd_kv_absmax, hyd_kv_scales_from_absmax), what the entry points
refuse, the scale rule's definition in torch (hydragen_amd/kv_quant.py), its power-of-two equivariance, the attention error
budget with calibrated against unit scales (float64 oracle), and the new kernels' scratch use."""
import ctypes as C
import math
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd import kv_quant as Q
from hydragen_amd._lib import KvAbsmaxParams, KvScalesParams
from tests import kv_scale_cases as cases
from tests.test_fp8_kv import FP8_REL_L2_BOUND

REPO = Path(__file__).resolve().parent.parent
NEW = {"hyd_kv_absmax", "hyd_kv_scales_from_absmax"}
PTR = 0x10000  # aligned, never dereferenced: every refusal comes before a launch


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_declared():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name)
    assert declared == set(_lib.EXPORTS)
    assert f"#define HYD_KV_ABSMAX_PASSES {_lib.KV_ABSMAX_PASSES}\n" in header
    assert lib.hyd_version() == 500 == _lib.ABI_VERSION  # additive: the version stays


def test_struct_sizes_gcc_vs_ctypes():
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
           'sizeof(hyd_kv_absmax_params), sizeof(hyd_kv_scales_params), offsetof(hyd_kv_absmax_params, dtype),'
           'offsetof(hyd_kv_absmax_params, n_rows), offsetof(hyd_kv_scales_params, c), offsetof(hyd_kv_scales_params, pow2));'
           'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got == [C.sizeof(KvAbsmaxParams), C.sizeof(KvScalesParams), KvAbsmaxParams.dtype.offset, KvAbsmaxParams.n_rows.offset,
                   KvScalesParams.c.offset, KvScalesParams.pow2.offset] == [104, 40, 80, 96, 28, 32]


# ---- validation -----------------------------------------------------------------------------------------------------------------
def _absmax(**kw):
    p = KvAbsmaxParams()
    p.k = p.v = p.amax = PTR
    p.dtype, p.Hkv, p.d, p.n_outer, p.n_rows = _lib.HYD_BF16, 4, 128, 2, 16
    p.k_head_stride = p.v_head_stride = 128
    p.k_row_stride = p.v_row_stride = 512
    p.k_outer_stride = p.v_outer_stride = 16 * 512
    for name, val in kw.items():
        setattr(p, name, val)
    return p


def _scales(**kw):
    p = KvScalesParams()
    p.amax = p.k_scale = p.v_scale = PTR
    p.Hkv, p.c, p.pow2 = 4, 2.0 / 448.0, 1
    for name, val in kw.items():
        setattr(p, name, val)
    return p


@pytest.mark.parametrize("kw, code, frag", [
    (dict(amax=None), -1, "amax is null"),
    (dict(k=None, v=None), -1, "k and v are both null"),
    (dict(d=12), -1, "d 12"),
    (dict(d=0), -1, "d 0"),
    (dict(d=264), -1, "d 264"),
    (dict(Hkv=0), -1, "Hkv 0"),
    (dict(n_outer=-1), -1, "n_outer -1"),
    (dict(n_rows=-1), -1, "n_rows -1"),
    (dict(dtype=_lib.HYD_F32), -2, "dtype 2"),
    (dict(dtype=_lib.HYD_FP8_E4M3), -2, "dtype 3"),
    (dict(k=PTR + 8), -1, "k must be 16-byte aligned"),
    (dict(v=PTR + 2), -1, "v must be 16-byte aligned"),
    (dict(amax=PTR + 2), -1, "amax / row_lens"),
    (dict(row_lens=PTR + 1), -1, "amax / row_lens"),
    (dict(k_outer_stride=4), -1, "k_outer_stride (4)"),
    (dict(k_row_stride=12), -1, "k_row_stride (12)"),
    (dict(k_head_stride=132), -1, "k_head_stride (132)"),
    (dict(v_outer_stride=4), -1, "v_outer_stride (4)"),
    (dict(v_row_stride=12), -1, "v_row_stride (12)"),
    (dict(v_head_stride=132), -1, "v_head_stride (132)"),
])
def test_absmax_refusals_name_the_field(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_kv_absmax(C.byref(_absmax(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


def test_absmax_null_params_and_zero_rows():
    lib = _lib.load()
    assert lib.hyd_kv_absmax(None, None) == -1 and "null params" in lib.hyd_last_error_string().decode()
    # nothing to read: a successful no-op, nothing is launched (these addresses are not memory)
    assert lib.hyd_kv_absmax(C.byref(_absmax(n_rows=0)), None) == 0
    assert lib.hyd_kv_absmax(C.byref(_absmax(n_outer=0)), None) == 0
    assert lib.hyd_kv_absmax(C.byref(_absmax(n_outer=0, n_rows=0, v=None)), None) == 0
    # ... but it is still validated
    assert lib.hyd_kv_absmax(C.byref(_absmax(n_rows=0, d=12)), None) == -1


@pytest.mark.parametrize("kw, frag", [
    (dict(amax=None), "amax / k_scale / v_scale is null"),
    (dict(k_scale=None), "amax / k_scale / v_scale is null"),
    (dict(v_scale=None), "amax / k_scale / v_scale is null"),
    (dict(v_scale=PTR + 2), "not aligned"),
    (dict(Hkv=0), "Hkv 0"),
    (dict(c=0.0), "c 0"),
    (dict(c=-1.0), "c -1"),
    (dict(c=float("inf")), "c inf"),
    (dict(c=float("nan")), "c nan"),
])
def test_scales_refusals_name_the_field(kw, frag):
    lib = _lib.load()
    assert lib.hyd_kv_scales_from_absmax(C.byref(_scales(**kw)), None) == -1
    assert frag in lib.hyd_last_error_string().decode()
    assert lib.hyd_kv_scales_from_absmax(None, None) == -1


def test_python_wrappers_refuse_bad_arguments():
    k = torch.zeros((2, 4, 2, 16), dtype=torch.bfloat16)
    amax = torch.zeros((2, 2))
    with pytest.raises(ValueError, match="both None"):
        Q.observe_absmax(None, None, amax)
    with pytest.raises(NotImplementedError, match="float16 / bfloat16"):
        Q.observe_absmax(k.float(), k.float(), amax)
    with pytest.raises(NotImplementedError, match="fp8 sources"):
        Q.observe_absmax(k.to(Q.FP8_DTYPE), None, amax)
    with pytest.raises(ValueError, match="multiple of 8"):
        Q.observe_absmax(k[..., :12], None, amax)
    with pytest.raises(ValueError, match="amax must be"):
        Q.observe_absmax(k, k, torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="row_lens"):
        Q.observe_absmax(k, k, amax, row_lens=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="margin"):
        Q.scales_from_absmax(amax, torch.ones(2), torch.ones(2), margin=0.0)
    with pytest.raises(ValueError, match="k_scale"):
        Q.scales_from_absmax(amax, torch.ones(3), torch.ones(2))


# ---- the definitions ------------------------------------------------------------------------------------------------------------
def test_absmax_reference_ignores_nonfinite_and_rows_past_the_lengths():
    k = torch.zeros((2, 4, 2, 8), dtype=torch.float16)
    v = torch.zeros_like(k)
    k[0, 1, 0, 3] = -3.0
    k[0, 2, 0, 0] = float("nan")
    k[0, 0, 1, 7] = float("-inf")
    k[1, 3, 1, 0] = 5.0       # past row_lens[1] = 3 below
    k[1, 2, 1, 1] = -0.0
    v[1, 0, 1, 2] = 2.0 ** -24  # the smallest f16 subnormal
    assert torch.equal(Q.absmax_reference(k, v), torch.tensor([[3.0, 5.0], [0.0, 2.0 ** -24]]))
    assert torch.equal(Q.absmax_reference(k, v, torch.tensor([4, 3])), torch.tensor([[3.0, 0.0], [0.0, 2.0 ** -24]]))
    assert torch.equal(Q.absmax_reference(k, None, torch.tensor([1, 0])), torch.zeros((2, 2)))
    assert torch.equal(Q.absmax_reference(None, k[0]), torch.tensor([[0.0, 0.0], [3.0, 0.0]]))  # [rows, Hkv, d], V alone
    # the CPU route of observe_absmax keeps a running maximum and leaves the row of a None tensor alone
    amax = torch.tensor([[4.0, 1.0], [7.0, 7.0]])
    Q.observe_absmax(k, None, amax)
    assert torch.equal(amax, torch.tensor([[4.0, 5.0], [7.0, 7.0]]))


def _f32(x):
    return torch.tensor(x, dtype=torch.float64).to(torch.float32)


def test_scale_rule_keeps_powers_of_two_and_rounds_everything_else_up():
    ks = list(range(-60, 61, 7)) + [-1, 0, 1]
    # margin 448: c == 1.0 exactly, so t == amax -- a power of two is kept, one fp32 ulp above it goes to the next power
    p2 = _f32([2.0 ** k for k in ks])
    assert torch.equal(Q.scales_from_absmax_reference(p2, margin=448.0), p2)
    up = torch.nextafter(p2, _f32([float("inf")] * len(ks)))
    assert torch.equal(Q.scales_from_absmax_reference(up, margin=448.0), 2 * p2)
    down = torch.nextafter(p2, _f32([0.0] * len(ks)))
    assert torch.equal(Q.scales_from_absmax_reference(down, margin=448.0), p2)
    # the default margin 2: amax = 448 * 2^k / 2 gives 2^k, not 2^(k + 1) (224 * float32(1 / 224) is within half an ulp of 1 from
    # above, or just below 1: both round up to 1), and one bf16 ulp above (225 * 2^k) gives the next power
    assert torch.equal(Q.scales_from_absmax_reference(224 * p2), p2)
    assert torch.equal(Q.scales_from_absmax_reference(225 * p2), 2 * p2)
    assert torch.equal(Q.scales_from_absmax_reference(_f32([100.0, 300.0, 448.0, 449.0]), margin=1.0), _f32([0.25, 1.0, 1.0, 2.0]))


def test_scale_rule_zero_clamps_and_the_16_bit_maxima():
    f16_max, bf16_max = 65504.0, float(torch.finfo(torch.bfloat16).max)
    f16_tiny, bf16_tiny = 2.0 ** -24, 2.0 ** -133  # smallest subnormals
    amax = _f32([0.0, f16_max, bf16_max, f16_tiny, bf16_tiny, 1e-38, 2.0 ** -93])
    s = Q.scales_from_absmax_reference(amax)
    assert s[0] == 1.0                                           # nothing observed
    assert s[1] == 512.0                                         # 65504 / 224 = 292.4
    assert s[2] == 2.0 ** 100 and s[2] < bf16_max / 224          # clamped from 2^121
    assert s[3] == 2.0 ** -31                                    # 2^-24 / 224 = 2^-31.8
    assert s[4] == s[5] == s[6] == 2.0 ** -100                   # clamped from below (2^-93 / 224 = 2^-100.8)
    assert all(math.frexp(float(x))[0] == 0.5 for x in s)        # every one a power of two
    lin = Q.scales_from_absmax_reference(amax, pow2=False)
    c = _f32(2.0 / 448.0)
    assert lin[0] == 1.0 and lin[1] == amax[1] * c and lin[2] == 2.0 ** 100 and lin[3] == amax[3] * c
    assert lin[4] == lin[5] == lin[6] == 2.0 ** -100
    # a huge margin overflows the product: the clamp takes it
    assert Q.scales_from_absmax_reference(_f32([bf16_max]), margin=1e6)[0] == 2.0 ** 100
    # the CPU route of scales_from_absmax writes the same values in place
    ks, vs = torch.empty(7), torch.empty(7)
    Q.scales_from_absmax(torch.stack([amax, amax.flip(0)]), ks, vs)
    assert torch.equal(ks, s) and torch.equal(vs, s.flip(0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k", [-10, -6, -1, 3, 6])
def test_power_of_two_rescaling_moves_the_scale_and_no_byte(dtype, k):
    g = torch.Generator().manual_seed(7 + k)
    x = torch.randn((3, 33, 4, 64), generator=g) * torch.tensor([0.02, 1.0, 1.0, 40.0]).reshape(1, 1, 4, 1)
    if dtype == torch.float16:  # keep x * 2^k out of f16's subnormals, where the rescaled numbers would round
        x = torch.where(x.abs() < 2.0 ** -4, torch.copysign(torch.tensor(2.0 ** -4), x), x)
    x = x.to(dtype)
    y = (x.float() * 2.0 ** k).to(dtype)
    assert torch.equal(y.float(), x.float() * 2.0 ** k)  # exact in the format: the same numbers at another exponent
    sx = Q.scales_from_absmax_reference(Q.absmax_reference(x, None))[0]
    sy = Q.scales_from_absmax_reference(Q.absmax_reference(y, None))[0]
    assert torch.equal(sy, sx * 2.0 ** k)
    assert torch.equal(Q.quantize_kv(x, sx).view(torch.uint8), Q.quantize_kv(y, sy).view(torch.uint8))
    # and a dequantized value is exactly a value of the 16-bit dtype
    back = Q.dequantize_kv(Q.quantize_kv(x, sx), sx, torch.float32)
    assert torch.equal(back, back.to(dtype).float())


# ---- the error budget: what the feature is for ------------------------------------------------------------------------------------
# relative L2 of float64 attention on dequantize(quantize(K / V)) against float64 attention on the bf16 inputs, B 4 x S 64 x H 4 x
# D 128.  Measured with these seeds: calibrated 3.6e-2 ... 4.1e-2 (whole tensor and worst head); unit scales 2.8e-1 ... 8.8e-1.
@pytest.mark.parametrize("name", sorted(cases.STATS))
def test_error_budget_calibrated_holds_and_unit_scales_do_not(name):
    q, k, v = cases.make_inputs(name)
    want = cases.attention64(q, k, v)
    scales = Q.scales_from_absmax_reference(Q.absmax_reference(k, v))
    cal = cases.rel_l2(cases.attention64(q, cases.fp8_round_trip(k, scales[0]), cases.fp8_round_trip(v, scales[1])), want)
    ones = torch.ones(cases.H)
    unit = cases.rel_l2(cases.attention64(q, cases.fp8_round_trip(k, ones), cases.fp8_round_trip(v, ones)), want)
    print(f"{name}: calibrated whole {cal[0]:.3e} worst head {cal[1]:.3e}; unit whole {unit[0]:.3e} worst head {unit[1]:.3e}")
    assert 1e-3 < cal[0] <= FP8_REL_L2_BOUND and cal[1] <= FP8_REL_L2_BOUND, cal
    assert unit[0] > FP8_REL_L2_BOUND, unit


# ---- the kernels' registers ---------------------------------------------------------------------------------------------------
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_kv_scale_kernels_have_no_scratch():
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                          str(REPO / "hydragen_amd" / "csrc" / "kv_scale.hip"), "-o", "-"], capture_output=True, text=True, check=True).stdout
    seen = []
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spill == 0 and scratch == 0 and vgpr <= 128, (name, vgpr, spill, scratch)
        seen.append(name)
    assert len(seen) == 3 and sum("kv_absmax_kernel" in n for n in seen) == 2 and sum("kv_scales_kernel" in n for n in seen) == 1
    assert "global_load_dwordx4" in out  # 16-byte vector loads
