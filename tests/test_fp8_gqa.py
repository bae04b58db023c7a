"""-m "not gpu": fp8 unique K/V caches on grouped-query heads -- which shapes the C ABI takes natively (hyd_kv_quant_supported, the
decode-level hyd_decode_kv_quant_supported) and the build pins of the new kernel file (suffix_attn_gqa_fp8.hip)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from hydragen_amd import _lib
from hydragen_amd._lib import DecodeParams, KvQuant, SuffixParams
from tests.test_build_quality import valu_sgpr_to_vmem_hazards

REPO = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"


def _sp(B=1024, nq=1, Hq=32, Hkv=8, D=128, S=64, dtype=_lib.HYD_BF16):
    p = SuffixParams()
    p.dtype, p.B, p.nq, p.Hq, p.Hkv, p.D, p.kv_len = dtype, B, nq, Hq, Hkv, D, S
    p.k_head_stride = p.v_head_stride = D
    p.k_tok_stride = p.v_tok_stride = Hkv * D
    p.k_batch_stride = p.v_batch_stride = S * Hkv * D
    return p


def _kq(flags=_lib.HYD_KVQ_GQA):
    kq = KvQuant()
    kq.kv_dtype, kq.flags = _lib.HYD_FP8_E4M3, flags
    return kq


def test_new_query_exported_and_declared():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    assert "hyd_decode_kv_quant_supported" in set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert "hyd_decode_kv_quant_supported" in _lib.EXPORTS and hasattr(lib, "hyd_decode_kv_quant_supported")
    assert "#define HYD_KVQ_GQA 1" in header and _lib.HYD_KVQ_GQA == 1
    assert lib.hyd_version() == 500  # additive


@pytest.mark.parametrize("dtype", [_lib.HYD_BF16, _lib.HYD_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape, native", [
    (dict(Hq=32, Hkv=8, D=128), True),            # C3
    (dict(Hq=64, Hkv=8, D=128), True),            # C5, llama3_70b
    (dict(Hq=8, Hkv=1, D=128), True),             # C5 TP = 8 slice
    (dict(Hq=8, Hkv=2, D=64), True),
    (dict(Hq=8, Hkv=1, D=256, B=2048), True),
    (dict(Hq=12, Hkv=4, D=128), True),            # 3-row units
    (dict(Hq=8, Hkv=2, D=128, nq=2), True),
    (dict(Hq=4, Hkv=2, D=128), False),            # 2 rows per unit: the dot-product kernel's shapes
    (dict(Hq=8, Hkv=8, D=128, nq=2), False),
    (dict(Hq=32, Hkv=8, D=96), False),
    (dict(Hq=2, Hkv=2, D=128), False),
    (dict(Hq=32, Hkv=32, D=128), True),           # the token-row kernel, as before
])
def test_kv_quant_supported_on_grouped_query_shapes(shape, native, dtype):
    lib = _lib.load()
    p = _sp(dtype=dtype, **shape)
    assert lib.hyd_kv_quant_supported(C.byref(p), C.byref(_kq())) == int(native)
    # callers that do not set HYD_KVQ_GQA keep the answers of the ABI as first released: grouped-query units are refused
    assert lib.hyd_kv_quant_supported(C.byref(p), C.byref(_kq(0))) == int(shape["Hq"] == shape["Hkv"] == 32)


def _decode(B, Hq, Hkv, P, S, sls, D=128):
    d = DecodeParams()
    d.suffix = _sp(B=B, Hq=Hq, Hkv=Hkv, D=D, S=S)
    d.n_levels = 1
    lv = d.levels[0]
    lv.sb, lv.kv_len = 1, P
    lv.k_head_stride = lv.v_head_stride = D
    lv.k_tok_stride = lv.v_tok_stride = Hkv * D
    lv.k_group_stride = lv.v_group_stride = P * Hkv * D
    d.phase = _lib.HYD_PHASE_ALL
    d.single_launch_small = sls
    return d


def test_decode_kv_quant_supported():
    lib = _lib.load()
    ask = lambda d, kq=None: lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(kq or _kq()))  # noqa: E731
    for sls in (0, 1):
        assert ask(_decode(128, 32, 8, 2048, 96, sls)) == 1
        assert ask(_decode(6, 32, 32, 96, 50, sls)) == 1  # Hq == Hkv: the flag is ignored, the pair runs
    # a call so small that 16-bit caches run it as ONE launch: refused with the flag, native without
    assert ask(_decode(6, 32, 8, 96, 50, 1)) == 0
    assert ask(_decode(6, 32, 8, 96, 50, 0)) == 1
    # shapes the suffix pass does not take stay refused; no quantization is always "supported"
    assert ask(_decode(128, 4, 2, 2048, 96, 0)) == 0
    assert ask(_decode(128, 32, 8, 2048, 96, 0), _kq(0)) == 0  # without HYD_KVQ_GQA
    same = KvQuant()
    same.kv_dtype = _lib.HYD_BF16
    assert ask(_decode(6, 32, 8, 96, 50, 1), same) == 1
    assert lib.hyd_decode_kv_quant_supported(C.byref(_decode(6, 32, 8, 96, 50, 1)), None) == 1


def test_refused_calls_fail_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.hyd_last_error_string().decode()  # noqa: E731
    d = _decode(6, 32, 8, 96, 50, 1)
    d.suffix.q = d.suffix.out = d.suffix.k = d.suffix.v = d.levels[0].k = d.levels[0].v = 4096  # never dereferenced
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(_kq()), None) == -2 and "ONE launch" in err()
    g = _sp(Hq=4, Hkv=2)
    g.q = g.out = g.k = g.v = 4096
    assert lib.hyd_suffix_attn_fwd_kvq(C.byref(g), C.byref(_kq()), None) == -2 and "not native" in err()


# ---- build pins of suffix_attn_gqa_fp8.hip ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm():
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not installed")
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           str(REPO / "hydragen_amd" / "csrc" / "suffix_attn_gqa_fp8.hip"), "-o", "-"],
                          capture_output=True, text=True, check=True).stdout


def test_fp8_gqa_kernels_registers(asm):
    metas = []
    for blk in asm.split("  - .agpr_count:")[1:]:
        g = lambda pat: int(re.search(pat, blk).group(1))  # noqa: E731
        metas.append((re.search(r"\.name:\s+(\S+)", blk).group(1), int(blk.split()[0]), g(r"\.vgpr_count:\s+(\d+)"),
                      g(r"\.vgpr_spill_count:\s+(\d+)"), g(r"\.sgpr_spill_count:\s+(\d+)"), g(r"\.private_segment_fixed_size:\s+(\d+)")))
    # {f16, bf16} x ({64, 128} x ({4 waves per unit} + {1, 2, 4 kv heads per workgroup}) + 256 x {1, 2 kv heads per workgroup})
    assert len(metas) == 20, [m[0] for m in metas]
    for name, agpr, vgpr, spill, sspill, scratch in metas:
        assert "suffix_attn_gqa_fp8_kernel" in name
        assert spill == 0 and sspill == 0 and scratch == 0, (name, spill, sspill, scratch)
        # (the count covers the unified file: accumulator registers sit on top of the vector ones)
        assert vgpr - agpr <= 256, (name, vgpr, agpr)
        if "ELi256E" not in name:
            assert agpr == 0 and vgpr <= 256, (name, agpr, vgpr)


def test_fp8_gqa_stream_has_only_the_hand_placed_waits(asm):
    """Between the first and the last LDS-DMA hipcc adds no counted vector-memory wait of its own (it cannot see the DMAs): the only
    counted one is the hand-placed wait of the two-set scheme, which leaves the younger step's 2 * D / 32 requests out."""
    seen = 0
    for m in re.finditer(r"^(_ZN3hyd\d+suffix_attn_gqa_fp8_kernel\w+):(.*?)s_endpgm", asm, flags=re.S | re.M):
        seen += 1
        body = m.group(2)
        first_dma = body.find(" lds")
        assert first_dma > 0, m.group(1)
        lines = body[first_dma:].splitlines()
        last_dma = max(i for i, ln in enumerate(lines) if ln.rstrip().endswith(" lds") or " lds " in ln)
        counted = [ln.strip() for ln in lines[:last_dma] if re.search(r"s_waitcnt vmcnt\((?!0\))", ln)]
        d = int(re.search(r"ELi(64|128|256)E", m.group(1)).group(1))
        if d <= 128:
            counted = [ln for ln in counted if ln != f"s_waitcnt vmcnt({2 * d // 32})"]
        assert not counted, (m.group(1), counted[:3])
    assert seen == 20


def test_fp8_gqa_dma_keeps_its_distance_from_valu_written_scalars(asm):
    bad = valu_sgpr_to_vmem_hazards(asm)
    assert not bad, f"{len(bad)} hazards, first: {bad[:3]}"
