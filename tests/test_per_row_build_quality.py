"""-m "not gpu": register allocation of the per-row sampling kernels (csrc/sample_rows.hip), read from the assembly's metadata the
way tests/test_build_quality.py reads the build, and the scalar samplers' untouched kernel sets."""
import re
from pathlib import Path

import pytest

HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")


def _kernels(src):
    from tests.test_build_quality import _device_asm, _metadata

    _, kernels = _metadata(src)
    lds = {}
    for blk in _device_asm(src).split("  - .agpr_count:")[1:]:
        lds[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    return kernels, lds, _device_asm(src)


def test_per_row_kernels_have_no_scratch_and_keep_their_registers():
    """Six kernels (two families x three dtypes), nothing spilled, no scratch, no LDS beyond the scalar kernels' (the 2400 bytes of
    sample_filter.hip's histogram and reduction slots; the penalty tables' 72032).  The penalised family keeps two workgroups per
    CU (<= 64 VGPRs, <= 80 KB); the family without penalties sits at 63 / 65 / 70 VGPRs (f16 / bf16 / fp32; the constrained scalar
    kernels it extends: 61 / 61 / 66) -- the row's scalar values cost it a few registers where they meet vector operands, and the
    fp32 instantiation leaves the samplers' 50-66 range (profiles/per_row_sampling.md records the counts and the reason)."""
    kernels, lds, asm = _kernels("sample_rows.hip")
    plain = {re.search(r"ILi(\d)E", k["name"]).group(1): k for k in kernels if "sample_rows_kernel" in k["name"]}
    pen = {re.search(r"ILi(\d)E", k["name"]).group(1): k for k in kernels if "sample_rows_penalty_kernel" in k["name"]}
    assert len(plain) == 3 and len(pen) == 3 and len(kernels) == 6, [k["name"] for k in kernels]
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] <= 128, k  # 1024 threads = 4 waves per SIMD
    for k in pen.values():
        assert 50 <= k["vgpr"] <= 64 and lds[k["name"]] <= 80 * 1024, (k, lds[k["name"]])
    for k in plain.values():
        assert lds[k["name"]] <= 4096, (k, lds[k["name"]])
    assert 50 <= plain["0"]["vgpr"] <= 66 and 50 <= plain["1"]["vgpr"] <= 66  # HYD_F16 0, HYD_BF16 1: the samplers' range
    if "roc-7.2.0 26014" in asm:  # what this hipcc gives (its .ident line), pinned as tests/test_sampling_penalties.py pins its kernels
        assert {d: k["vgpr"] for d, k in plain.items()} == {"0": 63, "1": 65, "2": 70}
        assert {d: k["vgpr"] for d, k in pen.items()} == {"0": 58, "1": 58, "2": 58}


def test_scalar_sampler_files_hold_the_kernels_they_held():
    """The per-row forms are instantiations of their own, in a file of their own: the scalar files' kernel sets are what they were."""
    for src, n in (("sample_filter.hip", 3), ("sample_penalty.hip", 4), ("sample_constrain.hip", 6)):
        kernels, _, _ = _kernels(src)
        assert len(kernels) == n and not any("rows" in k["name"] for k in kernels), (src, [k["name"] for k in kernels])
