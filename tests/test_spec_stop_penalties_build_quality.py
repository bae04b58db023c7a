"""-m "not gpu": what hipcc makes of csrc/draft_accept_stop.hip and csrc/sample_penalty_drafts.hip, read from the assembly's
metadata the way tests/test_per_row_build_quality.py reads it, and the untouched kernel sets of the files beside them."""
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
    return kernels, lds


def test_the_accept_kernels_are_two_and_use_no_lds_and_no_scratch():
    """draft_accept_stop_kernel<with states or not>: one row per lane, nothing in LDS, nothing spilled."""
    kernels, lds = _kernels("draft_accept_stop.hip")
    assert len(kernels) == 2 and all("draft_accept_stop_kernel" in k["name"] for k in kernels), [k["name"] for k in kernels]
    assert {re.search(r"ILb(\d)E", k["name"]).group(1) for k in kernels} == {"0", "1"}
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and lds[k["name"]] == 0, (k, lds[k["name"]])


def test_the_draft_sampler_is_three_kernels_at_two_rows_per_cu():
    """Three dtypes; no spill, no scratch; <= 64 VGPRs and the penalty kernel's LDS (<= 80 KB): two 1024-thread rows per CU."""
    kernels, lds = _kernels("sample_penalty_drafts.hip")
    assert len(kernels) == 3 and all("sample_penalty_drafts_kernel" in k["name"] for k in kernels), [k["name"] for k in kernels]
    assert {re.search(r"ILi(\d)E", k["name"]).group(1) for k in kernels} == {"0", "1", "2"}
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] <= 64 and lds[k["name"]] <= 80 * 1024, (k, lds[k["name"]])
    assert {lds[k["name"]] for k in kernels} == set(_kernels("sample_penalty.hip")[1][n] for n in _kernels("sample_penalty.hip")[1]
                                                   if "sample_penalty_kernel" in n)  # the penalty kernel's own LDS, not more


def test_the_files_beside_them_hold_the_kernels_they_held():
    for src, n, word in (("sample_penalty.hip", 4, "drafts"), ("sample_constrain.hip", 6, "drafts"), ("sample_filter.hip", 3, "drafts"),
                         ("sample_rows.hip", 6, "drafts"), ("draft_accept.hip", 2, "stop")):
        kernels, _ = _kernels(src)
        assert len(kernels) == n and not any(word in k["name"] for k in kernels), (src, [k["name"] for k in kernels])
    assert sorted(re.search(r"ILb(\d)E", k["name"]).group(1) for k in _kernels("draft_accept.hip")[0]) == ["0", "1"]
