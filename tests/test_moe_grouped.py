"""-m "not gpu": hyd_moe_mlp_grouped without a device -- its exports, refusals and workspace formula, and the register / LDS
allocation of csrc/moe_grouped.hip."""
import ctypes as C
import re
from pathlib import Path

import pytest

from hydragen_amd import _lib, moe
from tests.test_moe_abi import REPO, _params


def test_entry_points_are_declared_listed_and_exported():
    header, lib = (REPO / "include" / "hydragen_hip.h").read_text(), _lib.load()
    for name in ("hyd_moe_grouped_workspace_bytes", "hyd_moe_mlp_grouped"):
        assert re.search(rf"HYD_API \w+ {name}\(", header) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.hyd_version() == 500 and f"#define HYD_MOE_GROUPED_MAX_ROWS {moe.MOE_GROUPED_MAX_ROWS}\n" in header
    assert moe.MOE_GROUPED_MAX_ROWS == 2048 and moe.MOE_GROUPED_MIN_ROWS >= 512


@pytest.mark.parametrize("kw, code, frag", [
    (dict(T=0), -1, "T 0: 1 to 2048"), (dict(T=2049), -1, "T 2049: 1 to 2048"), (dict(E=257, k=8), -1, "E 257"), (dict(k=3, E=2), -1, "k 3 exceeds E 2"),
    (dict(H=96, x_row_stride=96, y_row_stride=96), -1, "H 96"), (dict(I=48), -1, "I 48"), (dict(x=0), -1, "x is null"),
    (dict(down=0x40004), -1, "down must be 16-byte aligned"), (dict(workspace=0), -3, "workspace"), (dict(workspace=0x60008), -3, "16-byte"),
])
def test_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_moe_mlp_grouped(C.byref(_params(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


def test_row_129_is_the_grouped_calls_alone():
    """hyd_moe_mlp refuses T = 129; the grouped call takes it to the last argument check (the workspace's size) and, where no device
    is present, to its first launch (on a device the call would run on the made-up addresses: it is not made there)."""
    import torch

    lib = _lib.load()
    assert lib.hyd_moe_mlp(C.byref(_params(T=129)), None) == -1 and "T 129: 1 to 128" in lib.hyd_last_error_string().decode()
    assert lib.hyd_moe_mlp_grouped(C.byref(_params(T=129, workspace_bytes=1024)), None) == -3
    assert "moe_mlp_grouped needs" in lib.hyd_last_error_string().decode() and "for T 129 " in lib.hyd_last_error_string().decode()
    if not torch.cuda.is_available():
        assert lib.hyd_moe_mlp_grouped(C.byref(_params(T=129)), None) == -4  # HYD_ERR_LAUNCH
        assert "moe_mlp_grouped kernel launches failed" in lib.hyd_last_error_string().decode()


def test_workspace_query_is_the_headers_formula():
    lib = _lib.load()
    q, r16 = lib.hyd_moe_grouped_workspace_bytes, lambda n: (n + 15) // 16 * 16
    for T, E, k, H, I in ((1, 4, 1, 64, 32), (129, 200, 8, 192, 96), (1024, 8, 2, 4096, 14336), (2048, 256, 8, 2048, 768)):
        n = T * k  # ids, weights, counts, slots, tiles, act, yslot
        want = 3 * r16(4 * n) + r16(4 * E) + 16 * ((n + 63) // 64 + min(E, n)) + r16(2 * n * I) + r16(4 * n * H)
        assert q(T, E, k, H, I, _lib.HYD_BF16) == q(T, E, k, H, I, _lib.HYD_F16) == want
    assert q(2049, 8, 2, 64, 32, 1) == q(0, 8, 2, 64, 32, 1) == q(8, 257, 2, 64, 32, 1) == q(8, 2, 3, 64, 32, 1) == q(8, 8, 2, 96, 32, 1) == q(8, 8, 2, 64, 48, 1) == 0
    assert q(8, 8, 2, 64, 32, _lib.HYD_F32) == 0
    assert lib.hyd_moe_mlp_grouped(C.byref(_params(T=129, workspace_bytes=q(129, 8, 2, 128, 64, 1) - 1)), None) == -3


def test_kernels_have_no_scratch_no_spills_and_two_workgroups_per_cu():
    """Two 64 KB workgroups per CU are two waves per SIMD: 256 unified VGPRs a wave and at most 80 KB of LDS a workgroup."""
    from tests.test_build_quality import HIPCC, _device_asm, _metadata

    if not Path(HIPCC).exists():
        pytest.skip("hipcc not installed")
    _, kernels = _metadata("moe_grouped.hip")
    assert len(kernels) == 10, [k["name"] for k in kernels]  # count, place, 2 dtypes x 2 tile heights x (gate_up, down)
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 256, k
    blocks = _device_asm("moe_grouped.hip").split("  - .agpr_count:")[1:]
    lds = [int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)) for b in blocks if re.search(r"\.name:\s+\S*(gate_up|down)_kernel", b)]
    assert len(lds) == 8 and 0 < min(lds) and max(lds) <= 80 << 10, lds
