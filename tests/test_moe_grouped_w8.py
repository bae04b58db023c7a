"""-m "not gpu": hyd_moe_mlp_grouped_w8 without a device -- its export, refusals and workspace, and the register / LDS allocation of
csrc/moe_grouped_w8.hip."""
import ctypes as C
import re
from pathlib import Path

import pytest

from hydragen_amd import _lib, moe
from tests.test_moe_abi import REPO, _params


def params8(gate_up_scale=0x70000, down_scale=0x80000, **kw):
    src, p = _params(**kw), moe.MoeW8Params()
    for name, _ in moe.MoeParams._fields_:
        setattr(p, name, getattr(src, name))
    p.gate_up_scale, p.down_scale = gate_up_scale, down_scale
    return p


def test_entry_point_is_declared_listed_exported_and_takes_the_grouped_workspace():
    header, lib, name = (REPO / "include" / "hydragen_hip.h").read_text(), _lib.load(), "hyd_moe_mlp_grouped_w8"
    assert re.search(rf"HYD_API int {name}\(const hyd_moe_w8_params\* p, void\* stream\);", header) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.hyd_version() == 500
    need = lib.hyd_moe_grouped_workspace_bytes(129, 8, 2, 128, 64, _lib.HYD_BF16)
    assert lib.hyd_moe_mlp_grouped_w8(C.byref(params8(T=129, workspace_bytes=need - 1)), None) == -3
    assert f"moe_mlp_grouped_w8 needs {need} workspace bytes for T 129 " in lib.hyd_last_error_string().decode()


@pytest.mark.parametrize("kw, code, frag", [
    (dict(T=0), -1, "T 0: 1 to 2048"), (dict(T=2049), -1, "T 2049: 1 to 2048"), (dict(H=96, x_row_stride=96, y_row_stride=96), -1, "H 96"),
    (dict(I=48), -1, "I 48"), (dict(k=3, E=2), -1, "k 3 exceeds E 2"), (dict(gate_up_scale=0), -1, "gate_up_scale / down_scale is null"),
    (dict(down_scale=0), -1, "gate_up_scale / down_scale is null"), (dict(down=0x40004), -1, "down must be 16-byte aligned"), (dict(workspace=0), -3, "workspace"),
])
def test_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_moe_mlp_grouped_w8(C.byref(params8(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


def test_row_129_reaches_the_launch():
    """Where no device is present the call gets to its first launch (on a device it would run on the made-up addresses: not made there)."""
    import torch

    lib = _lib.load()
    if not torch.cuda.is_available():
        assert lib.hyd_moe_mlp_grouped_w8(C.byref(params8(T=129)), None) == -4  # HYD_ERR_LAUNCH
        assert "moe_mlp_grouped_w8 kernel launches failed" in lib.hyd_last_error_string().decode()


def test_kernels_have_no_scratch_no_spills_and_two_workgroups_per_cu():
    """Two workgroups per CU are two waves per SIMD: 256 unified VGPRs a wave and at most 80 KB of LDS a workgroup."""
    from tests.test_build_quality import HIPCC, _device_asm, _metadata

    if not Path(HIPCC).exists():
        pytest.skip("hipcc not installed")
    _, kernels = _metadata("moe_grouped_w8.hip")
    assert len(kernels) == 8, [k["name"] for k in kernels]  # 2 dtypes x 2 tile heights x (gate_up, down)
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 256, k
    lds = [int(n) for n in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", _device_asm("moe_grouped_w8.hip"))]
    assert len(lds) == 8 and 0 < min(lds) and max(lds) <= 80 << 10, lds
