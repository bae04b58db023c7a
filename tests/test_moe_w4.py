"""-m "not gpu": 4-bit experts without a device: quantizer, definition, quantize_experts(dtype=fp4), hyd_moe_mlp_w4's mirror and refusals, moe_w4.hip's registers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, moe
from hydragen_amd.weight_quant import FP4_DTYPE, _group_values, quantize_weight_fp4
from tests.test_build_quality import HIPCC, _metadata
from tests.test_moe_abi import REPO, tiny_hf

U8, F32 = torch.uint8, torch.float32


def test_quantizer_is_quantize_weight_fp4_per_row_and_the_cpu_mlp_is_the_definition():
    g = torch.Generator().manual_seed(0)
    gate_up, down = ((torch.randn(s, generator=g) * sd).to(torch.bfloat16) for s, sd in (((3, 64, 64), 0.3), ((3, 64, 32), 0.1)))
    gate_up[1, 5], down[2, 7] = 0, down[2, 7] * 1000  # a zero row (scale 1) and a row 1000 x larger than the others
    q = moe.quantize_experts_fp4(gate_up, down)
    deq = moe.dequantize_experts_fp4(*q)
    for w, (w4, sh, sc), d in ((gate_up, q[:3], deq[0]), (down, q[3:], deq[1])):
        E, N, K = w.shape
        w4r, shr, scr = quantize_weight_fp4(w.view(-1, K))
        assert [t.dtype for t in (w4, sh, sc)] == [U8, U8, F32] and (w4.shape, sh.shape, sc.shape) == ((E, N, K // 2), (E, N, K // 32), (E, N))
        assert torch.equal(w4.view(w4r.shape), w4r) and torch.equal(sh.view(shr.shape), shr) and torch.equal(sc.view(-1), scr)
        assert d.dtype == torch.float64 and torch.equal(d, (_group_values(w4r, shr, torch.float64) * scr.double()[:, None]).view(E, N, K))
    # Quantizing the dequantized weights again changes no VALUE.  It does change bytes, by quantize_weight_fp4's own rule: a group (or
    # row) whose largest code came out as 3.0 (|t| in (3, 3.5]) now has absmax / 6 equal to half its step, so the rule picks the next
    # smaller power of two and writes 6.0 under shift + 1 (or half the scale) -- here 62 of 384 gate_up shifts and 36 of 192 down scales.
    assert all(torch.equal(a, b) for a, b in zip(moe.dequantize_experts_fp4(*moe.quantize_experts_fp4(*deq)), deq))
    x, router = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((7, 64), (3, 64)))
    kw = dict(gate_up_scale=q[2], down_scale=q[5], gate_up_shift=q[1], down_shift=q[4])
    y, ids, w = moe.moe_mlp(x, router, q[0], q[3], 2, True, return_routing=True, **kw)
    assert torch.equal(y, moe.moe_reference(x, router, *deq, 2, True).to(torch.bfloat16)) and ids.shape == w.shape == (7, 2)
    with pytest.raises(ValueError, match="come together"):
        moe.moe_mlp(x, router, q[0], q[3], 2, True, gate_up_shift=q[1], down_shift=q[4])


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_quantize_experts_fp4_replaces_the_modules_and_the_state_dict_round_trips(kind):
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    m, twin = (HydragenLlamaForCausalLM.from_hf_model(tiny_hf(kind)) for _ in range(2))
    want = moe.quantize_experts_fp4(m.model.layers[0].mlp.experts.gate_up_proj, m.model.layers[0].mlp.experts.down_proj)
    with pytest.raises(NotImplementedError, match="float8_e4m3fn and .*float4_e2m1fn_x2"):
        m.quantize_experts(dtype=torch.int8)
    m.quantize_experts(dtype=FP4_DTYPE)
    e = m.model.layers[0].mlp.experts
    assert isinstance(e, moe.Fp4Experts) and not list(e.parameters()) and [n for n, _ in e.named_buffers()] == list(moe.Fp4Experts.NAMES)
    assert [b.dtype for b in e.buffers()] == [U8, U8, F32] * 2
    x = torch.randn(5, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    with torch.no_grad():  # the module's CPU forward is the definition on the dequantized weights
        ref = moe.moe_reference(x, m.model.layers[0].mlp.gate.weight, *moe.dequantize_experts_fp4(*e.buffers()), 2, kind == "mixtral")
        assert torch.equal(m.model.layers[0].mlp(x), ref.to(x.dtype))
    twin.quantize_experts(dtype=FP4_DTYPE)
    for b in twin.model.layers[0].mlp.experts.buffers():
        b.view(U8).zero_()
    twin.load_state_dict(m.state_dict())
    assert "model.layers.0.mlp.experts.down_proj_shift" in m.state_dict() and all(torch.equal(v.view(U8), twin.state_dict()[n].view(U8)) for n, v in m.state_dict().items())
    m.half()
    assert [b.dtype for b in e.buffers()] == [U8, U8, F32] * 2 and e.dtype == torch.float16 and m.model.layers[0].mlp.gate.weight.dtype == torch.float16
    assert all(torch.equal(a, b) for a, b in zip(e.buffers(), want))
    with pytest.raises(RuntimeError, match="already"):
        m.quantize_experts(dtype=FP4_DTYPE)


def test_mirror_has_the_c_layout_and_the_entry_point_is_exported(tmp_path):
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    lib = _lib.load()
    assert re.search(r"HYD_API int hyd_moe_mlp_w4\(", header) and "hyd_moe_mlp_w4" in _lib.EXPORTS and hasattr(lib, "hyd_moe_mlp_w4") and lib.hyd_version() == 500
    fields = [n for n, _ in moe.MoeW4Params._fields_]
    body = 'printf("%zu ", sizeof(hyd_moe_w4_params));' + "".join(f'printf("%zu ", offsetof(hyd_moe_w4_params, {n}));' for n in fields)
    (tmp_path / "s.c").write_text('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    want = [C.sizeof(moe.MoeW4Params)] + [getattr(moe.MoeW4Params, n).offset for n in fields]
    assert fields[-4:] == ["gate_up_scale", "down_scale", "gate_up_shift", "down_shift"] and list(map(int, subprocess.check_output([str(tmp_path / "s")]).split())) == want


@pytest.mark.parametrize("kw, code, frag", [
    (dict(gate_up_shift=0), -1, "gate_up_shift / down_shift is null"), (dict(down_shift=0), -1, "is null"), (dict(gate_up_scale=0), -1, "gate_up_scale / down_scale is null"),
    (dict(down_scale=0x80001), -1, "not aligned"), (dict(H=256, x_row_stride=256, y_row_stride=256, gate_up_shift=0x90004), -1, "8-byte aligned"),
    (dict(I=256, down_shift=0xa0001), -1, "8-byte aligned"), (dict(T=129), -1, "T 129"), (dict(H=96, x_row_stride=96, y_row_stride=96), -1, "H 96"),
    (dict(I=48), -1, "I 48"), (dict(workspace_bytes=1024), -3, "workspace bytes"),
    (dict(gate_up_shift=0x90001, down_shift=0xa0003, workspace=0), -3, "workspace"),  # H 128, I 64: no alignment asked of the shifts; the next check answers
])
def test_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    p = moe.MoeW4Params()
    base = dict(x=0x10000, logits=0x20000, gate_up=0x30000, down=0x40000, y=0x50000, workspace=0x60000, workspace_bytes=1 << 30, T=8, E=8, k=2, H=128, I=64,
                renormalize=1, dtype=_lib.HYD_BF16, x_row_stride=128, y_row_stride=128, gate_up_scale=0x70000, down_scale=0x80000, gate_up_shift=0x90000, down_shift=0xa0000)
    for k, v in {**base, **kw}.items():
        setattr(p, k, v)
    assert _lib.load().hyd_moe_mlp_w4(C.byref(p), None) == code and frag in _lib.load().hyd_last_error_string().decode()


# unified VGPRs as built (120 / 172 / 120 / 156, both dtypes), rounded up to the next allocation step of 8 and one step of slack: DESIGN 4.23''
VGPR_BUDGET = [(r"gate_up_w4_kernelINS_\w+ELi1E", 128), (r"gate_up_w4_kernelINS_\w+ELi2E", 184), (r"down_w4_kernelINS_\w+ELi1E", 128), (r"down_w4_kernelINS_\w+ELi2E", 168)]


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_moe_w4_kernels_have_no_scratch_no_spills_and_stay_in_their_vgpr_budget():
    _, kernels = _metadata("moe_w4.hip")
    assert len(kernels) == 8, [k["name"] for k in kernels]  # 2 dtypes x 2 tilings x (gate_up, down)
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        lims = [lim for pat, lim in VGPR_BUDGET if re.search(pat, k["name"])]
        assert len(lims) == 1 and k["vgpr"] <= lims[0], k
