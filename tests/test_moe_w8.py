"""-m "not gpu": fp8 experts without a device: quantizer, definition, quantize_experts(), hyd_moe_mlp_w8's mirror and refusals, moe_w8.hip's registers."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, moe
from hydragen_amd.weight_quant import quantize_weight
from tests.test_moe_abi import REPO, tiny_hf
from hydragen_amd.kv_quant import FP8_DTYPE as FP8
from tests.test_build_quality import HIPCC, _metadata
from tests.test_weight_fp8 import tiny_model


def test_quantizer_is_quantize_weight_per_row_and_the_cpu_mlp_is_the_definition():
    g = torch.Generator().manual_seed(0)
    gate_up, down = ((torch.randn(s, generator=g) * sd).to(torch.bfloat16) for s, sd in (((3, 64, 64), 0.3), ((3, 64, 32), 0.1)))
    gate_up[1, 5], down[2, 7] = 0, down[2, 7] * 1000  # a zero row (scale 1) and a row with a scale of its own
    q = moe.quantize_experts(gate_up, down)
    for w, w8, s in ((gate_up, q[0], q[1]), (down, q[2], q[3])):
        w8r, sr = quantize_weight(w.view(-1, w.shape[2]))
        assert w8.dtype == FP8 and w8.shape == w.shape and torch.equal(w8.view(torch.uint8).view(w8r.shape), w8r.view(torch.uint8)) and torch.equal(s.view(-1), sr)
    deq = moe.dequantize_experts(*q)
    for d, w8, s in zip(deq, q[0::2], q[1::2]):  # code * scale, exactly; a 16-bit dtype holds it; quantizing it again changes no value
        assert d.dtype == torch.float64 and torch.equal(d, w8.double() * s.double()[..., None])
    for other in (moe.dequantize_experts(*q, dtype=torch.bfloat16), moe.dequantize_experts(*moe.quantize_experts(*deq))):
        assert all(torch.equal(a.double(), b) for a, b in zip(other, deq))
    x, router = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((7, 64), (3, 64)))
    y, ids, w = moe.moe_mlp(x, router, q[0], q[2], 2, True, return_routing=True, gate_up_scale=q[1], down_scale=q[3])
    assert torch.equal(y, moe.moe_reference(x, router, *deq, 2, True).to(torch.bfloat16)) and ids.shape == w.shape == (7, 2)


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_quantize_experts_replaces_the_modules_and_the_state_dict_round_trips(kind):
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    hf = tiny_hf(kind)
    m, twin = (HydragenLlamaForCausalLM.from_hf_model(hf) for _ in range(2))
    want = moe.quantize_experts(m.model.layers[0].mlp.experts.gate_up_proj, m.model.layers[0].mlp.experts.down_proj)
    m.quantize_experts()
    e = m.model.layers[0].mlp.experts
    bufs = (e.gate_up_proj, e.gate_up_proj_scale, e.down_proj, e.down_proj_scale)
    assert isinstance(e, moe.Fp8Experts) and not list(e.parameters()) and [b.dtype for b in bufs] == [FP8, torch.float32] * 2
    x = torch.randn(5, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    with torch.no_grad():  # the module's CPU forward is the definition on the dequantized weights
        assert torch.equal(m.model.layers[0].mlp(x), moe.moe_reference(x, m.model.layers[0].mlp.gate.weight, *moe.dequantize_experts(*bufs), 2, kind == "mixtral").to(x.dtype))
    twin.quantize_experts()
    for b in twin.model.layers[0].mlp.experts.buffers():
        b.view(torch.uint8).zero_()
    twin.load_state_dict(m.state_dict())
    assert "model.layers.0.mlp.experts.down_proj_scale" in m.state_dict() and all(torch.equal(v.view(torch.uint8), twin.state_dict()[n].view(torch.uint8)) for n, v in m.state_dict().items())
    m.half()
    assert [b.dtype for b in e.buffers()] == [FP8, torch.float32] * 2 and e.dtype == torch.float16 and m.model.layers[0].mlp.gate.weight.dtype == torch.float16
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(e.buffers(), want))
    with pytest.raises(RuntimeError, match="already"):
        m.quantize_experts()
    with pytest.raises(NotImplementedError, match="without experts"):
        tiny_model().quantize_experts()


def test_mirror_has_the_c_layout_and_the_entry_point_is_exported(tmp_path):
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    lib = _lib.load()
    assert re.search(r"HYD_API int hyd_moe_mlp_w8\(", header) and "hyd_moe_mlp_w8" in _lib.EXPORTS and hasattr(lib, "hyd_moe_mlp_w8") and lib.hyd_version() == 500
    fields = [n for n, _ in moe.MoeW8Params._fields_]
    body = 'printf("%zu ", sizeof(hyd_moe_w8_params));' + "".join(f'printf("%zu ", offsetof(hyd_moe_w8_params, {n}));' for n in fields)
    (tmp_path / "s.c").write_text('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    want = [C.sizeof(moe.MoeW8Params)] + [getattr(moe.MoeW8Params, n).offset for n in fields]
    assert list(map(int, subprocess.check_output([str(tmp_path / "s")]).split())) == want


@pytest.mark.parametrize("kw, code, frag", [
    (dict(gate_up_scale=0), -1, "gate_up_scale / down_scale is null"), (dict(down_scale=0), -1, "is null"), (dict(gate_up_scale=0x70002), -1, "not aligned"),
    (dict(down_scale=0x80001), -1, "not aligned"), (dict(T=129), -1, "T 129"), (dict(H=96, x_row_stride=96, y_row_stride=96), -1, "H 96"), (dict(I=48), -1, "I 48"),
    (dict(down=0x40004), -1, "down must be 16-byte aligned"), (dict(workspace_bytes=1024), -3, "workspace bytes"),
])
def test_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    p = moe.MoeW8Params()
    base = dict(x=0x10000, logits=0x20000, gate_up=0x30000, down=0x40000, y=0x50000, workspace=0x60000, workspace_bytes=1 << 30, T=8, E=8, k=2, H=128,
                I=64, renormalize=1, dtype=_lib.HYD_BF16, x_row_stride=128, y_row_stride=128, gate_up_scale=0x70000, down_scale=0x80000)
    for k, v in {**base, **kw}.items():
        setattr(p, k, v)
    assert _lib.load().hyd_moe_mlp_w8(C.byref(p), None) == code and frag in _lib.load().hyd_last_error_string().decode()


# unified VGPRs as built (116-120 / 160-168), rounded up to the next allocation step of 8 and one step of slack: DESIGN 4.23'
VGPR_BUDGET = [(r"gate_up_w8_kernelINS_\w+ELi1E", 128), (r"gate_up_w8_kernelINS_\w+ELi2E", 176), (r"down_w8_kernelINS_\w+ELi1E", 128), (r"down_w8_kernelINS_\w+ELi2E", 168)]


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_moe_w8_kernels_have_no_scratch_no_spills_and_stay_in_their_vgpr_budget():
    _, kernels = _metadata("moe_w8.hip")
    assert len(kernels) == 8, [k["name"] for k in kernels]  # 2 dtypes x 2 tilings x (gate_up, down)
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        lims = [lim for pat, lim in VGPR_BUDGET if re.search(pat, k["name"])]
        assert len(lims) == 1 and k["vgpr"] <= lims[0], k
