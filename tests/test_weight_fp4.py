"""-m "not gpu": 4-bit (e2m1) linear-layer weights (hydragen_amd/weight_quant.py, csrc/linear_w4.hip) -- the quantizer against its
stated rule and error bound, the model shell on the CPU, the new entry points' bookkeeping and refusals replayed without a device."""
import copy
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd import weight_quant as wq
from tests.test_weight_fp8 import _weights, dequantized_twin, tiny_model

REPO = Path(__file__).resolve().parent.parent
FP4 = torch.float4_e2m1fn_x2


def _w(seed=0):
    w = _weights(seed, N=48, K=96)  # rows of very different magnitude, a zero row, a row one value sets the scale of
    w[9, 32:64] = 0                 # a zero group
    w[11, :32] *= 2.0 ** -15        # a group far below its row: its shift clamps at 12
    return w


def test_scales_shifts_and_codes_follow_the_rule_and_the_elementwise_bound():
    w = _w()
    w4, shift, scale = wq.quantize_weight_fp4(w)
    assert (w4.dtype, w4.shape, shift.dtype, shift.shape, scale.dtype, scale.shape) == (torch.uint8, (48, 48), torch.uint8, (48, 3), torch.float32, (48,))
    assert torch.equal(torch.frexp(scale)[0], torch.full((48,), 0.5)), "every scale is a power of two"
    assert int(shift.max()) == 12 and shift[11, 0] == 12 and int(shift[:, :].min()) == 0
    amax = w.abs().amax(1).double()
    nz = amax > 0
    assert bool((scale.double()[nz] * 6 >= amax[nz]).all()) and bool((scale.double()[nz] * 3 < amax[nz]).all()), "the smallest power of two >= absmax / 6"
    assert scale[5] == 1.0 and not w4[5].any() and not shift[5].any(), "a zero row: scale 1, codes 0, shifts 0"
    assert shift[9, 1] == 0 and not w4[9, 16:32].any(), "a zero group: shift 0, codes 0"
    gscale = (scale.double()[:, None] * torch.exp2(-shift.double())).repeat_interleave(32, dim=1)
    gmax = w.abs().view(48, 3, 32).amax(2).double()
    free = ((shift < 12) & (gmax > 0)).repeat_interleave(32, dim=1)  # groups whose own power of two was expressed exactly
    assert bool((gscale * 6 >= w.abs().double())[free].all()) and bool(((gscale * 3)[:, ::32] < gmax)[free[:, ::32]].all())
    err = (wq.dequantize_weight_fp4(w4, shift, scale, torch.float32).double() - w.double()).abs()
    assert bool((err <= torch.maximum(w.double().abs(), gscale) / 4)[free].all())


def test_ties_go_to_the_even_mantissa_infinities_clamp_and_nan_is_refused():
    row = torch.zeros((1, 32))
    row[0, :11] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -5.0, float("inf"), float("-inf")])
    w4, shift, scale = wq.quantize_weight_fp4(row)
    assert scale[0] == 1.0 and shift[0, 0] == 0
    got = wq.dequantize_weight_fp4(w4, shift, scale, torch.float32)[0, :11]
    assert got.tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -4.0, 6.0, -6.0]
    with pytest.raises(ValueError, match="NaN"):
        wq.quantize_weight_fp4(torch.full((1, 32), float("nan")))


def test_concatenation_along_n_is_exact_and_the_reference_is_the_float64_product():
    a, b = _w(1), _w(2) * 100
    qa, qb, qab = wq.quantize_weight_fp4(a), wq.quantize_weight_fp4(b), wq.quantize_weight_fp4(torch.cat([a, b]))
    for i in range(3):
        assert torch.equal(torch.cat([qa[i], qb[i]]), qab[i])
    lins = [torch.nn.Linear(96, 48, bias=False) for _ in range(2)]
    lins[0].weight.data, lins[1].weight.data = a, b
    mod = wq.Fp4Linear.from_linears(lins)
    assert torch.equal(mod.weight, qab[0]) and torch.equal(mod.weight_shift, qab[1]) and torch.equal(mod.weight_scale, qab[2])
    x = torch.randn((5, 96), generator=torch.Generator().manual_seed(5)).bfloat16()
    assert torch.equal(wq.linear_reference_fp4(x, *qa), x.double() @ wq.dequantize_weight_fp4(*qa, torch.float64).T)


@pytest.fixture(scope="module")
def models():
    m = tiny_model()
    ref = copy.deepcopy(m)
    m.quantize_weights(dtype=FP4)
    return m, ref


def test_cpu_forward_equals_the_model_on_dequantized_16_bit_weights(models):
    m, ref = models
    assert isinstance(m.model.layers[0].self_attn.qkv_proj, wq.Fp4Linear) and isinstance(m.lm_head, torch.nn.Linear)
    twin = dequantized_twin(m, copy.deepcopy(ref))
    for mm in (m, twin):
        mm.model.set_disable_hydragen(True)
        mm.model.set_disable_attention(True)
    ids = torch.randint(0, 512, (3, 9), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(9)[None].expand(3, 9)
    with torch.no_grad():
        got, want = m(ids, pos, full_logits=True), twin(ids, pos, full_logits=True)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    lin = m.model.layers[0].mlp.down_proj
    x = torch.randn((3, lin.in_features), generator=torch.Generator().manual_seed(0)).bfloat16()
    assert torch.equal(lin(x), torch.nn.functional.linear(x, lin.dequantized()))


def test_state_dict_round_trip_is_exact_and_a_cast_keeps_the_buffers(models):
    m, _ = models
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for stem in ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj"):
        assert all(f"model.layers.0.{stem}.{b}" in sd for b in ("weight", "weight_shift", "weight_scale"))
    other = tiny_model(seed=7)
    with pytest.raises(NotImplementedError):
        other.quantize_weights(dtype=torch.float8_e5m2)
    other.quantize_weights(dtype=FP4)
    assert not torch.equal(other.model.layers[0].mlp.down_proj.weight, m.model.layers[0].mlp.down_proj.weight)
    other.load_state_dict(sd)
    got = other.state_dict()
    assert got.keys() == sd.keys() and all(got[k].dtype == v.dtype and torch.equal(got[k], v) for k, v in sd.items())
    mod = copy.deepcopy(m.model.layers[0].self_attn.o_proj).to(torch.float16)
    ref = m.model.layers[0].self_attn.o_proj
    assert mod.dtype == torch.float16 and mod.weight_scale.dtype == torch.float32 and mod.weight.dtype == mod.weight_shift.dtype == torch.uint8
    assert torch.equal(mod.weight, ref.weight) and torch.equal(mod.weight_shift, ref.weight_shift) and torch.equal(mod.weight_scale, ref.weight_scale)


# ---- the ABI, replayed without a device ----------------------------------------------------------------------------------------
NEW = ("hyd_linear_w4_workspace_bytes", "hyd_linear_w4", "hyd_weight_widen_w4")


def test_entry_points_are_declared_exported_and_their_mirrors_have_the_c_layout(tmp_path):
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"HYD_API \w+ {name}\(", header) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.hyd_version() == 500
    fields = {"hyd_linear_w4_params": wq.LinearW4Params, "hyd_weight_widen_w4_params": wq.WeightWidenW4Params}
    body = ""
    for cname, mirror in fields.items():
        body += f'printf("%zu ", sizeof({cname}));' + "".join(f'printf("%zu ", offsetof({cname}, {n}));' for n, _ in mirror._fields_)
    (tmp_path / "s.c").write_text('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    want = [v for mirror in fields.values() for v in [C.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]]
    assert list(map(int, subprocess.check_output([str(tmp_path / "s")]).split())) == want


def _params(cls, base, kw):
    p = cls()
    for k, v in {**base, **kw}.items():
        setattr(p, k, v)
    return p


def _linear(**kw):
    return _params(wq.LinearW4Params, dict(x=0x10000, w4=0x20000, shift=0x60000, scale=0x30000, y=0x40000, workspace=0x50000, workspace_bytes=1 << 30,
                                           M=8, N=4096, K=4096, dtype=_lib.HYD_BF16, x_row_stride=4096, y_row_stride=4096), kw)


def _widen(**kw):
    return _params(wq.WeightWidenW4Params, dict(w4=0x20000, shift=0x60000, scale=0x30000, out=0x40000, N=40, K=64, dtype=_lib.HYD_F16, out_row_stride=64), kw)


@pytest.mark.parametrize("kw, code, frag", [
    (dict(x=0), -1, "x is null"), (dict(w4=0), -1, "w4 is null"), (dict(shift=0), -1, "shift is null"), (dict(scale=0), -1, "scale is null"),
    (dict(y=0), -1, "y is null"), (dict(x=0x10008), -1, "x must be 16-byte aligned"), (dict(w4=0x20004), -1, "w4 must be 16-byte aligned"),
    (dict(shift=0x60008), -1, "shift must be 16-byte aligned"), (dict(y=0x40002), -1, "y must be 16-byte aligned"),
    (dict(scale=0x30002), -1, "scale is not aligned"), (dict(dtype=_lib.HYD_F32), -2, "dtype"), (dict(dtype=_lib.HYD_FP8_E4M3), -2, "dtype"),
    (dict(K=4112, x_row_stride=4112), -1, "multiple of 32"), (dict(K=0), -1, "must be >= 1"), (dict(N=0), -1, "must be >= 1"),
    (dict(M=0), -1, "M 0"), (dict(x_row_stride=4092), -1, "multiple of 8"), (dict(y_row_stride=4100), -1, "multiple of 8"),
    (dict(x_row_stride=4088), -1, "x_row_stride"), (dict(y_row_stride=4088), -1, "y_row_stride"),
    (dict(workspace=0), -3, "workspace"), (dict(workspace_bytes=1024), -3, "workspace bytes"), (dict(workspace=0x50008), -3, "16-byte"),
])
def test_linear_w4_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_linear_w4(C.byref(_linear(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


@pytest.mark.parametrize("kw, code, frag", [
    (dict(w4=0), -1, "w4 is null"), (dict(shift=0), -1, "shift is null"), (dict(out=0), -1, "out is null"), (dict(scale=0), -1, "scale is null"),
    (dict(out=0x40008), -1, "out must be 16-byte aligned"), (dict(shift=0x60004), -1, "shift must be 16-byte aligned"),
    (dict(dtype=_lib.HYD_F32), -2, "dtype"), (dict(K=48, out_row_stride=64), -1, "multiple of 32"), (dict(out_row_stride=68), -1, "multiple of 8"),
    (dict(out_row_stride=56), -1, "out_row_stride"), (dict(N=0), -1, "must be >= 1"),
])
def test_weight_widen_w4_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_weight_widen_w4(C.byref(_widen(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


def test_null_params_and_the_workspace_query():
    lib = _lib.load()
    assert lib.hyd_linear_w4(None, None) == -1 and "null params" in lib.hyd_last_error_string().decode()
    assert lib.hyd_weight_widen_w4(None, None) == -1 and "null params" in lib.hyd_last_error_string().decode()
    q = lib.hyd_linear_w4_workspace_bytes
    assert q(0, 64, 64) == q(1, 0, 64) == q(1, 64, 0) == 0
    assert q(16, 32, 32) == 0 and q(100, 272, 160) == 0, "a K of one step is never split"
    assert q(7, 41, 4096) == 2 * 7 * 44 * 4, "N is padded to 4 floats per slice row; 16 steps over 4 waves x 2 steps: 2 splits"
    assert q(33, 41, 4096) == 8 * 33 * 44 * 4, "more than 32 rows: the waves share the K range, 16 steps over 2 steps: 8 splits"
    b = q(8, 4096, 4096)
    assert lib.hyd_linear_w4(C.byref(_linear(workspace_bytes=b - 1)), None) == -3
