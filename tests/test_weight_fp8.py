"""-m "not gpu": fp8 linear-layer weights (hydragen_amd/weight_quant.py, csrc/linear_w8.hip) -- the quantizer against its stated
rule and its derived error bound, the fused modules of a quantized model, the model shell on the CPU (the torch definition), the
ABI bookkeeping and refusals of the new entry points replayed without a device, and the kernels' register metadata."""
import copy
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd.kv_quant import scales_from_absmax_reference
from hydragen_amd.weight_quant import Fp8Linear, dequantize_weight, linear_reference, quantize_weight

REPO = Path(__file__).resolve().parent.parent
FP8 = torch.float8_e4m3fn
MODEL_SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)]  # Llama-2-7B: q|k|v, o, gate|up, down (N, K)


def _weights(seed=0, N=48, K=96):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((N, K), generator=g) * torch.logspace(-6, 3, N)[:, None]  # rows of very different magnitude
    w[5] = 0
    w[7, 3:] = 0  # one value sets the scale
    return w


# ---- the quantizer -------------------------------------------------------------------------------------------------------------
def test_scales_are_the_kv_rule_powers_of_two_and_one_for_zero_rows():
    w = _weights()
    w8, s = quantize_weight(w)
    assert w8.dtype == FP8 and w8.shape == w.shape and s.dtype == torch.float32 and s.shape == (w.shape[0],)
    m, _ = torch.frexp(s)
    assert torch.equal(m, torch.full_like(m, 0.5)), "every scale is a power of two"
    assert torch.equal(s, scales_from_absmax_reference(w.abs().amax(1), margin=1.0, pow2=True))
    assert s[5] == 1.0 and torch.equal(w8[5].float(), torch.zeros(w.shape[1]))
    # the smallest power of two >= absmax / 448: the scale fits the row, half of it does not
    amax = w.abs().amax(1).double()
    nz = amax > 0
    assert bool((s.double()[nz] * 448 >= amax[nz] * (1 - 2.0 ** -20)).all()) and bool((s.double()[nz] * 224 < amax[nz]).all())
    assert torch.equal(w8.float(), (w / s[:, None]).clamp(-448, 448).to(FP8).float())


def test_no_nan_code_for_infinite_and_huge_inputs():
    w = _weights(1)
    w[0, 0], w[0, 1], w[1, 0], w[2, 2] = float("inf"), float("-inf"), 3e38, -3e38
    w8, s = quantize_weight(w)
    codes = w8.view(torch.uint8)
    assert not bool(((codes & 0x7F) == 0x7F).any()), "0x7f / 0xff are the NaN codes"
    d = dequantize_weight(w8, s, torch.float32)
    assert d[0, 0] == 448 * s[0] and d[0, 1] == -448 * s[0] and d[1, 0] == 448 * s[1] and d[2, 2] == -448 * s[2]
    assert s[0] == quantize_weight(_weights(1)[:1].clone().index_fill_(1, torch.tensor([0, 1]), 0.0))[1][0], "the scale comes from the finite values"
    with pytest.raises(ValueError, match="NaN"):
        quantize_weight(torch.tensor([[1.0, float("nan")]]))


def test_round_trip_is_exact_on_the_fp8_grid_and_within_the_derived_bound_off_it():
    w = _weights(2).bfloat16()
    w8, s = quantize_weight(w)
    on_grid = dequantize_weight(w8, s, torch.bfloat16)  # bf16 values that are already scale * e4m3 values
    w8b, sb = quantize_weight(on_grid)
    assert torch.equal(dequantize_weight(w8b, sb, torch.bfloat16), on_grid)
    # |deq - w| <= 2^-4 |w| + scale 2^-10: half an ulp of a normal e4m3 value (3 mantissa bits), the subnormal half step below it
    for ww in (w.float(), _weights(3)):
        q, sc = quantize_weight(ww)
        err = (dequantize_weight(q, sc, torch.float32).double() - ww.double()).abs()
        assert bool((err <= 2.0 ** -4 * ww.double().abs() + sc.double()[:, None] * 2.0 ** -10).all())


def test_linear_reference_is_the_float64_product():
    w8, s = quantize_weight(_weights(4))
    x = torch.randn((5, w8.shape[1]), generator=torch.Generator().manual_seed(5)).bfloat16()
    want = x.double() @ dequantize_weight(w8, s, torch.float64).T
    assert torch.equal(linear_reference(x, w8, s), want)


# ---- the model shell on the CPU ------------------------------------------------------------------------------------------------
def tiny_model(dtype=torch.bfloat16, device="cpu", seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=128, intermediate_size=352, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=128)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=device, seed=seed, std=0.05)


def dequantized_twin(q, ref, dtype=None):
    """`ref` (a copy of the model from before quantize_weights) with every projection's weight replaced by the dequantized
    weight of `q`'s module, in plain nn.Linear."""
    def put(lin, w):
        lin.weight.data = w.to(lin.weight.dtype if dtype is None else dtype).clone()

    for lq, lr in zip(q.model.layers, ref.model.layers):
        a, m = lq.self_attn, lq.mlp
        nq, nk = lr.self_attn.q_proj.weight.shape[0], lr.self_attn.k_proj.weight.shape[0]
        w = a.qkv_proj.dequantized(torch.float32)
        put(lr.self_attn.q_proj, w[:nq]), put(lr.self_attn.k_proj, w[nq:nq + nk]), put(lr.self_attn.v_proj, w[nq + nk:])
        put(lr.self_attn.o_proj, a.o_proj.dequantized(torch.float32))
        w = m.gate_up_proj.dequantized(torch.float32)
        put(lr.mlp.gate_proj, w[: w.shape[0] // 2]), put(lr.mlp.up_proj, w[w.shape[0] // 2:])
        put(lr.mlp.down_proj, m.down_proj.dequantized(torch.float32))
    if isinstance(q.lm_head, Fp8Linear):
        put(ref.lm_head, q.lm_head.dequantized(torch.float32))
    return ref


@pytest.fixture(scope="module")
def models():
    m = tiny_model()
    ref = copy.deepcopy(m)
    m.quantize_weights()
    return m, ref


def _layer_bytes(m):
    """Bytes of every projection of the decoder layers: parameters and buffers of the nn.Linear / Fp8Linear modules."""
    return sum(t.numel() * t.element_size() for l in m.model.layers.modules() if isinstance(l, (torch.nn.Linear, Fp8Linear))
               for t in list(l.parameters()) + list(l.buffers()))


def test_fused_modules_are_the_concatenation_of_per_projection_quantization(models):
    m, ref = models
    for lq, lr in zip(m.model.layers, ref.model.layers):
        for fused, names, owner in ((lq.self_attn.qkv_proj, ("q_proj", "k_proj", "v_proj"), lr.self_attn),
                                    (lq.mlp.gate_up_proj, ("gate_proj", "up_proj"), lr.mlp)):
            pairs = [quantize_weight(getattr(owner, n).weight) for n in names]
            assert torch.equal(fused.weight.view(torch.uint8), torch.cat([p[0] for p in pairs]).view(torch.uint8))
            assert torch.equal(fused.weight_scale, torch.cat([p[1] for p in pairs]))
        assert lq.self_attn.q_proj is None and lq.self_attn.k_proj is None and lq.self_attn.v_proj is None
        assert lq.mlp.gate_proj is None and lq.mlp.up_proj is None
        assert isinstance(lq.self_attn.o_proj, Fp8Linear) and isinstance(lq.mlp.down_proj, Fp8Linear)
    assert isinstance(m.lm_head, torch.nn.Linear) and m.lm_head.weight.dtype == torch.bfloat16, "lm_head is skipped by default"
    assert m.model.embed_tokens.weight.dtype == torch.bfloat16


def test_quantize_weights_halves_the_layers_bytes(models):
    m, ref = models
    c = m.config
    n_out = 3 * c.hidden_size + c.hidden_size + 2 * c.intermediate_size + c.hidden_size  # output channels per layer: one fp32 scale each
    n_w = 4 * c.hidden_size * c.hidden_size + 3 * c.hidden_size * c.intermediate_size
    assert _layer_bytes(ref) == c.num_hidden_layers * 2 * n_w
    assert _layer_bytes(m) == c.num_hidden_layers * (n_w + 4 * n_out)


def test_forward_equals_the_model_on_dequantized_16_bit_weights(models):
    m, ref = models
    twin = dequantized_twin(m, copy.deepcopy(ref))
    for mm in (m, twin):  # the layers without attention kernels: projections, RoPE, norms, MLP -- all torch on the CPU
        mm.model.set_disable_hydragen(True)
        mm.model.set_disable_attention(True)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 512, (3, 9), generator=g)
    pos = torch.arange(9)[None].expand(3, 9)
    with torch.no_grad():
        got, want = m(ids, pos, full_logits=True), twin(ids, pos, full_logits=True)
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_lm_head_is_quantized_when_not_skipped_and_unknown_names_are_refused():
    m = tiny_model(seed=3)
    with pytest.raises(ValueError, match="unknown"):
        m.quantize_weights(skip=("lm_head", "embed"))
    with pytest.raises(NotImplementedError):
        m.quantize_weights(dtype=torch.float8_e5m2)
    m.quantize_weights(skip=())
    assert isinstance(m.lm_head, Fp8Linear) and m.lm_head.weight.dtype == FP8
    assert m.model.embed_tokens.weight.dtype == torch.bfloat16


def test_state_dict_round_trip_is_exact(models):
    m, _ = models
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    keys = [k for k in sd if "layers.0." in k]
    for stem in ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj"):
        assert f"model.layers.0.{stem}.weight" in keys and f"model.layers.0.{stem}.weight_scale" in keys
    assert sd["model.layers.0.self_attn.qkv_proj.weight"].dtype == FP8
    other = tiny_model(seed=7)
    other.quantize_weights()
    assert not torch.equal(other.model.layers[0].mlp.down_proj.weight.view(torch.uint8), m.model.layers[0].mlp.down_proj.weight.view(torch.uint8))
    other.load_state_dict(sd)
    got = other.state_dict()
    assert got.keys() == sd.keys()
    for k, v in sd.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k].view(torch.uint8) if v.dtype == FP8 else got[k], v.view(torch.uint8) if v.dtype == FP8 else v), k


def test_a_dtype_cast_keeps_codes_and_scales_and_sets_the_activation_dtype():
    lin = torch.nn.Linear(64, 40, bias=True).bfloat16()
    mod = Fp8Linear.from_linears((lin,))
    codes, scale = mod.weight.view(torch.uint8).clone(), mod.weight_scale.clone()
    x = torch.randn((3, 64), generator=torch.Generator().manual_seed(0))
    for dtype in (torch.float16, torch.float32):
        mod.to(dtype)
        assert mod.weight.dtype == FP8 and torch.equal(mod.weight.view(torch.uint8), codes)
        assert mod.weight_scale.dtype == torch.float32 and torch.equal(mod.weight_scale, scale)
        assert mod.dtype == dtype and mod.bias.dtype == dtype
        want = torch.nn.functional.linear(x.to(dtype), dequantize_weight(mod.weight, scale, dtype), mod.bias)
        assert torch.equal(mod(x.to(dtype)), want)


def test_second_call_and_tensor_parallel_sharding_afterwards_raise(models):
    from hydragen_amd.tp import apply_tp, make_tp_files

    m, _ = models
    with pytest.raises(RuntimeError, match="already"):
        m.quantize_weights()
    with pytest.raises(RuntimeError, match="fp8 weights"):
        apply_tp(m, rank=0, world_size=2)
    with pytest.raises(RuntimeError, match="fp8 weights"):
        make_tp_files(m, "/nonexistent-never-created", num_splits=2)


def test_quantizing_a_tensor_parallel_shard_quantizes_the_shard():
    from hydragen_amd.tp import apply_tp

    m = tiny_model(seed=4)
    full = copy.deepcopy(m)
    apply_tp(m, rank=1, world_size=2)
    m.quantize_weights()
    a, f = m.model.layers[0].self_attn, full.model.layers[0].self_attn
    assert a.qkv_proj.weight.shape == (3 * 64, 128) and a.o_proj.weight.shape == (128, 64)
    assert torch.equal(a.qkv_proj.weight[:64].view(torch.uint8), quantize_weight(f.q_proj.weight[64:])[0].view(torch.uint8))
    assert torch.equal(a.o_proj.weight.view(torch.uint8), quantize_weight(f.o_proj.weight[:, 64:])[0].view(torch.uint8))


# ---- the ABI, replayed without a device ----------------------------------------------------------------------------------------
def test_entry_points_are_declared_mirrored_and_exported():
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    for decl in (r"HYD_API size_t hyd_linear_w8_workspace_bytes\(int32_t M, int32_t N, int32_t K\);",
                 r"HYD_API int hyd_linear_w8\(const hyd_linear_w8_params\* p, void\* stream\);",
                 r"HYD_API int hyd_weight_widen\(const hyd_weight_widen_params\* p, void\* stream\);"):
        assert re.search(decl, header), decl
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(_lib.lib_path())], text=True)
    for name in ("hyd_linear_w8", "hyd_linear_w8_workspace_bytes", "hyd_weight_widen"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert any(ln.split()[-1] == name and " T " in ln for ln in out.splitlines())
    assert lib.hyd_version() == 500


def test_struct_layouts_match_the_c_compiler(tmp_path):
    fields = {"hyd_linear_w8_params": _lib.LinearW8Params, "hyd_weight_widen_params": _lib.WeightWidenParams}
    body = ""
    for cname, mirror in fields.items():
        body += f'printf("%zu ", sizeof({cname}));' + "".join(f'printf("%zu ", offsetof({cname}, {n}));' for n, _ in mirror._fields_)
    (tmp_path / "s.c").write_text('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "s")]).split()))
    want = []
    for mirror in fields.values():
        want += [C.sizeof(mirror)] + [getattr(mirror, n).offset for n, _ in mirror._fields_]
    assert got == want


def _linear(**kw):
    p = _lib.LinearW8Params()
    p.x, p.w8, p.scale, p.y, p.workspace, p.workspace_bytes = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 1 << 30
    p.M, p.N, p.K, p.dtype, p.x_row_stride, p.y_row_stride = 8, 4096, 4096, _lib.HYD_BF16, 4096, 4096
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _widen(**kw):
    p = _lib.WeightWidenParams()
    p.w8, p.scale, p.out, p.N, p.K, p.dtype, p.out_row_stride = 0x20000, 0x30000, 0x40000, 40, 64, _lib.HYD_F16, 64
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code, frag", [
    (dict(x=0), -1, "x is null"), (dict(w8=0), -1, "w8 is null"), (dict(scale=0), -1, "scale is null"), (dict(y=0), -1, "y is null"),
    (dict(x=0x10008), -1, "x must be 16-byte aligned"), (dict(w8=0x20004), -1, "w8 must be 16-byte aligned"),
    (dict(y=0x40002), -1, "y must be 16-byte aligned"), (dict(scale=0x30002), -1, "scale is not aligned"),
    (dict(dtype=_lib.HYD_F32), -2, "dtype"), (dict(dtype=_lib.HYD_FP8_E4M3), -2, "dtype"),
    (dict(K=4104, x_row_stride=4104), -1, "multiple of 16"), (dict(K=0), -1, "must be >= 1"), (dict(N=0), -1, "must be >= 1"),
    (dict(M=0), -1, "M 0"), (dict(x_row_stride=4092), -1, "multiple of 8"), (dict(y_row_stride=4100), -1, "multiple of 8"),
    (dict(x_row_stride=4088), -1, "x_row_stride"), (dict(y_row_stride=4088), -1, "y_row_stride"),
    (dict(workspace=0), -3, "workspace"), (dict(workspace_bytes=1024), -3, "workspace bytes"), (dict(workspace=0x50008), -3, "16-byte"),
])
def test_linear_w8_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_linear_w8(C.byref(_linear(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


@pytest.mark.parametrize("kw, code, frag", [
    (dict(w8=0), -1, "w8 is null"), (dict(out=0), -1, "out is null"), (dict(scale=0), -1, "scale is null"),
    (dict(out=0x40008), -1, "out must be 16-byte aligned"), (dict(dtype=_lib.HYD_F32), -2, "dtype"),
    (dict(K=60, out_row_stride=64), -1, "multiple of 8"), (dict(out_row_stride=60), -1, "multiple of 8"),
    (dict(out_row_stride=56), -1, "out_row_stride"), (dict(N=0), -1, "must be >= 1"),
])
def test_weight_widen_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_weight_widen(C.byref(_widen(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


def test_null_params_are_refused():
    lib = _lib.load()
    assert lib.hyd_linear_w8(None, None) == -1 and "null params" in lib.hyd_last_error_string().decode()
    assert lib.hyd_weight_widen(None, None) == -1 and "null params" in lib.hyd_last_error_string().decode()


def test_workspace_query_covers_the_model_shapes_and_is_zero_without_a_split():
    """The plan is shapes-only.  Split slices are fp32 [M, N rounded up to 4]: the query is a whole number of them, at least two
    when it is not zero; a call with one byte less is refused.  The widest shape (gate|up) fills the chip on its own at one row and
    at 256, and so does q|k|v at 512 rows: no split, no workspace."""
    lib = _lib.load()
    q = lib.hyd_linear_w8_workspace_bytes
    assert q(1, 22016, 4096) == 0 and q(256, 22016, 4096) == 0 and q(512, 12288, 4096) == 0
    assert q(16, 32, 16) == 0 and q(1, 1, 16) == 0 and q(100, 272, 80) == 0, "a K of one step is never split"
    assert q(0, 4096, 4096) == 0 and q(1, 0, 4096) == 0 and q(1, 4096, 0) == 0
    for N, K in MODEL_SHAPES:
        for M in (1, 256):
            b = q(M, N, K)
            slice_bytes = M * ((N + 3) // 4 * 4) * 4
            assert b % slice_bytes == 0 and b // slice_bytes != 1 and b // slice_bytes <= 16, (M, N, K, b)
            if b:
                assert lib.hyd_linear_w8(C.byref(_linear(M=M, N=N, K=K, x_row_stride=K, y_row_stride=N, workspace_bytes=b - 1)), None) == -3
    assert q(1, 4096, 4096) > 0 and q(1, 4096, 11008) > 0 and q(1, 12288, 4096) > 0, "the narrow shapes split at one row"
    assert q(7, 41, 4096) == 4 * 7 * 44 * 4, "N is padded to 4 floats per slice row; 32 steps over 4 waves x 2 steps: 4 splits"
    assert q(33, 41, 4096) == 16 * 33 * 44 * 4, "more than 32 rows: the waves share the K range, 32 steps over 2 steps: 16 splits"


# ---- build quality -------------------------------------------------------------------------------------------------------------
VGPR_BUDGET = [(r"linear_w8_kernelINS_\w+ELi1E", 128), (r"linear_w8_kernelINS_\w+ELi2E", 128), (r"linear_w8_rows_kernelINS_\w+ELi4E", 168),
               (r"linear_w8_rows_kernelINS_\w+ELi8E", 256), (r"linear_w8_reduce_kernel", 32), (r"weight_widen_kernel", 64)]


def test_linear_w8_kernels_have_no_scratch_no_spills_and_stay_in_their_vgpr_budget():
    from tests.test_build_quality import HIPCC, _metadata

    if not Path(HIPCC).exists():
        pytest.skip("hipcc not installed")
    src, kernels = _metadata("linear_w8.hip")
    assert len(kernels) == 12, [k["name"] for k in kernels]  # 2 dtypes x (2 + 2 row tilings + reduce) + 2 widen
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        lims = [lim for pat, lim in VGPR_BUDGET if re.search(pat, k["name"])]
        assert len(lims) == 1 and k["vgpr"] <= lims[0], k
