"""-m "not gpu": the mixture-of-experts entry points without a device (hyd_moe_mlp's refusals, the workspace formula, the ctypes
mirror), from_hf_model on tiny Mixtral / Qwen3-MoE models on the CPU, and the register allocation of csrc/moe.hip."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, moe

REPO = Path(__file__).resolve().parent.parent


def tiny_hf(kind, **over):
    """A one-layer transformers model with experts: H 64, one 64-wide head, E 4, k 2, vocab 32; I 48 -> 64 (the kernels' I % 32)."""
    tf = pytest.importorskip("transformers")
    kw = dict(hidden_size=64, num_experts_per_tok=2, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1, head_dim=64, vocab_size=32,
              max_position_embeddings=128, sliding_window=None)
    if kind == "mixtral":
        cfg = tf.MixtralConfig(num_local_experts=4, intermediate_size=64, **{**kw, **over})
    else:
        cfg = tf.Qwen3MoeConfig(num_experts=4, moe_intermediate_size=64, intermediate_size=96, norm_topk_prob=False, **{**kw, **over})
    torch.manual_seed(3)
    return tf.AutoModelForCausalLM.from_config(cfg).to(torch.bfloat16).eval()


def test_mirror_has_the_c_layout_and_the_entry_points_are_exported(tmp_path):
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    lib = _lib.load()
    for name in ("hyd_moe_workspace_bytes", "hyd_moe_mlp"):
        assert re.search(rf"HYD_API \w+ {name}\(", header) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.hyd_version() == 500 and f"#define HYD_MOE_MAX_ROWS {moe.MOE_MAX_ROWS}\n" in header
    body = 'printf("%zu ", sizeof(hyd_moe_params));' + "".join(f'printf("%zu ", offsetof(hyd_moe_params, {n}));' for n, _ in moe.MoeParams._fields_)
    (tmp_path / "s.c").write_text('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    want = [C.sizeof(moe.MoeParams)] + [getattr(moe.MoeParams, n).offset for n, _ in moe.MoeParams._fields_]
    assert list(map(int, subprocess.check_output([str(tmp_path / "s")]).split())) == want


def _params(**kw):
    p = moe.MoeParams()
    base = dict(x=0x10000, logits=0x20000, gate_up=0x30000, down=0x40000, y=0x50000, workspace=0x60000, workspace_bytes=1 << 30, T=8, E=8, k=2, H=128,
                I=64, renormalize=1, dtype=_lib.HYD_BF16, x_row_stride=128, y_row_stride=128)
    for k, v in {**base, **kw}.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code, frag", [
    (dict(T=129), -1, "T 129"), (dict(T=0), -1, "T 0"), (dict(E=257, k=8), -1, "E 257"), (dict(k=9, E=16), -1, "k 9"), (dict(k=3, E=2), -1, "k 3 exceeds E 2"),
    (dict(H=96, x_row_stride=96, y_row_stride=96), -1, "H 96"), (dict(I=48), -1, "I 48"), (dict(gate_up=0x30008), -1, "gate_up must be 16-byte aligned"),
    (dict(down=0x40004), -1, "down must be 16-byte aligned"), (dict(workspace_bytes=1024), -3, "workspace bytes"), (dict(workspace=0), -3, "workspace"),
    (dict(workspace=0x60008), -3, "16-byte"), (dict(x=0), -1, "x is null"), (dict(logits=0), -1, "logits is null"), (dict(y=0x50002), -1, "y must be 16-byte"),
    (dict(dtype=_lib.HYD_F32), -2, "dtype"), (dict(x_row_stride=64), -1, "x_row_stride"), (dict(y_row_stride=132), -1, "multiple of 8"),
    (dict(renormalize=2), -1, "renormalize"), (dict(weights_out=0x70002), -1, "not aligned"),
])
def test_refusals_come_with_their_message_before_any_launch(kw, code, frag):
    lib = _lib.load()
    assert lib.hyd_moe_mlp(C.byref(_params(**kw)), None) == code
    assert frag in lib.hyd_last_error_string().decode()


def test_null_params_and_the_workspace_formula():
    lib = _lib.load()
    assert lib.hyd_moe_mlp(None, None) == -1 and "null params" in lib.hyd_last_error_string().decode()
    q, r16 = lib.hyd_moe_workspace_bytes, lambda n: (n + 15) // 16 * 16
    for T, E, k, H, I in ((1, 4, 1, 64, 32), (33, 200, 8, 192, 96), (128, 8, 2, 4096, 14336), (128, 256, 8, 2048, 768)):
        n = T * k  # ids, weights, counts, offsets, slots, act, yslot: each slice rounded up to 16 bytes
        want = 3 * r16(4 * n) + r16(4 * E) + r16(4 * (E + 1)) + r16(2 * n * I) + r16(4 * n * H)
        assert q(T, E, k, H, I, _lib.HYD_BF16) == q(T, E, k, H, I, _lib.HYD_F16) == want
    assert q(129, 8, 2, 64, 32, 1) == q(8, 257, 2, 64, 32, 1) == q(8, 8, 9, 64, 32, 1) == q(8, 2, 3, 64, 32, 1) == q(8, 8, 2, 96, 32, 1) == q(8, 8, 2, 64, 48, 1) == 0
    assert q(8, 8, 2, 64, 32, _lib.HYD_F32) == 0
    assert lib.hyd_moe_mlp(C.byref(_params(workspace_bytes=q(8, 8, 2, 128, 64, 1) - 1)), None) == -3


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_from_hf_model_builds_the_experts_and_the_cpu_forward_is_the_definition(kind):
    from hydragen_amd import tp
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    hf = tiny_hf(kind)
    m = HydragenLlamaForCausalLM.from_hf_model(hf)
    c, mlp = m.config, m.model.layers[0].mlp
    assert (c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size, c.norm_topk_prob, c.qk_norm) == (4, 2, 64, kind == "mixtral", kind == "qwen3_moe")
    assert isinstance(mlp, moe.MoeMLP) and (mlp.top_k, mlp.renormalize) == (2, kind == "mixtral")
    sd = hf.state_dict()
    args = [sd[f"model.layers.0.mlp.{n}"] for n in ("gate.weight", "experts.gate_up_proj", "experts.down_proj")]
    assert all(torch.equal(a, b) for a, b in zip(args, (mlp.gate.weight, mlp.experts.gate_up_proj, mlp.experts.down_proj)))
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    with torch.no_grad():
        got = mlp(x)
    assert got.shape == x.shape and torch.equal(got.view(10, 64), moe.moe_reference(x.view(10, 64), *args, 2, kind == "mixtral").to(torch.bfloat16))
    for call in (lambda: tp.apply_tp(m, 0, 2), lambda: tp.make_tp_files(m, "unused", 2), m.quantize_weights):
        with pytest.raises(NotImplementedError, match="experts"):
            call()


def test_from_hf_model_refuses_what_the_shell_does_not_run():
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    with pytest.raises(NotImplementedError, match="sliding_window"):
        HydragenLlamaForCausalLM.from_hf_model(tiny_hf("mixtral", sliding_window=16))
    with pytest.raises(NotImplementedError, match="mlp_only_layers"):
        HydragenLlamaForCausalLM.from_hf_model(tiny_hf("qwen3_moe", mlp_only_layers=[0]))


# unified VGPRs (arch + accumulator) as built, rounded up to the next allocation step of 8 and one step of slack: DESIGN 4.23
VGPR_BUDGET = [(r"moe_route_kernel", 48), (r"moe_group_kernel", 40), (r"moe_gate_up_kernelINS_\w+ELi1E", 104), (r"moe_gate_up_kernelINS_\w+ELi2E", 152),
               (r"moe_down_kernelINS_\w+ELi1E", 104), (r"moe_down_kernelINS_\w+ELi2E", 152), (r"moe_combine_kernel", 32)]


def test_moe_kernels_have_no_scratch_no_spills_and_stay_in_their_vgpr_budget():
    from tests.test_build_quality import HIPCC, _metadata

    if not Path(HIPCC).exists():
        pytest.skip("hipcc not installed")
    _, kernels = _metadata("moe.hip")
    assert len(kernels) == 13, [k["name"] for k in kernels]  # group + 2 dtypes x (route, combine, 2 tilings x (gate_up, down))
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        lims = [lim for pat, lim in VGPR_BUDGET if re.search(pat, k["name"])]
        assert len(lims) == 1 and k["vgpr"] <= lims[0], k
