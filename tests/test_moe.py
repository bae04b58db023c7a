"""-m "not gpu": the mixture-of-experts definition and its error bound (hydragen_amd/moe.py) -- the tie rule on hand-made rows, an fp32
evaluation in a kernel's order of operations inside the bound, and transformers' own Mixtral / Qwen3-MoE blocks against the definition
(weight layouts and routing semantics)."""
import pytest
import torch

from hydragen_amd import moe

T, H, I, E, K = 33, 64, 48, 4, 2


def test_routing_definition_on_hand_made_rows():
    logits = torch.tensor([[1.0, 3.0, 3.0, 0.5], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]])
    ids, w = moe.route_reference(logits, 2, True)
    assert ids.tolist() == [[1, 2], [0, 1], [2, 3]], "descending, equal logits to the lower index"
    assert w.dtype == torch.float64 and torch.allclose(w.sum(1), torch.ones(3, dtype=torch.float64), rtol=0, atol=1e-15)
    ids, w = moe.route_reference(logits, 4, False)  # k = E: the whole softmax, sorted
    assert ids.tolist() == [[1, 2, 0, 3], [0, 1, 2, 3], [2, 3, 0, 1]]
    assert torch.equal(w, torch.softmax(logits.double(), 1).gather(1, ids)) and torch.allclose(w.sum(1), torch.ones(3, dtype=torch.float64))
    assert float(moe.route_reference(logits, 2, False)[1][0].sum()) < 1
    with pytest.raises(ValueError):
        moe.route_reference(logits, 5, True)


def _inputs(dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(s, generator=g) * sd).to(dtype) for s, sd in (((T, H), 1.0), ((E, H), 0.1), ((E, 2 * I, H), 0.1), ((E, H, I), 0.1)))


def _emulate_fp32(x, router, gate_up, down, k, renorm):
    """What a kernel computes, in its order and precisions, on the host: the 16-bit router logits the definition routes by (so the
    route is the definition's by construction), fp32 softmax weights, fp32 products, act rounded to 16 bits, the weighted rows added
    in j order, one rounding."""
    logits = torch.nn.functional.linear(x, router)
    ids = moe.route_reference(logits, k, renorm)[0]
    w = torch.softmax(logits.float(), dim=1).gather(1, ids)
    w = w / w.sum(1, keepdim=True) if renorm else w
    out = torch.zeros(x.shape)
    for j in range(k):
        gu = torch.einsum("th,tnh->tn", x.float(), gate_up.float()[ids[:, j]])
        act = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]).to(x.dtype).float()
        out += torch.einsum("ti,thi->th", act, down.float()[ids[:, j]]) * w[:, j, None]
    return out.to(x.dtype).double()


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_fp32_emulation_of_a_kernel_is_inside_the_bound_and_a_swapped_layout_far_outside(dtype, renorm):
    """The bound is derived, not measured: the fp32 evaluation has to fit.  It must not be vacuous either: it is u16 (|y| + the sum of
    absolute products, about sqrt(I) |y| for random signs) plus fp32 terms, a few per cent of |y| in bfloat16; and up rows in front of
    gate rows must miss it by orders of magnitude."""
    x, router, gate_up, down = _inputs(dtype)
    ref, bound = moe.moe_reference(x, router, gate_up, down, K, renorm), moe.moe_error_bound(x, router, gate_up, down, K, renorm)
    err = (_emulate_fp32(x, router, gate_up, down, K, renorm) - ref).abs()
    print(f"{dtype} renorm={renorm}: max err / bound {float((err / bound).max()):.3f}, median bound / |ref| {float((bound / ref.abs()).median()):.4f}")
    assert float(ref.abs().max()) > 0.01 and bool((err <= bound).all())
    u16 = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert float((bound / ref.abs()).median()) < u16 * (2 + 2 * I ** 0.5)
    swapped = torch.cat([gate_up[:, I:], gate_up[:, :I]], 1)
    assert float(((_emulate_fp32(x, router, swapped, down, K, renorm) - ref).abs() / bound).max()) > 100


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_transformers_blocks_compute_the_definition(kind):
    """transformers' own sparse blocks in bfloat16 on the CPU against moe_reference on their weights: parameter layout (gate rows,
    then up rows), top-k order and the renormalisation switch.  The router's F.linear is the same call in both, so the logits agree
    bit for bit; rows whose k + 1 largest logits hold a tie are taken out of x beforehand (there the two tie rules may differ: the
    docstring of route_reference), so the routes agree by construction.  transformers rounds about eight times to bfloat16 where the
    definition rounds twice, so the outputs agree to a few per cent (mean relative difference < 0.05; the Qwen3 golden test allows
    0.15 for a whole model), and a swapped layout is off by order one."""
    tf = pytest.importorskip("transformers")
    kw = dict(hidden_size=H, intermediate_size=I, num_experts_per_tok=K, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=32)
    if kind == "mixtral":
        from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock as Block
        cfg, renorm = tf.MixtralConfig(num_local_experts=E, **kw), True
    else:
        from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeSparseMoeBlock as Block
        cfg, renorm = tf.Qwen3MoeConfig(num_experts=E, moe_intermediate_size=I, norm_topk_prob=False, **kw), False
    x, router, gate_up, down = _inputs(torch.bfloat16, seed=11)
    block = Block(cfg).to(torch.bfloat16).eval()
    block.load_state_dict({"gate.weight": router, "experts.gate_up_proj": gate_up, "experts.down_proj": down})
    top = torch.sort(torch.nn.functional.linear(x, router).float(), dim=1, descending=True).values[:, : K + 1]
    x = x[(top[:, :-1] > top[:, 1:]).all(1)]
    assert x.shape[0] > T // 2
    with torch.no_grad():
        _, scores, indices = block.gate(x)
        ids, w = moe.route_reference(torch.nn.functional.linear(x, router), K, renorm)
        assert torch.equal(indices, ids) and torch.allclose(scores.double(), w, rtol=2.0 ** -7, atol=0)
        got = block(x[None])[0].double()
    rdiff = lambda a, b: float((2 * (a - b).abs() / (a.abs() + b.abs() + 1e-8)).mean())  # noqa: E731
    ref = moe.moe_reference(x, router, gate_up, down, K, renorm)
    print(f"{kind}: mean relative difference {rdiff(got, ref):.4f}")
    assert rdiff(got, ref) < 0.05
    assert rdiff(got, moe.moe_reference(x, router, torch.cat([gate_up[:, I:], gate_up[:, :I]], 1), down, K, renorm)) > 0.5
