"""-m gpu: the fp8 expert kernels (csrc/moe_w8.hip through hydragen_amd/moe.py) against the float64 definition on the dequantized weights
and its bound, every e4m3 code at every byte of a lane's step, buffers, chunked calls, and quantize_experts() models through the shell."""
import copy

import pytest
import torch

from hydragen_amd import _lib, moe
from tests.test_moe_abi import tiny_hf
from tests.test_moe_gpu import IDS, crafted_logits, inputs
from tests.test_weight_fp8_gpu import DEV, DTYPES, GUARD, SENT16

pytestmark = pytest.mark.gpu


def run(x, logits, q, k, renorm, **kw):
    return moe.moe_rows_w8(x, logits, *q, k, renorm, torch.empty_like(x), **kw)


def ratio_to_bound(y, x, logits, q, k, gate_up=None):  # max |y - moe_reference| / moe_error_bound on the dequantized weights (gate_up: a map of them)
    gu, dn = moe.dequantize_experts(*(t.cpu() for t in q))
    args = (x.cpu(), x.new_zeros((gu.shape[0], x.shape[1])).cpu(), gu if gate_up is None else gate_up(gu), dn, k, True)
    ref, bound = moe.moe_reference(*args, logits=logits.cpu()), moe.moe_error_bound(*args, logits=logits.cpu())
    return float(((y.cpu().double() - ref).abs() / bound).max()), float(ref.abs().max())


@pytest.mark.parametrize("variant", ["random", "same", 16, 17])
@pytest.mark.parametrize("I", [32, 96, 160])
@pytest.mark.parametrize("H", [64, 192, 320])
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mlp_is_inside_the_error_bound_of_the_definition(dtype, E, k, H, I, variant):
    """|y - moe_reference(dequantized)| <= moe_error_bound(dequantized) elementwise, routed by the device's logits, no row left out.  H = 64:
    half a step; 192, 320: uneven splits with a half-step tail; I = 160: a step and a quarter.  A gate/up swap misses by > 100 bounds."""
    for T in (1, 17, 128):
        x, router, gate_up, down = inputs(T, E, H, I, dtype, 7 * T + E)
        q = moe.quantize_experts(gate_up, down)
        logits = crafted_logits(torch.nn.functional.linear(x, router), variant, k)
        y = run(x, logits, q, k, True)
        ratio, top = ratio_to_bound(y, x, logits, q, k)
        print(f"T {T}: max err / bound {ratio:.3f}")
        assert top > 0.01 and ratio <= 1, T
    assert ratio_to_bound(y, x, logits, q, k, gate_up=lambda w: torch.cat([w[:, I:], w[:, :I]], 1))[0] > 100


def test_every_code_at_every_byte_position_of_a_step():
    """f16, 512 rows in four calls.  Row t holds one non-zero element, at kt = t % 256, and chooses experts 8 (t // 32) .. + 7 with equal
    weights; expert e's up matrix has one non-zero row n_e = e % 32.  So g, u and the down sum of a slot are single products: of the gate
    code (e + kt) % 128 and the (negative) up code of the mirrored magnitude at byte kt % 32 of a lane's step, and of the down codes
    (h + n_e) % 256 at byte n_e: over the rows, every finite code at each of a step's 32 bytes in both products.  A wrong code or byte
    moves a term by >= 2^-4 relative, 2^-8 of a row's sum, against a bound near 2^-10."""
    T, E, k, H, I = 512, 128, 8, 256, 32
    finite = lambda c: torch.where(c % 128 == 127, c - 1, c)  # noqa: E731  (0x7f and 0xff are the NaN codes)
    e, n, kk, h = torch.arange(E), torch.arange(I), torch.arange(H), torch.arange(H)
    cg = finite((e[:, None] + kk[None]) % 128)  # [E, H]
    gu8 = torch.zeros(E, 2 * I, H, dtype=torch.uint8)
    gu8[:, :I] = cg[:, None]
    gu8[e, I + e % 32] = ((126 - cg) | 0x80).to(torch.uint8)
    dn8 = finite((h[:, None] + n[None]) % 256).to(torch.uint8).expand(E, H, I).contiguous()
    gus = torch.ldexp(torch.ones(E, 2 * I), (e[:, None] + torch.arange(2 * I)[None]) % 3 - 1)
    dns = torch.ldexp(torch.ones(E, H), -((e[:, None] + h[None]) % 4))
    t, x = torch.arange(T), torch.zeros(T, H, dtype=torch.float16)
    x[t, t % 256] = 1.25
    chosen = 8 * (t // 32)[:, None] + torch.arange(k)[None]  # [T, k]
    logits = torch.full((T, E), -10.0, dtype=torch.float16).scatter_(1, chosen, 10.0)
    q = [a.to(DEV) for a in (gu8.view(torch.float8_e4m3fn), gus, dn8.view(torch.float8_e4m3fn), dns)]
    y = torch.cat([run(x[r:r + 128].to(DEV), logits[r:r + 128].to(DEV), q, k, True) for r in range(0, T, 128)])
    ratio, top = ratio_to_bound(y, x, logits, q, k)
    print(f"max err / bound {ratio:.3f}, max |ref| {top:.1f}")
    assert top > 100 and ratio <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_buffers_stay_intact_calls_repeat_rows_are_independent_and_waves_take_several_steps(dtype):
    """H = 704: 1, 2, 1, 2 steps per wave, I = 544: 1, 1, 1, 2 -- the bound test's shapes never reach a wave's second step (prefetched registers)."""
    T, E, k, H, I = 33, 8, 2, 704, 544
    x, router, gate_up, down = inputs(T, E, H, I, dtype, 5)
    q = moe.quantize_experts(gate_up, down)
    need = int(_lib.load().hyd_moe_workspace_bytes(T, E, k, H, I, _lib.HYD_F16 if dtype == torch.float16 else _lib.HYD_BF16))

    def call(x):
        yb = torch.full((T + 2, H + 24), SENT16, dtype=dtype, device=DEV)
        wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        moe.moe_rows_w8(x, torch.nn.functional.linear(x, router), *q, k, True, yb[1:T + 1, 8:8 + H], workspace=wsb[GUARD:GUARD + need])
        torch.cuda.synchronize()
        assert bool((yb[0] == SENT16).all()) and bool((yb[T + 1] == SENT16).all()) and bool((yb[:, :8] == SENT16).all()) and bool((yb[:, 8 + H:] == SENT16).all())
        assert bool((wsb[:GUARD] == 0xA5).all()) and bool((wsb[GUARD + need:] == 0xA5).all()), "bytes around the workspace were written"
        return yb[1:T + 1, 8:8 + H].clone()

    y = call(x)
    assert torch.equal(y, call(x)) and ratio_to_bound(y, x, torch.nn.functional.linear(x, router), q, k)[0] <= 1
    yn = call(x.index_fill(0, torch.tensor([5], device=DEV), float("nan")))
    assert torch.equal(yn[:5], y[:5]) and torch.equal(yn[6:], y[6:]) and bool(torch.isnan(yn[5]).all())


def test_long_calls_are_the_chunk_calls():
    T, E, k, H, I = 300, 8, 2, 64, 32
    x, router, gate_up, down = inputs(T, E, H, I, torch.bfloat16, 9)
    q = moe.quantize_experts(gate_up, down)
    y, ids, w = moe.moe_mlp(x.view(3, 100, H), router, q[0], q[2], k, True, return_routing=True, gate_up_scale=q[1], down_scale=q[3])
    logits = torch.nn.functional.linear(x, router)
    for rows in (slice(0, 128), slice(128, 256), slice(256, 300)):
        ic, wc = (torch.empty((rows.stop - rows.start, k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32))
        yc = run(x[rows], logits[rows], q, k, True, ids_out=ic, weights_out=wc)
        assert torch.equal(y.view(T, H)[rows], yc) and torch.equal(ids[rows], ic) and torch.equal(w[rows], wc)
    assert y.shape == (3, 100, H) and torch.equal(ids.cpu().long(), moe.route_reference(logits.cpu(), k, True)[0])


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_models_with_fp8_experts_run_through_the_shell(kind):
    """quantize_experts() on a one-layer model, generate() with the graph off and on: the same tokens, and logits within test_moe_gpu.py's
    0.15 (mean relative difference) of transformers' bf16 forward of the same model with its experts replaced by their dequantized values."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    hf = tiny_hf(kind)
    model = HydragenLlamaForCausalLM.from_hf_model(copy.deepcopy(hf).to(DEV))
    model.quantize_experts()
    e, he = model.model.layers[0].mlp.experts, hf.model.layers[0].mlp.experts
    he.gate_up_proj.data, he.down_proj.data = moe.dequantize_experts(*(b.cpu() for b in e.buffers()), dtype=torch.bfloat16)
    prompt = torch.randint(1, 32, (1, 12), generator=torch.Generator().manual_seed(2))
    new, runs = 4, []
    for graph in (False, True):
        model.graph(graph)
        model.setup_caches(max_unique_batch_size=2, max_unique_seq_length=16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[12])
        out, logits = model.generate(input_ids=[prompt.to(DEV)], num_return_sequences=2, max_new_tokens=new, temperature=0.0, return_logits=True)
        runs.append((out.cpu(), torch.stack(list(logits), 1).float().cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][0].shape == (2, new)
    with torch.no_grad():
        want = hf(torch.cat([prompt, runs[0][0][:1, : new - 1]], 1)).logits[0, -new:].float()
    rdiff = lambda a, b: float((2 * (a - b).abs() / (a.abs() + b.abs() + 1e-8)).mean())  # noqa: E731
    for out, got in runs:
        print(f"{kind}: mean relative difference to transformers on the dequantized experts {rdiff(got[0], want):.4f}")
        assert rdiff(got[0], want) < 0.15
