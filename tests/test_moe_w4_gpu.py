"""-m gpu: the 4-bit expert kernels (csrc/moe_w4.hip) against the float64 definition and its bound, crafted codes and shifts, buffers, chunks, the shell."""
import copy

import pytest
import torch

from hydragen_amd import _lib, moe
from hydragen_amd.weight_quant import FP4_DTYPE
from tests.test_moe_abi import tiny_hf
from tests.test_moe_gpu import IDS, crafted_logits, inputs
from tests.test_weight_fp8_gpu import DEV, DTYPES, GUARD, SENT16

pytestmark = pytest.mark.gpu


def run(x, logits, q, k, renorm, **kw):
    return moe.moe_rows_w4(x, logits, *q, k, renorm, torch.empty_like(x), **kw)


def ratio_to_bound(y, x, logits, q, k, gate_up=None):  # max |y - moe_reference| / moe_error_bound on the dequantized weights (gate_up: a map of them)
    gu, dn = moe.dequantize_experts_fp4(*(t.cpu() for t in q))
    args = (x.cpu(), x.new_zeros((gu.shape[0], x.shape[1])).cpu(), gu if gate_up is None else gate_up(gu), dn, k, True)
    ref, bound = moe.moe_reference(*args, logits=logits.cpu()), moe.moe_error_bound(*args, logits=logits.cpu())
    return float(((y.cpu().double() - ref).abs() / bound).max()), float(ref.abs().max())


@pytest.mark.parametrize("variant", ["random", "same", 16, 17])
@pytest.mark.parametrize("H, I", [(64, 32), (192, 96), (256, 256), (320, 160)])
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mlp_is_inside_the_error_bound_of_the_definition(dtype, E, k, H, I, variant):
    """|y - moe_reference(dequantized)| <= moe_error_bound(dequantized) elementwise, by the device's logits, no row left out.  (64, 32): half a unit, one
    group; (192, 96): a tail inside a step; (256, 256): one step through the shared shift load; (320, 160): a step and a tail through the own-byte path.
    T = 17: a gate/up swap > 50 bounds away, rolled shifts > 25 -- half of what the references lie apart on the CPU (>= 79 / >= 34 over these cases)."""
    for T in (1, 17, 128):
        x, router, gate_up, down = inputs(T, E, H, I, dtype, 7 * T + E)
        q = moe.quantize_experts_fp4(gate_up, down)
        logits = crafted_logits(torch.nn.functional.linear(x, router), variant, k)
        y = run(x, logits, q, k, True)
        ratio, top = ratio_to_bound(y, x, logits, q, k)
        print(f"T {T}: max err / bound {ratio:.3f}")
        assert top > 0.01 and ratio <= 1, T
        if T == 17:
            assert ratio_to_bound(y, x, logits, q, k, gate_up=lambda w: torch.cat([w[:, I:], w[:, :I]], 1))[0] > 50
            assert ratio_to_bound(y, x, logits, (q[0], q[1].roll(1, 2), *q[2:]), k)[0] > 25
            assert I == 32 or ratio_to_bound(y, x, logits, (*q[:4], q[4].roll(1, 2), q[5]), k)[0] > 25  # (one group: nothing to roll)


@pytest.mark.parametrize("K", [256, 320])
@pytest.mark.parametrize("walk", ["gate", "up", "down"])
def test_every_code_under_every_shift_at_every_position_of_a_step(walk, K):
    """f16.  Rows of x hold one non-zero element (at kt), an up matrix one non-zero row per column, and in the gate / up walks expert e's down matrix
    feeds output channels 32 (e % 8) .. + 31 only: every output element is ONE product chain g -> silu(g) u -> act wd.  gate / up walk (E 256, k 8, H = K,
    I 32, 8192 rows): the walked matrix holds code (e + kt) % 16 under shift (e // 16 + kt // 32) % 13 (x carries 2^shift), the other one 1.0 under the
    same shift; row t takes kt = K - 256 + t % 256 and experts 8 (t // 256) .. + 7.  down walk (E 4, k 1, H 256, I = K): act's one element is at
    n = K - 256 + (kt + 64 e) % 256, down holds code (h + n) % 16 under shift (h // 16 + n // 32 + e) % 13.  Each walk: 16 codes x 13 shifts at each of
    the 256 k of a step; K = 256: the shared shift load, K = 320: own bytes.  A wrong nibble, byte or shift moves u or wd by a factor >= 1.5 or the sign,
    >= 1/3 of the element, and g likewise: through silu >= 5.5 % here (silu(-0.9375) = -0.2638, silu(-1.875) = -0.2493).  The bound is near 0.2 %."""
    f16, ar = torch.float16, torch.arange
    down_walk = walk == "down"
    (E, k, H, I, T) = (4, 1, 256, K, 1024) if down_walk else (256, 8, K, 32, 8192)
    e, t = ar(E), ar(T)
    kt, kk = H - 256 + t % 256, ar(H)
    gu, gsh = torch.zeros(E, 2 * I, H, dtype=torch.uint8), torch.zeros(E, 2 * I, H // 32, dtype=torch.uint8)
    dn, dsh = torch.zeros(E, H, I, dtype=torch.uint8), torch.zeros(E, H, I // 32, dtype=torch.uint8)
    x, one = torch.zeros(T, H, dtype=f16), 2  # (code 2 is 1.0)
    if down_walk:
        n = I - 256 + (kk[None] + 64 * e[:, None]) % 256  # [E, H]: the up row that column kt feeds
        gu[:, :I] = one
        gu[e[:, None], I + n, kk[None]] = one
        h, nn = ar(H)[None, :, None], ar(I)[None, None]
        dn[:] = (h + nn) % 16
        dsh[:] = (h // 16 + ar(I // 32)[None, None] + e[:, None, None]) % 13
        x[t, kt] = 1.25
        gus = torch.ldexp(torch.ones(E, 2 * I), torch.cat([-(ar(I) % 2), 4 - ar(I) % 2])[None].expand(E, -1))  # u of order 16: yslot stays far above f16's half steps
        chosen = (t // 256)[:, None]
    else:
        walked = ((e[:, None] + kk[None]) % 16).to(torch.uint8)  # [E, H]
        gsh[:] = ((e[:, None] // 16 + ar(H // 32)[None]) % 13)[:, None]
        gu[:, :I] = walked[:, None] if walk == "gate" else one
        gu[e, I + e % 32] = walked if walk == "up" else one
        dn[e[:, None], ar(H)[None], (e % 32)[:, None]] = (one * (ar(H)[None] // 32 == (e % 8)[:, None])).to(torch.uint8)
        x[t, kt] = 1.25 * torch.ldexp(torch.ones(T), ((t // 256) // 2 + kt // 32) % 13).to(f16)
        gus = torch.ldexp(torch.ones(E, 2 * I), -((e[:, None] + ar(2 * I)[None]) % 2))
        chosen = 8 * (t // 256)[:, None] + ar(k)[None]
    dns = torch.ldexp(torch.ones(E, H), -((e[:, None] + ar(H)[None]) % 2))
    logits = torch.full((T, E), -10.0, dtype=f16).scatter_(1, chosen, 10.0)
    pack = lambda c: c[..., 0::2] | (c[..., 1::2] << 4)  # noqa: E731
    q = [a.to(DEV) for a in (pack(gu), gsh, gus, pack(dn), dsh, dns)]
    y = torch.cat([run(x[r:r + 128].to(DEV), logits[r:r + 128].to(DEV), q, k, True) for r in range(0, T, 128)])
    ratio, top = ratio_to_bound(y, x, logits, q, k)
    print(f"max err / bound {ratio:.3f}, max |ref| {top:.2f}")
    assert top > 0.5 and ratio <= 1


@pytest.mark.parametrize("H, I", [(1280, 1056), (1344, 1280)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_buffers_stay_intact_calls_repeat_rows_are_independent_and_waves_take_several_units(dtype, H, I):
    """Each product with K % 256 == 0 (1280) and without (1344, 1056): 9 to 11 units, two or three per wave (the bound test: one at most): prefetch hand-over."""
    T, E, k = 33, 4, 2
    x, router, gate_up, down = inputs(T, E, H, I, dtype, 5)
    q = moe.quantize_experts_fp4(gate_up, down)
    need = int(_lib.load().hyd_moe_workspace_bytes(T, E, k, H, I, _lib.HYD_F16 if dtype == torch.float16 else _lib.HYD_BF16))

    def call(x):
        yb = torch.full((T + 2, H + 24), SENT16, dtype=dtype, device=DEV)
        wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        moe.moe_rows_w4(x, torch.nn.functional.linear(x, router), *q, k, True, yb[1:T + 1, 8:8 + H], workspace=wsb[GUARD:GUARD + need])
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
    q = moe.quantize_experts_fp4(gate_up, down)
    y, ids, w = moe.moe_mlp(x.view(3, 100, H), router, q[0], q[3], k, True, return_routing=True, gate_up_shift=q[1], gate_up_scale=q[2], down_shift=q[4], down_scale=q[5])
    logits = torch.nn.functional.linear(x, router)
    for rows in (slice(0, 128), slice(128, 256), slice(256, 300)):
        ic, wc = (torch.empty((rows.stop - rows.start, k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32))
        yc = run(x[rows], logits[rows], q, k, True, ids_out=ic, weights_out=wc)
        assert torch.equal(y.view(T, H)[rows], yc) and torch.equal(ids[rows], ic) and torch.equal(w[rows], wc)
    assert y.shape == (3, 100, H) and torch.equal(ids.cpu().long(), moe.route_reference(logits.cpu(), k, True)[0])


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_models_with_fp4_experts_run_through_the_shell(kind):
    """generate() with the graph off and on: the same tokens; logits within test_moe_gpu.py's 0.15 of transformers' bf16 forward on the dequantized experts."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    hf = tiny_hf(kind)
    model = HydragenLlamaForCausalLM.from_hf_model(copy.deepcopy(hf).to(DEV))
    model.quantize_experts(dtype=FP4_DTYPE)
    e, he = model.model.layers[0].mlp.experts, hf.model.layers[0].mlp.experts
    he.gate_up_proj.data, he.down_proj.data = moe.dequantize_experts_fp4(*(b.cpu() for b in e.buffers()), dtype=torch.bfloat16)
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
