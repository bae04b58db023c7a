"""-m gpu: the mixture-of-experts kernels (csrc/moe.hip through hydragen_amd/moe.py) against the float64 definition and its error
bound, routing alone, buffers and repeatability, chunked long calls, and Mixtral / Qwen3-MoE models through the shell."""
import copy
import ctypes as C

import pytest
import torch

from hydragen_amd import moe
from tests.test_moe_abi import tiny_hf
from tests.test_weight_fp8_gpu import DEV, DTYPES, GUARD, SENT16

pytestmark = pytest.mark.gpu
IDS = ["f16", "bf16"]


def inputs(T, E, H, I, dtype, seed):
    """x, router, gate_up, down.  Router rows of std 0.5 give logits of std 4 and more, so a row's k weights are far from equal; gate
    and up rows of std 0.3 give pre-activations of order 2 and more: silu(g) u - silu(u) g vanishes to second order for small g and u,
    and a swapped layout could then hide inside a bfloat16 bound."""
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(s, generator=g) * sd).to(dtype).to(DEV) for s, sd in (((T, H), 1.0), ((E, H), 0.5), ((E, 2 * I, H), 0.3), ((E, H, I), 0.1)))


def run(x, logits, gate_up, down, k, renorm, routing=False):
    T = x.shape[0]
    ids, w = (torch.empty((T, k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32)) if routing else (None, None)
    y = moe.moe_rows(x, logits, gate_up, down, k, renorm, torch.empty_like(x), ids, w)
    return (y, ids, w) if routing else y


@pytest.mark.parametrize("renorm", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("E, k", [(4, 1), (4, 4), (8, 2), (128, 8), (200, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_routing_alone_is_the_definition(dtype, E, k, renorm):
    """ids exactly route_reference's -- on an all-equal row, a row of few distinct values, a row of zeros of either sign, and random
    rows --, weights within 4 2^-23 relative (renormalised: (k + 5) 2^-23, what the bound grants the weight and the combine)."""
    for T in (1, 33, 128):
        g = torch.Generator().manual_seed(100 * E + T)
        logits = (torch.randn(T, E, generator=g) * 2).to(dtype)
        logits[0] = 1.5
        if T > 3:
            logits[1] = torch.randint(-1, 2, (E,), generator=g).to(dtype)
            logits[2] = torch.where(torch.arange(E) % 2 == 0, 0.0, -0.0).to(dtype)
            logits[3, E // 2:] = logits[3, : E - E // 2].flip(0)
        x, _, gate_up, down = inputs(T, E, 64, 32, dtype, 1)
        _, ids, w = run(x, logits.to(DEV), gate_up, down, k, renorm, routing=True)
        want_ids, want_w = moe.route_reference(logits, k, renorm)
        assert torch.equal(ids.cpu().long(), want_ids), T
        rel = float(((w.cpu().double() - want_w).abs() / want_w).max())
        print(f"T {T}: max relative weight error {rel * 2 ** 23:.2f} x 2^-23")
        assert rel <= ((k + 5) if renorm else 4) * 2.0 ** -23, T


def crafted_logits(logits, variant, k):
    """`same`: every row chooses experts 0 .. k - 1 (T slots each: several passes; all other experts empty); 16 / 17: exactly that
    many rows choose expert 1."""
    logits = logits.clone()
    if variant == "same":
        for j in range(k):
            logits[:, j] = 50 - j
    elif variant in (16, 17):
        logits[:, 1] = -50
        logits[:variant, 1] = 50
    return logits


@pytest.mark.parametrize("variant", ["random", "same", 16, 17])
@pytest.mark.parametrize("H, I", [(64, 32), (64, 96), (192, 32), (192, 96)])
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mlp_is_inside_the_error_bound_of_the_definition(dtype, E, k, H, I, variant):
    """|y - moe_reference| <= moe_error_bound elementwise, both routed by the logits the device used: no row is left out.  H = 64
    is one step (three waves without one), 192 an uneven split; I = 32 half a step of the down product, 96 one and a half.  Up rows
    in front of gate rows must miss by more than 100 bounds."""
    for T in (1, 17, 128):
        x, router, gate_up, down = inputs(T, E, H, I, dtype, 7 * T + E)
        logits = crafted_logits(torch.nn.functional.linear(x, router), variant, k)
        y = run(x, logits, gate_up, down, k, True).cpu().double()
        args = [t.cpu() for t in (x, router, gate_up, down)]
        ref = moe.moe_reference(*args, k, True, logits=logits.cpu())
        bound = moe.moe_error_bound(*args, k, True, logits=logits.cpu())
        ratio = float(((y - ref).abs() / bound).max())
        print(f"T {T}: max err / bound {ratio:.3f}")
        assert float(ref.abs().max()) > 0.01 and ratio <= 1, T
    args[2] = torch.cat([args[2][:, I:], args[2][:, :I]], 1)
    assert float(((y - moe.moe_reference(*args, k, True, logits=logits.cpu())).abs() / bound).max()) > 100


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_buffers_stay_intact_calls_repeat_and_rows_are_independent(dtype):
    from hydragen_amd import _lib
    from hydragen_amd.flash import _stream

    T, E, k, H, I = 33, 8, 2, 192, 96
    x, router, gate_up, down = inputs(T, E, H, I, dtype, 5)
    logits = torch.nn.functional.linear(x, router)
    lib = _lib.load()
    need = int(lib.hyd_moe_workspace_bytes(T, E, k, H, I, _lib.HYD_F16 if dtype == torch.float16 else _lib.HYD_BF16))

    def call(x, logits):
        yb = torch.full((T + 2, H + 24), SENT16, dtype=dtype, device=DEV)
        wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        moe.moe_rows(x, logits, gate_up, down, k, False, yb[1:T + 1, 8:8 + H], workspace=wsb[GUARD:GUARD + need])
        torch.cuda.synchronize()
        assert bool((yb[0] == SENT16).all()) and bool((yb[T + 1] == SENT16).all()) and bool((yb[:, :8] == SENT16).all()) and bool((yb[:, 8 + H:] == SENT16).all())
        assert bool((wsb[:GUARD] == 0xA5).all()) and bool((wsb[GUARD + need:] == 0xA5).all()), "bytes around the workspace were written"
        return yb[1:T + 1, 8:8 + H].clone()

    y = call(x, logits)
    assert torch.equal(y, call(x, logits)) and bool(torch.isfinite(y).all())
    xn = x.clone()
    xn[5] = float("nan")
    yn = call(xn, torch.nn.functional.linear(xn, router))
    keep = torch.arange(T, device=DEV) != 5
    assert torch.equal(yn[keep], y[keep]) and bool(torch.isnan(yn[5]).all())
    p = moe.MoeParams()  # a refusal on the device: nothing is launched, the message names the field
    assert lib.hyd_moe_mlp(C.byref(p), _stream()) == -1 and "T 0" in lib.hyd_last_error_string().decode()


def test_long_calls_are_the_chunk_calls():
    T, E, k, H, I = 300, 8, 2, 64, 32
    x, router, gate_up, down = inputs(T, E, H, I, torch.bfloat16, 9)
    y, ids, w = moe.moe_mlp(x.view(3, 100, H), router, gate_up, down, k, True, return_routing=True)
    logits = torch.nn.functional.linear(x, router)
    for r in range(0, T, moe.MOE_MAX_ROWS):
        rows = slice(r, min(T, r + moe.MOE_MAX_ROWS))
        yc, ic, wc = run(x[rows], logits[rows], gate_up, down, k, True, routing=True)
        assert torch.equal(y.view(T, H)[rows], yc) and torch.equal(ids[rows], ic) and torch.equal(w[rows], wc)
    assert y.shape == (3, 100, H) and torch.equal(ids.cpu().long(), moe.route_reference(logits.cpu(), k, True)[0])


@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_models_with_experts_run_through_the_shell(kind):
    """from_hf_model on a one-layer model, prefill and greedy decode steps with the graph off and on: the same tokens, and logits
    that agree with transformers' own bf16 forward (on the CPU) of the prompt and the chosen tokens by the mean relative difference
    of tests/test_moe.py, within the 0.15 the Qwen3 golden test grants a whole model."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    hf = tiny_hf(kind)
    model = HydragenLlamaForCausalLM.from_hf_model(copy.deepcopy(hf).to(DEV))
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
        print(f"{kind}: mean relative difference to transformers {rdiff(got[0], want):.4f}")
        assert rdiff(got[0], want) < 0.15
