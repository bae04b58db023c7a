"""-m gpu: 4-bit (e2m1) linear-layer weights on the device -- hyd_linear_w4 and hyd_weight_widen_w4 against the definition
(hydragen_amd/weight_quant.py), then the quantized model shell: decode logits, the widen route, generate() with the graph on and off.

Every kernel call goes through `call`: x and y are row-strided views, y and the split-K workspace are carved out of larger buffers
filled with a sentinel, and the bytes around them must still hold it afterwards."""
import copy
import ctypes as C

import pytest
import torch

from tests.test_weight_fp8_gpu import DEV, DTYPES, GUARD, NEW, PROMPT, SENT16, gen, tiny, x_outlier, x_unit, x_wide

pytestmark = pytest.mark.gpu
FP4 = torch.float4_e2m1fn_x2
FP8 = torch.float8_e4m3fn


def call(x, w4, shift, scale):
    """hyd_linear_w4 on a strided x into a strided y with sentinels all round; returns y [M, N] (a copy)."""
    from hydragen_amd import _lib, weight_quant as wq
    from hydragen_amd.flash import _stream

    lib = _lib.load()
    (M, K), N = x.shape, w4.shape[0]
    xs, ys = K + 24, (N + 7) // 8 * 8 + 16
    xb = torch.full((M + 1, xs), float("nan"), dtype=x.dtype, device=DEV)  # what lies between the rows must not be read into a sum
    xb[:M, :K] = x
    yb = torch.full((M + 3, ys), SENT16, dtype=x.dtype, device=DEV)
    need = int(lib.hyd_linear_w4_workspace_bytes(M, N, K))
    wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    p = wq.LinearW4Params()
    p.x, p.w4, p.shift, p.scale, p.y = xb.data_ptr(), w4.data_ptr(), shift.data_ptr(), scale.data_ptr(), yb.data_ptr()
    p.workspace, p.workspace_bytes = (wsb.data_ptr() + GUARD, need) if need else (0, 0)
    p.x_row_stride, p.y_row_stride, p.M, p.N, p.K = xs, ys, M, N, K
    p.dtype = _lib.HYD_F16 if x.dtype == torch.float16 else _lib.HYD_BF16
    _lib.check(lib.hyd_linear_w4(C.byref(p), _stream()))
    torch.cuda.synchronize()
    assert bool((yb[M:] == SENT16).all()) and bool((yb[:, N:] == SENT16).all()), "rows past M / columns past N were written"
    assert bool((wsb[:GUARD] == 0xA5).all()) and bool((wsb[GUARD + need:] == 0xA5).all()), "bytes around the workspace were written"
    return yb[:M, :N].clone()


def random_w(N, K, g, max_shift=12, scale_exp=(-3, 3)):
    w4 = torch.randint(0, 256, (N, K // 2), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    shift = torch.randint(0, max_shift + 1, (N, K // 32), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    return w4, shift, torch.exp2(torch.randint(*scale_exp, (N,), device=DEV, generator=g).float())


MS, NS = (1, 16, 17, 32, 33, 64, 65, 128), (40, 272)


@pytest.mark.parametrize("K", [32, 64, 96, 160, 4096, 11008])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_products_are_exact_in_any_accumulation_order(dtype, K):
    """Integer x in [-4, 4], any code, shifts in {0, 1, 2}, scales 2^-3 .. 2^2: every partial sum is a multiple of 2^-3 below
    2^21, so fp32 accumulation is exact whatever the order and the result is the definition rounded once.  The grid covers both
    forms and every row tiling, the channel tail and a quad tail, a group tail (K = 32 .. 160: less than one step, K % 256 != 0
    with the byte-wise shift loads), a step tail (11008 = 43 steps) and both split depths of either form (N = 272 / 40)."""
    from hydragen_amd.weight_quant import linear_reference_fp4

    g = gen(K)
    x_all = torch.randint(-4, 5, (max(MS), K), device=DEV, generator=g).to(dtype)
    w4, shift, scale = random_w(max(NS), K, g, max_shift=2)
    ref_all = linear_reference_fp4(x_all, w4, shift, scale).to(dtype)  # one reference: rows and channels are independent
    for M in MS:
        for N in NS:
            got = call(x_all[:M], w4[:N].contiguous(), shift[:N].contiguous(), scale[:N].contiguous())
            assert torch.equal(got, ref_all[:M, :N]), (M, N, K)


@pytest.mark.parametrize("K", [256, 288])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_code_with_every_shift_is_widened_exactly_at_every_position(dtype, K):
    """Channel n holds code (k + n) % 16 at k and shift (n // 16 + k // 32) % 13 on group k // 32: over the 208 channels every code
    meets every shift at every nibble of every 16-byte load of a step (K = 288: and of a tail step with byte-wise shift loads).
    One-hot rows of x (1.0 and -0.5) pick single k: y is the dequantized value times the pick, exactly -- through the rows form
    (all K rows at once), through the small form (32 rows at a time), and through hyd_weight_widen_w4 into a strided buffer."""
    from hydragen_amd.weight_quant import dequantize_weight_fp4, weight_widen_fp4

    N = 16 * 13
    n, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None]
    idx = ((k + n) % 16).to(torch.uint8)
    w4 = (idx[:, 0::2] | (idx[:, 1::2] << 4)).contiguous()
    shift = ((n // 16 + k[:, ::32] // 32) % 13).to(torch.uint8).contiguous()
    scale = torch.exp2((torch.arange(N, device=DEV) % 4).float())
    pick = torch.where(torch.arange(K, device=DEV) % 2 == 0, 1.0, -0.5)
    want = dequantize_weight_fp4(w4, shift, scale, torch.float32).T * pick[:, None]  # [K, N], exact in fp32
    assert torch.equal(want.to(dtype).float(), want) and float(want.abs()[want != 0].min()) == 2.0 ** -14, "16-bit values, down to 0.5 * 2^-12 * 0.5"
    x = torch.diag(pick).to(dtype)
    assert torch.equal(call(x, w4, shift, scale).float(), want)
    for m in range(0, K, 32):
        assert torch.equal(call(x[m : m + 32], w4, shift, scale).float(), want[m : m + 32]), m
    buf = torch.full((N, K + 8), SENT16, dtype=dtype, device=DEV)
    weight_widen_fp4(w4, shift, scale, buf[:, :K])
    assert torch.equal(buf[:, :K].view(torch.int16), dequantize_weight_fp4(w4, shift, scale, dtype).view(torch.int16))
    assert bool((buf[:, K:] == SENT16).all())


@pytest.mark.parametrize("make_x", [x_unit, x_wide, x_outlier])
@pytest.mark.parametrize("M, N, K", [(33, 272, 4096), (100, 40, 11008), (17, 272, 160)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_general_values_stay_within_the_derived_bound(dtype, M, N, K, make_x):
    """|y - y64| <= 2^-8 |y64| + K 2^-23 sum_k |x w| (bf16; 2^-11 for fp16): the bound of the fp8 kernel, the same arithmetic.
    Random codes and shifts over the whole format, scales 2^-4 .. 2^-1: |w| <= 3, so a 1e4 outlier stays inside fp16 with the rest
    of the row, and |w| >= 2^-17 on every non-zero code, so no output falls below fp16's normal range (where the format's step is
    absolute, 2^-24, and a relative bound says nothing) without the sum term covering that step."""
    from hydragen_amd.weight_quant import dequantize_weight_fp4, linear_reference_fp4

    g = gen(M * 7 + N)
    x = make_x(M, K, dtype, g)
    w4, shift, scale = random_w(N, K, g, scale_exp=(-4, 0))
    got = call(x, w4, shift, scale).double()
    y64 = linear_reference_fp4(x, w4, shift, scale)
    mag = x.double().abs() @ dequantize_weight_fp4(w4, shift, scale, torch.float64).abs().T
    bound = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11) * y64.abs() + K * 2.0 ** -23 * mag
    excess = (got - y64).abs() - bound
    assert torch.isfinite(got).all() and bool((excess <= 0).all()), f"worst excess {float(excess.max()):.3e}"


@pytest.mark.parametrize("M, N, K", [(33, 40, 4096), (70, 272, 96), (20, 40, 4096)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_poisoned_row_of_x_leaves_every_other_row_bit_identical(dtype, M, N, K):
    g = gen(M + K)
    x = x_unit(M, K, dtype, g)
    w = random_w(N, K, g)
    clean = call(x, *w)
    x[M // 2, ::2], x[M // 2, 1::2] = float("nan"), float("inf")
    got = call(x, *w)
    keep = torch.arange(M, device=DEV) != M // 2
    assert torch.equal(got[keep].view(torch.int16), clean[keep].view(torch.int16)) and not torch.isfinite(got[M // 2]).any()


@pytest.mark.parametrize("M, N, K, split", [(8, 272, 4096, True), (40, 272, 11008, True), (8, 272, 96, False), (100, 40, 160, False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_are_bit_identical(dtype, M, N, K, split):
    from hydragen_amd import _lib

    assert (_lib.load().hyd_linear_w4_workspace_bytes(M, N, K) > 0) == split
    g = gen(M + N)
    x, w = x_wide(M, K, dtype, g), random_w(N, K, g)
    assert torch.equal(call(x, *w).view(torch.int16), call(x, *w).view(torch.int16))


def test_the_module_routes_by_rows():
    from hydragen_amd.weight_quant import W4_MAX_ROWS, Fp4Linear, linear_w4

    g = gen(3)
    lin = torch.nn.Linear(160, 272, bias=True, device=DEV, dtype=torch.bfloat16)
    mod = Fp4Linear.from_linears((lin,))
    x = x_unit(W4_MAX_ROWS + 1, 160, torch.bfloat16, g)
    at = mod(x[:W4_MAX_ROWS].view(2, -1, 160))
    assert at.shape == (2, W4_MAX_ROWS // 2, 272)
    assert torch.equal(at.view(-1, 272), linear_w4(x[:W4_MAX_ROWS], mod.weight, mod.weight_shift, mod.weight_scale) + mod.bias), "the kernel runs at W4_MAX_ROWS"
    assert torch.equal(mod(x), torch.nn.functional.linear(x, mod.dequantized()) + mod.bias), "above it: widen + the 16-bit GEMM, exactly"


# ---- the model shell: test_weight_fp8_gpu's model tests (their criteria and margins) on a model quantized to e2m1 -------------------
_MODELS = {}


@pytest.fixture
def shell(monkeypatch):
    """Swaps the fp8 file's models() cache for (e2m1 model, its twin on dequantized 16-bit nn.Linear weights, prompts), built once."""
    import tests.test_weight_fp8_gpu as f8
    from hydragen_amd.weight_quant import Fp4Linear
    from tests.test_weight_fp8 import dequantized_twin

    if not _MODELS:
        q = tiny()
        ref = copy.deepcopy(q)
        q.quantize_weights(dtype=FP4)
        twin = dequantized_twin(q, ref)
        for m in (q, twin):
            m.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[512])
        _MODELS["m"] = (q, twin, torch.randint(1, 512, (2, PROMPT), device=DEV, generator=gen(11)))
    assert isinstance(_MODELS["m"][0].model.layers[0].mlp.down_proj, Fp4Linear)
    monkeypatch.setattr(f8, "_MODELS", _MODELS)
    return f8


def test_decode_logits_and_the_widen_route_of_a_long_prefill(shell):
    shell.test_decode_logits_are_within_twice_the_16_bit_models_own_rounding_noise()
    shell.test_a_prefill_with_more_rows_than_the_kernel_takes_equals_the_16_bit_gemm_exactly()


@pytest.mark.parametrize("kw", [dict(), dict(draft_tokens=3, draft="prompt_lookup"), dict(kv_cache_dtype=FP8)], ids=["plain", "drafts", "fp8-kv"])
def test_generate_with_the_decode_graph_returns_the_tokens_of_eager_decoding(shell, kw):
    shell.test_generate_with_the_decode_graph_returns_the_tokens_of_eager_decoding(kw)
