"""-m gpu: fp8 linear-layer weights on the device -- hyd_linear_w8 and hyd_weight_widen against the definition
(hydragen_amd/weight_quant.py), then the quantized model shell: decode logits, the widen route of long prefills, and generate()
with the decode graph on and off.

Every kernel call of this file goes through `call`: x and y are row-strided views, y and the split-K workspace are carved out of
larger buffers filled with a sentinel, and the bytes around them must still hold it afterwards."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
DTYPES = [torch.float16, torch.bfloat16]
SENT16 = -21504.0  # exactly representable in f16 and bf16; no test produces it
GUARD = 256        # sentinel bytes on either side of the workspace


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def call(x, w8, scale):
    """hyd_linear_w8 on a strided x into a strided y with sentinels all round; returns y [M, N] (a copy)."""
    from hydragen_amd import _lib
    from hydragen_amd.flash import _stream

    lib = _lib.load()
    M, K = x.shape
    N = w8.shape[0]
    xs, ys = K + 24, (N + 7) // 8 * 8 + 16
    xb = torch.full((M + 1, xs), float("nan"), dtype=x.dtype, device=DEV)  # what lies between the rows is NaN: it must not be read into a sum
    xb[:M, :K] = x
    yb = torch.full((M + 3, ys), SENT16, dtype=x.dtype, device=DEV)
    need = int(lib.hyd_linear_w8_workspace_bytes(M, N, K))
    wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    p = _lib.LinearW8Params()
    p.x, p.w8, p.scale, p.y = xb.data_ptr(), w8.data_ptr(), scale.data_ptr(), yb.data_ptr()
    p.workspace, p.workspace_bytes = (wsb.data_ptr() + GUARD, need) if need else (0, 0)
    p.x_row_stride, p.y_row_stride, p.M, p.N, p.K = xs, ys, M, N, K
    p.dtype = _lib.HYD_F16 if x.dtype == torch.float16 else _lib.HYD_BF16
    _lib.check(lib.hyd_linear_w8(C.byref(p), _stream()))
    torch.cuda.synchronize()
    assert bool((yb[M:] == SENT16).all()) and bool((yb[:, N:] == SENT16).all()), "rows past M / columns past N were written"
    assert bool((wsb[:GUARD] == 0xA5).all()) and bool((wsb[GUARD + need:] == 0xA5).all()), "bytes around the workspace were written"
    return yb[:M, :N].clone()


def want16(x, w8, scale):
    from hydragen_amd.weight_quant import linear_reference

    return linear_reference(x, w8, scale).to(x.dtype)


# ---- exact cases ---------------------------------------------------------------------------------------------------------------
MS, NS = (1, 2, 15, 16, 17, 33, 100), (1, 16, 40, 272)


@pytest.mark.parametrize("K", [16, 32, 48, 80, 4096, 11008])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_integer_products_are_exact_in_any_accumulation_order(dtype, K):
    """x in [-2, 2], codes in [-4, 4], scales 2^-3 .. 2^2: every partial sum is an integer below 2^24, so fp32 accumulation is
    exact whatever the order and the result is the definition rounded once.  The grid covers the M tail, the N tail, the k-step
    tail (K % 128 != 0), one row, one channel, and at N = 272 and K = 4096 / 11008 the split plans of the model's depths."""
    g = gen(K)
    Mx, Nx = max(MS), max(NS)
    x_all = torch.randint(-2, 3, (Mx, K), device=DEV, generator=g).to(dtype)
    w_all = torch.randint(-4, 5, (Nx, K), device=DEV, generator=g).float().to(FP8)
    s_all = torch.exp2(torch.randint(-3, 3, (Nx,), device=DEV, generator=g).float())
    ref_all = want16(x_all, w_all, s_all)  # one reference: rows and channels are independent
    for M in MS:
        for N in NS:
            got = call(x_all[:M], w_all[:N].contiguous(), s_all[:N].contiguous())
            assert torch.equal(got, ref_all[:M, :N]), (M, N, K)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_finite_code_is_widened_exactly(dtype):
    """One-hot rows of x (1.0 and -0.5) pick single codes: y is the code times the scale (times the pick), exactly."""
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8, device=DEV)
    assert codes.numel() == 254
    N, K = 40, 256
    row = torch.cat([codes, torch.zeros(2, dtype=torch.uint8, device=DEV)])
    w8 = torch.stack([row.roll(7 * n) for n in range(N)]).view(FP8)  # every channel holds every code, at shifted k
    scale = torch.exp2((torch.arange(N, device=DEV) % 6 - 3).float())
    pick = torch.where(torch.arange(K, device=DEV) % 2 == 0, 1.0, -0.5)
    x = torch.diag(pick).to(dtype)  # M = K = 256 rows
    got = call(x, w8, scale)
    want = (w8.float() * scale[:, None]).T * pick[:, None]  # [K, N], exact in fp32
    assert torch.equal(want.to(dtype).float(), want), "the expected values are 16-bit values"
    assert torch.equal(got.float(), want)
    assert bool((got[:, 0].float().abs() == 448 * scale[0] * pick.abs()).any()) and bool((got.float().abs() == 2.0 ** -9 * scale[None] * 0.5).any())


# ---- general values ------------------------------------------------------------------------------------------------------------
def random_codes(N, K, g):
    c = torch.randint(0, 256, (N, K), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    return torch.where(c & 0x7F == 0x7F, torch.zeros_like(c), c).view(FP8)


def x_unit(M, K, dtype, g):
    return torch.randn((M, K), device=DEV, generator=g).to(dtype)


def x_wide(M, K, dtype, g):
    return (torch.randn((M, K), device=DEV, generator=g) * 30).to(dtype)


def x_outlier(M, K, dtype, g):
    x = torch.randn((M, K), device=DEV, generator=g)
    x[torch.arange(M, device=DEV), torch.randint(0, K, (M,), device=DEV, generator=g)] = 1e4
    return x.to(dtype)


@pytest.mark.parametrize("make_x", [x_unit, x_wide, x_outlier])
@pytest.mark.parametrize("M, N, K", [(33, 272, 4096), (100, 40, 11008), (17, 272, 80)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_general_values_stay_within_the_derived_bound(dtype, M, N, K, make_x):
    """|y - y64| <= 2^-8 |y64| + K 2^-23 sum_k |x w| (bf16; 2^-11 for fp16): twice the half-ulp of the one rounding plus twice the
    bound of an fp32 running sum of K terms.  Random codes over the whole format with scales that keep the products in fp16's
    range (2^-12 .. 2^-9: |w| <= 0.875, so that a 1e4 outlier stays below 65504 with the rest of the row)."""
    from hydragen_amd.weight_quant import linear_reference

    g = gen(M * 7 + N)
    x = make_x(M, K, dtype, g)
    w8 = random_codes(N, K, g)
    scale = torch.exp2(torch.randint(-12, -8, (N,), device=DEV, generator=g).float())
    got = call(x, w8, scale).double()
    y64 = linear_reference(x, w8, scale)
    mag = x.double().abs() @ (w8.double().abs() * scale.double()[:, None]).T
    bound = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11) * y64.abs() + K * 2.0 ** -23 * mag
    assert torch.isfinite(got).all()
    excess = (got - y64).abs() - bound
    assert bool((excess <= 0).all()), f"worst excess {float(excess.max()):.3e} at |y64| {float(y64.abs().flatten()[excess.argmax()]):.3e}"


# ---- row independence, determinism ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, N, K", [(33, 40, 4096), (70, 272, 48)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_poisoned_row_of_x_leaves_every_other_row_bit_identical(dtype, M, N, K):
    g = gen(3)
    x = x_unit(M, K, dtype, g)
    w8, scale = random_codes(N, K, g), torch.exp2(torch.randint(-12, -8, (N,), device=DEV, generator=g).float())
    clean = call(x, w8, scale)
    bad = x.clone()
    bad[7, 0], bad[7, K // 2], bad[7, K - 1] = float("nan"), float("inf"), float("-inf")
    got = call(bad, w8, scale)
    keep = torch.arange(M, device=DEV) != 7
    assert torch.equal(got[keep].view(torch.int16), clean[keep].view(torch.int16))
    assert bool(torch.isnan(got[7]).all())


@pytest.mark.parametrize("M, N, K, split", [(8, 272, 4096, True), (40, 272, 11008, True), (8, 272, 48, False), (100, 40, 80, False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_are_bit_identical(dtype, M, N, K, split):
    from hydragen_amd.weight_quant import workspace_bytes

    assert (workspace_bytes(M, N, K) > 0) == split
    g = gen(4)
    x, w8 = x_wide(M, K, dtype, g), random_codes(N, K, g)
    scale = torch.exp2(torch.randint(-12, -8, (N,), device=DEV, generator=g).float())
    a, b = call(x, w8, scale), call(x, w8, scale)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_python_wrapper_and_module_route_by_rows():
    """weight_quant.linear_w8 (contiguous tensors, its own workspace) agrees with the carved call; Fp8Linear takes the kernel up to
    W8_MAX_ROWS rows and widen + F.linear above, where it equals F.linear on dequantize_weight exactly."""
    from hydragen_amd import weight_quant as wq
    from tests.gpu_util import Recorder
    from hydragen_amd import _lib

    g = gen(5)
    lin = torch.nn.Linear(128, 352, bias=False, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.normal_(0, 0.05, generator=g)
    mod = wq.Fp8Linear.from_linears((lin,))
    x = x_unit(6, 128, torch.bfloat16, g)
    assert torch.equal(wq.linear_w8(x, mod.weight, mod.weight_scale), call(x, mod.weight, mod.weight_scale))
    rec, real = Recorder(_lib.load()), _lib._lib
    _lib._lib = rec
    try:
        small = mod(x.view(2, 3, 128))
        big = mod(x_unit(wq.W8_MAX_ROWS + 64, 128, torch.bfloat16, g).view(2, -1, 128))
    finally:
        _lib._lib = real
    assert [c for c in rec.calls if c in ("hyd_linear_w8", "hyd_weight_widen")] == ["hyd_linear_w8", "hyd_weight_widen"]
    assert small.shape == (2, 3, 352) and torch.equal(small.view(6, 352), call(x, mod.weight, mod.weight_scale))
    xb = x_unit(wq.W8_MAX_ROWS + 64, 128, torch.bfloat16, gen(6)).view(2, -1, 128)
    assert torch.equal(mod(xb), torch.nn.functional.linear(xb, wq.dequantize_weight(mod.weight, mod.weight_scale, torch.bfloat16)))
    assert big.shape == (2, wq.W8_MAX_ROWS // 2 + 32, 352)


# ---- hyd_weight_widen ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 4096])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_widen_is_dequantize_weight_bit_for_bit(dtype, K):
    from hydragen_amd.weight_quant import dequantize_weight, weight_widen

    N = 40
    g = gen(K)
    w8 = random_codes(N, K, g)
    scale = torch.exp2((torch.arange(N, device=DEV) % 11 - 8).float())  # 2^-8 .. 2^2
    buf = torch.full((N + 2, K + 16), SENT16, dtype=dtype, device=DEV)
    weight_widen(w8, scale, buf[:N, :K])
    torch.cuda.synchronize()
    assert torch.equal(buf[:N, :K].view(torch.int16), dequantize_weight(w8, scale, dtype).view(torch.int16))
    assert bool((buf[N:] == SENT16).all()) and bool((buf[:, K:] == SENT16).all())


# ---- the model shell -----------------------------------------------------------------------------------------------------------
NEW, PROMPT = 8, 16


def tiny(dtype=torch.bfloat16, seed=0):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=128, intermediate_size=352, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                      vocab_size=512, max_position_embeddings=512, rms_norm_eps=1e-5)
    return HydragenLlamaForCausalLM.from_config(cfg, dtype=dtype, device=DEV, seed=seed, std=0.05)


_MODELS = {}


def models():
    """(quantized model, its twin on dequantized 16-bit nn.Linear weights, prompts), built once."""
    if not _MODELS:
        from tests.test_weight_fp8 import dequantized_twin

        q = tiny()
        ref = copy.deepcopy(q)
        q.quantize_weights()
        twin = dequantized_twin(q, ref)
        for m in (q, twin):
            m.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[512])
        _MODELS["m"] = (q, twin, torch.randint(1, 512, (2, PROMPT), device=DEV, generator=gen(11)))
    return _MODELS["m"]


def _stack(logits):
    return (logits if isinstance(logits, torch.Tensor) else torch.stack(list(logits), 1)).float()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_decode_logits_are_within_twice_the_16_bit_models_own_rounding_noise():
    """Kernel route (6 rows per step): the quantized model against the same model on dequantized 16-bit nn.Linear weights, fed the
    same tokens.  The yardstick is that 16-bit model's own distance from the fp32 transformer on its weights, measured here; the
    factor 2 covers two independent accumulation orders."""
    from tests.test_model_gpu import ref_logits

    q, twin, prompts = models()
    G, l16 = twin.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, return_logits=True)
    _, lq = q.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, return_logits=True, token_overrides=G)
    l16, lq = _stack(l16), _stack(lq)
    full = torch.cat([prompts.repeat_interleave(3, 0), G], 1)
    l32 = ref_logits(twin, full)[:, PROMPT - 1 : PROMPT - 1 + NEW]
    assert lq.shape == l16.shape == l32.shape
    noise, dist = rel_l2(l16, l32), rel_l2(lq, l16)
    print(f"relative L2: fp8-weight model vs 16-bit twin {dist:.3e}; 16-bit twin vs fp32 transformer {noise:.3e}")
    assert torch.isfinite(lq).all() and dist <= 2 * noise


def test_a_prefill_with_more_rows_than_the_kernel_takes_equals_the_16_bit_gemm_exactly():
    from hydragen_amd.weight_quant import W8_MAX_ROWS

    q, twin, _ = models()
    n = W8_MAX_ROWS // 2 + 32  # 2 prompts: more than W8_MAX_ROWS rows per projection
    assert n <= 512, "the shared level of models() holds 512 tokens"
    long = torch.randint(1, 512, (2, n), device=DEV, generator=gen(12))
    # (three completions per prompt: the prompts are a SHARED level -- with one they would be unique prompts, and the unique cache
    # of models() holds NEW + 8 tokens)
    outs = [m.generate([long], num_return_sequences=3, max_new_tokens=1, temperature=0, return_logits=True) for m in (q, twin)]
    assert torch.equal(_stack(outs[0][1])[:, 0], _stack(outs[1][1])[:, 0])


@pytest.mark.parametrize("kw", [dict(), dict(draft_tokens=3, draft="prompt_lookup"), dict(kv_cache_dtype=FP8)], ids=["plain", "drafts", "fp8-kv"])
def test_generate_with_the_decode_graph_returns_the_tokens_of_eager_decoding(kw):
    q, _, prompts = models()
    kw = dict(kw)
    kv = kw.pop("kv_cache_dtype", None)
    if kv is not None:
        q.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[512], kv_cache_dtype=kv)
    try:
        run = lambda: q.generate([prompts], num_return_sequences=3, max_new_tokens=NEW, temperature=0, **kw)  # noqa: E731
        eager = run()
        q.graph(True)
        graphed = run()
        again = run()  # a replay of the captured graph
    finally:
        q.graph(False)
        if kv is not None:
            q.setup_caches(max_unique_batch_size=6, max_unique_seq_length=NEW + 8, max_shared_batch_sizes=[2], max_shared_seq_lengths=[512])
    assert eager.shape == (6, NEW) and torch.equal(eager, graphed) and torch.equal(eager, again)
