"""-m gpu: the grouped fp8 expert call (csrc/moe_grouped_w8.hip through moe.moe_rows_grouped_w8) against the float64 definition on the
dequantized weights and its bound, every e4m3 code at every byte of a step, buffers and repeatability, and the routes through moe_mlp
and MoeMLP."""
import pytest
import torch

from hydragen_amd import _lib, moe
from tests.test_moe_gpu import IDS, crafted_logits, inputs
from tests.test_moe_w8_gpu import ratio_to_bound
from tests.test_weight_fp8_gpu import DEV, DTYPES, GUARD, SENT16

pytestmark = pytest.mark.gpu


def run(x, logits, q, k, renorm, **kw):
    return moe.moe_rows_grouped_w8(x, logits, *q, k, renorm, torch.empty_like(x), **kw)


@pytest.mark.parametrize("variant", ["random", "same", 64, 65, 128, 129])
@pytest.mark.parametrize("H, I", [(64, 32), (192, 96), (320, 160), (704, 544)])
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grouped_fp8_mlp_is_inside_the_error_bound_of_the_definition(dtype, E, k, H, I, variant):
    """|y - moe_reference(dequantized)| <= moe_error_bound(dequantized) elementwise, both routed by the logits the device used, no row
    left out.  T = 130 and 300 at (4, 2) are row tiles of 64 and of 128; a number as variant puts exactly that many rows on expert 1
    (full tiles, and one row more).  The (H, I) give one step to eleven (the three-stage ring turns more than three times), last steps
    with zero-filled chunks, and half-live channel tiles.  Up rows in front of gate rows miss by > 100 bounds: every eighth output
    channel is a probe as in tests/moe_stress_cases.py (its down row holds one weight, +-0.25), because over dense channels the
    bound's sums of absolute products grow like I and the output like sqrt(I) -- measured on dense channels alone at (704, 544): 40 ..
    100 bounds, at the other shapes 125 and more."""
    probe = torch.arange(5, H, 8)
    for T in (1, 130, 300):
        x, router, gate_up, down = inputs(T, E, H, I, dtype, 7 * T + E)
        val = torch.where(down[:, probe, (7 * probe) % I] < 0, -0.25, 0.25).to(dtype)
        down[:, probe] = 0
        down[:, probe, (7 * probe) % I] = val
        q = moe.quantize_experts(gate_up, down)
        logits = torch.nn.functional.linear(x, router)
        if isinstance(variant, int):
            logits[:, 1] = -50
            logits[:variant, 1] = 50
        else:
            logits = crafted_logits(logits, variant, k)
        y = run(x, logits, q, k, True)
        ratio, top = ratio_to_bound(y, x, logits, q, k)
        print(f"T {T}: max err / bound {ratio:.3f}")
        assert top > 0.01 and ratio <= 1, T
    swapped = ratio_to_bound(y, x, logits, q, k, gate_up=lambda w: torch.cat([w[:, I:], w[:, :I]], 1))[0]
    print(f"gate and up rows swapped: max miss / bound {swapped:.1f}")
    assert swapped > 100


def test_every_code_at_every_byte_position_of_a_step():
    """test_moe_w8_gpu.py's construction in ONE grouped call of 512 rows (f16): row t holds one non-zero element, at kt = t % 256, and
    chooses experts 8 (t // 32) .. + 7 with equal weights; expert e's up matrix has one non-zero row n_e = e % 32.  g, u and the down sum
    of a slot are single products of the gate code (e + kt) % 128, the (negative) up code of the mirrored magnitude and the down codes
    (h + n_e) % 256 at byte n_e: every finite code at every byte of a 64-byte tile row, so at every byte of a fragment and every chunk
    of the swizzle, under scales of mixed exponents.  A wrong code or byte moves a term by >= 2^-4 relative."""
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
    ratio, top = ratio_to_bound(run(x.to(DEV), logits.to(DEV), q, k, True), x, logits, q, k)
    print(f"max err / bound {ratio:.3f}, max |ref| {top:.1f}")
    assert top > 100 and ratio <= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_buffers_stay_intact_calls_repeat_and_rows_are_independent(dtype):
    T, E, k, H, I = 300, 8, 2, 192, 96
    x, router, gate_up, down = inputs(T, E, H, I, dtype, 5)
    q = moe.quantize_experts(gate_up, down)
    need = int(_lib.load().hyd_moe_grouped_workspace_bytes(T, E, k, H, I, _lib.HYD_F16 if dtype == torch.float16 else _lib.HYD_BF16))

    def call(x, logits):
        yb = torch.full((T + 2, H + 24), SENT16, dtype=dtype, device=DEV)
        wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        moe.moe_rows_grouped_w8(x, logits, *q, k, False, yb[1:T + 1, 8:8 + H], workspace=wsb[GUARD:GUARD + need])
        torch.cuda.synchronize()
        assert bool((yb[0] == SENT16).all()) and bool((yb[T + 1] == SENT16).all()) and bool((yb[:, :8] == SENT16).all()) and bool((yb[:, 8 + H:] == SENT16).all())
        assert bool((wsb[:GUARD] == 0xA5).all()) and bool((wsb[GUARD + need:] == 0xA5).all()), "bytes around the workspace were written"
        return yb[1:T + 1, 8:8 + H].clone()

    logits = torch.nn.functional.linear(x, router)
    y = call(x, logits)
    assert torch.equal(y, call(x, logits)) and bool(torch.isfinite(y).all())
    xn = x.clone()
    xn[5] = float("nan")
    yn = call(xn, logits)
    keep = torch.arange(T, device=DEV) != 5
    assert torch.equal(yn[keep], y[keep]) and bool(torch.isnan(yn[5]).all())
    wide = torch.full((T, H + 8), float("nan"), dtype=dtype, device=DEV)
    wide[:, :H] = x
    assert torch.equal(call(wide[:, :H], logits), y)


def test_moe_mlp_and_the_module_take_the_grouped_fp8_call_where_asked():
    """grouped=True: hyd_moe_mlp_grouped_w8 per chunk of 2048 rows at 600 and at 2049 rows (y, ids, weights), eagerly and from a graph;
    grouped=False: the 128-row calls; 4-bit experts: ValueError; MoeMLP with Fp8Experts: the grouped call from
    MOE_GROUPED_W8_MIN_ROWS rows on, the 128-row calls below (and at 2048 rows where the measurement left no threshold)."""
    E, k, H, I, big = 8, 2, 64, 32, moe.MOE_GROUPED_MAX_ROWS
    x, router, gate_up, down = inputs(big + 1, E, H, I, torch.bfloat16, 11)
    logits = torch.nn.functional.linear(x, router)
    q = moe.quantize_experts(gate_up, down)
    kw = dict(gate_up_scale=q[1], down_scale=q[3])

    def chunks(T, rows_fn, step):
        parts = []
        for r in range(0, T, step):
            ids, w = (torch.empty((min(T, r + step) - r, k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32))
            parts.append((rows_fn(x[r:r + step][:T - r], logits[r:r + step][:T - r], *q, k, True, torch.empty_like(x[r:r + step][:T - r]), ids, w), ids, w))
        return [torch.cat(p) for p in zip(*parts)]

    for T in (600, big + 1):
        got = moe.moe_mlp(x[:T], router, q[0], q[2], k, True, return_routing=True, grouped=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, chunks(T, moe.moe_rows_grouped_w8, big)))
    assert torch.equal(moe.moe_mlp(x[:600], router, q[0], q[2], k, True, grouped=False, **kw), chunks(600, moe.moe_rows_w8, moe.MOE_MAX_ROWS)[0])
    q4 = moe.quantize_experts_fp4(gate_up, down)
    with pytest.raises(ValueError):
        moe.moe_mlp(x[:600], router, q4[0], q4[3], k, True, grouped=True, gate_up_shift=q4[1], gate_up_scale=q4[2], down_shift=q4[4], down_scale=q4[5])

    eager = moe.moe_mlp(x[:600], router, q[0], q[2], k, True, grouped=True, **kw)  # (the workspace exists before the capture)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = moe.moe_mlp(x[:600], router, q[0], q[2], k, True, grouped=True, **kw)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)

    mlp = moe.MoeMLP(H, I, E, k, True).to(DEV).to(torch.bfloat16)
    mlp.gate.weight.data, mlp.experts = router, moe.Fp8Experts(*q)
    at = moe.MOE_GROUPED_W8_MIN_ROWS
    if at is None:
        assert torch.equal(mlp(x[:big]), chunks(big, moe.moe_rows_w8, moe.MOE_MAX_ROWS)[0])
    else:
        assert torch.equal(mlp(x[:at]), chunks(at, moe.moe_rows_grouped_w8, big)[0])
        assert torch.equal(mlp(x[:at - 1]), chunks(at - 1, moe.moe_rows_w8, moe.MOE_MAX_ROWS)[0])
