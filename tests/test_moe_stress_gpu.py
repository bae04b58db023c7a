"""-m gpu: the four expert calls (moe.moe_rows, moe_rows_grouped, moe_rows_w8, moe_rows_w4) and moe_mlp on the cases of
tests/moe_stress_cases.py -- waves with several steps under second passes and partly filled tiles, route shapes the grouping treats
specially, strided x, a workspace reused across routings and shapes, hard routing rows, and moe_mlp's second grouped chunk.  Every MLP
comparison is |y - moe_reference| <= moe_error_bound elementwise with no row excused (tests/test_moe_stress.py shows on the CPU that an
fp32 evaluation in a kernel's order fits)."""
import pytest
import torch

from hydragen_amd import _lib, moe
from tests import moe_stress_cases as cs
from tests.test_weight_fp8_gpu import DEV, GUARD, SENT16

pytestmark = pytest.mark.gpu
CALLS = {"rows": moe.moe_rows, "grouped": moe.moe_rows_grouped, "w8": moe.moe_rows_w8, "w4": moe.moe_rows_w4}
DT = list(cs.DTYPES)


def run_call(call, x, logits, weights, k, renorm, out=None, **kw):
    return CALLS[call](x, logits, *weights, k, renorm, torch.empty_like(x) if out is None else out, **kw)


def on_device(b):
    return b.x.to(DEV), b.logits.to(DEV), tuple(t.to(DEV) for t in b.weights)


def held(cases):
    """Every case inside the bound; returns the largest ratio."""
    worst = 0.0
    for c in cases:
        b = cs.build(c)
        x, logits, weights = on_device(b)
        y = run_call(c.call, x, logits, weights, c.k, c.renorm).cpu().double()
        ref, bound = cs.reference_and_bound(c, b)
        ratio = float(((y - ref).abs() / bound).max())
        print(f"{c.id}: max err / bound {ratio:.3f}")
        assert float(ref.abs().max()) > 0.01 and bool(torch.isfinite(y).all()) and ratio <= 1, (c.id, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("call, H, I", [(call, H, I) for call, shapes in cs.DEEP.items() for H, I in shapes])
@pytest.mark.parametrize("dtype", DT)
def test_deep_products_are_inside_the_bound(dtype, call, H, I):
    """Every wave's prefetch and hand-over (cs.waves_steps: tests/test_moe_stress.py lists the steps), a half-step tail, and with them a
    second pass over `red`, half-filled and one-row tiles, full and one-row row tiles of the grouped call, and one plain-softmax case."""
    print(f"deep {call} {dtype} ({H}, {I}): largest err / bound {held(cs.deep_cases(call, dtype, H, I)):.3f}")


@pytest.mark.parametrize("E, k", cs.ROUTE_SHAPES)
@pytest.mark.parametrize("call", ["rows", "grouped"])
@pytest.mark.parametrize("dtype", DT)
def test_route_shapes_are_inside_the_bound(dtype, call, E, k):
    """k = 1 (no addition in the combine), k = E, E = 1 and E = 256 (the group kernel's arrays to their end); scattered slots, every slot on
    the highest experts (the grouped call's last wave places its own tiles and clears the table's tail), and one slot per expert (the grouped
    call at (256, 8): 256 one-row tiles in a table of 260)."""
    print(f"route shapes {call} {dtype} E {E} k {k}: largest err / bound {held(cs.route_cases(call, dtype, E, k)):.3f}")


@pytest.mark.parametrize("dtype", DT)
def test_the_one_tile_two_tile_dispatch_boundary_is_inside_the_bound(dtype):
    print(f"MT boundary {dtype}: largest err / bound {held(cs.boundary_cases(dtype)):.3f}")


@pytest.mark.parametrize("call", ["w8", "w4"])
@pytest.mark.parametrize("dtype", DT)
def test_quantized_calls_on_the_highest_experts_and_with_one_expert_per_row(dtype, call):
    print(f"routes {call} {dtype}: largest err / bound {held(cs.quantized_route_cases(call, dtype)):.3f}")


def _need(call, T, E, k, H, I, dtype):
    query = _lib.load().hyd_moe_grouped_workspace_bytes if call == "grouped" else _lib.load().hyd_moe_workspace_bytes
    return int(query(T, E, k, H, I, _lib.HYD_F16 if dtype == "f16" else _lib.HYD_BF16))


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("dtype", DT)
def test_strided_x_is_the_contiguous_call(dtype, call):
    """x as a view with row stride H + 8 and H + 64 inside a NaN-filled buffer (a kernel that stepped by H would read NaN), out strided
    between sentinels: the bits of the contiguous call.  A single row of such a buffer is passed with stride H (one row: the stride is
    never used), so T = 1 holds the view's base pointer only."""
    E, k, H, I = 8, 2, 192, 96
    for T in (130 if call == "grouped" else 33, 1):
        b = cs.build(cs.Case(call, dtype, T, E, k, H, I, "random"))
        x, logits, weights = on_device(b)
        want = run_call(call, x, logits, weights, k, True)
        assert bool(torch.isfinite(want).all())
        for pad in (8, 64):
            xb = torch.full((T + 2, H + pad), float("nan"), dtype=x.dtype, device=DEV)
            xb[1:T + 1, :H] = x
            yb = torch.full((T + 2, H + 24), SENT16, dtype=x.dtype, device=DEV)
            xs = xb[1:T + 1, :H]
            assert xs.stride(0) == H + pad and (T == 1 or not xs.is_contiguous())
            run_call(call, xs, logits, weights, k, True, out=yb[1:T + 1, 8:8 + H])
            torch.cuda.synchronize()
            assert torch.equal(yb[1:T + 1, 8:8 + H], want), (T, pad)
            assert bool((yb[0] == SENT16).all()) and bool((yb[T + 1] == SENT16).all()) and bool((yb[:, :8] == SENT16).all()) and bool((yb[:, 8 + H:] == SENT16).all())


@pytest.mark.parametrize("call", list(CALLS))
def test_a_reused_workspace_gives_the_bits_of_a_fresh_one(call):
    """One workspace of the larger need through a scattered routing, a concentrated one, a smaller T with another layout (and, grouped,
    another tile height) and the first again: each the bits of the same call on a fresh 0xA5-filled workspace of its own size.  The grouped
    call's tile table is valid only up to where its last wave clears it; stale entries of the scattered call lie behind."""
    dtype, E, k, H, I = "bf16", 8, 2, 192, 96
    big, small = (300, 130) if call == "grouped" else (128, 17)
    shared = torch.full((_need(call, big, E, k, H, I, dtype) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    for T, variant in ((big, "random"), (big, "same"), (small, "random"), (big, "random")):
        x, logits, weights = on_device(cs.build(cs.Case(call, dtype, T, E, k, H, I, variant)))
        need = _need(call, T, E, k, H, I, dtype)
        fresh = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
        want = run_call(call, x, logits, weights, k, True, workspace=fresh)
        got = run_call(call, x, logits, weights, k, True, workspace=shared[GUARD:-GUARD])
        torch.cuda.synchronize()
        assert torch.equal(got, want) and bool(torch.isfinite(want).all()), (T, variant)
    assert bool((shared[:GUARD] == 0xA5).all()) and bool((shared[-GUARD:] == 0xA5).all()), "bytes around the workspace were written"


@pytest.mark.parametrize("E, k", cs.HARD_ROUTES)
@pytest.mark.parametrize("call", ["rows", "grouped"])
@pytest.mark.parametrize("dtype", DT)
def test_hard_routing_rows_route_as_the_definition(dtype, call, E, k):
    """cs.hard_rows: ids exactly route_reference's; weights within 4 2^-23 relative ((k + 5) 2^-23 renormalised) wherever the wanted weight
    is a normal fp32 number, and within 2^-126 absolutely below (whether expf flushes a denormal is the math library's business; a wanted 0
    is 0 or inside that floor); no NaN (every row has a finite maximum).  The grouped call takes the rows repeated to 130."""
    names, rows = cs.hard_rows(E, k, dtype)
    if call == "grouped":
        rows = rows.repeat(-(-130 // len(names)), 1)[:130]
    T = rows.shape[0]
    x, _, weights = on_device(cs.build(cs.Case(call, dtype, T, E, k, 64, 32, "random")))
    for renorm in (True, False):
        ids, w = (torch.empty((T, k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32))
        y = run_call(call, x, rows.to(DEV), weights, k, renorm, ids_out=ids, weights_out=w)
        want_ids, want_w = moe.route_reference(rows, k, renorm)
        w = w.cpu().double()
        wrong = (ids.cpu().long() != want_ids).any(1).nonzero()[:, 0].tolist()
        assert not wrong, [names[t % len(names)] for t in wrong]
        assert not bool(torch.isnan(w).any()) and not bool(torch.isnan(y).any())
        normal = want_w >= 2.0 ** -126
        rel = float(((w - want_w).abs() / want_w)[normal].max())
        low = float((w - want_w).abs()[~normal].max()) if bool((~normal).any()) else 0.0
        print(f"renormalize {renorm}: max relative weight error {rel * 2 ** 23:.2f} x 2^-23, below fp32's normal range {low / 2.0 ** -126:.3f} x 2^-126")
        assert rel <= ((k + 5) if renorm else 4) * 2.0 ** -23 and low <= 2.0 ** -126


@pytest.mark.parametrize("T", [2049, 2648])
def test_long_moe_mlp_takes_a_second_grouped_chunk(T):
    """Past MOE_GROUPED_MAX_ROWS: y, ids and weights are moe_rows_grouped's per chunk of 2048 rows -- at 2049 the second chunk is a
    one-row call with another tile height and another workspace --, and the last chunk is inside the bound."""
    c = cs.Case("grouped", "bf16", T, 8, 2, 64, 32, "random")
    b = cs.build(c)
    x, _, (gate_up, down) = on_device(b)
    router = b.router.to(DEV)
    y, ids, w = moe.moe_mlp(x, router, gate_up, down, c.k, True, return_routing=True)
    logits = torch.nn.functional.linear(x, router)
    for r in range(0, T, moe.MOE_GROUPED_MAX_ROWS):
        rows = slice(r, min(T, r + moe.MOE_GROUPED_MAX_ROWS))
        ic, wc = (torch.empty((rows.stop - r, c.k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32))
        yc = moe.moe_rows_grouped(x[rows], logits[rows], gate_up, down, c.k, True, torch.empty_like(x[rows]), ic, wc)
        assert torch.equal(y[rows], yc) and torch.equal(ids[rows], ic) and torch.equal(w[rows], wc), r
    assert r == 2048 and y.shape == (T, c.H)
    args = (b.x[rows], b.router, b.gate_up, b.down, c.k, True)
    ref, bound = moe.moe_reference(*args, logits=logits[rows].cpu()), moe.moe_error_bound(*args, logits=logits[rows].cpu())
    ratio = float(((y[rows].cpu().double() - ref).abs() / bound).max())
    print(f"T {T}: the last chunk's {T - r} rows, max err / bound {ratio:.3f}")
    assert float(ref.abs().max()) > 0.01 and ratio <= 1
