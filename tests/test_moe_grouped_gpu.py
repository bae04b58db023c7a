"""-m gpu: the grouped mixture-of-experts call (csrc/moe_grouped.hip through moe.moe_rows_grouped) against the float64 definition and
its error bound, its routing at the largest slot count, buffers and repeatability, and the route through moe_mlp."""
import pytest
import torch

from hydragen_amd import _lib, moe
from tests.test_moe_gpu import IDS, crafted_logits, inputs
from tests.test_weight_fp8_gpu import DEV, DTYPES, GUARD, SENT16

pytestmark = pytest.mark.gpu


def run(x, logits, gate_up, down, k, renorm):
    ids, w = (torch.empty((x.shape[0], k), dtype=dt, device=DEV) for dt in (torch.int32, torch.float32))
    return moe.moe_rows_grouped(x, logits, gate_up, down, k, renorm, torch.empty_like(x), ids, w), ids, w


@pytest.mark.parametrize("variant", ["random", "same", 64, 65, 128, 129])
@pytest.mark.parametrize("H, I", [(64, 32), (64, 96), (192, 32), (192, 96), (320, 160)])
@pytest.mark.parametrize("E, k", [(4, 2), (128, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grouped_mlp_is_inside_the_error_bound_of_the_definition(dtype, E, k, H, I, variant):
    """|y - moe_reference| <= moe_error_bound elementwise, both routed by the logits the device used.  T = 130 and 300 at (4, 2) are
    row tiles of 64 and of 128; a number as variant puts exactly that many rows on expert 1 (full tiles, and one row more).  The
    (H, I) give one step and five, half steps, and half-live channel tiles.  Up rows in front of gate rows miss by > 100 bounds."""
    for T in (1, 130, 300):
        x, router, gate_up, down = inputs(T, E, H, I, dtype, 7 * T + E)
        logits = torch.nn.functional.linear(x, router)
        if isinstance(variant, int):
            logits[:, 1] = -50
            logits[:variant, 1] = 50
        else:
            logits = crafted_logits(logits, variant, k)
        y = run(x, logits, gate_up, down, k, True)[0].cpu().double()
        args = [t.cpu() for t in (x, router, gate_up, down)]
        ref = moe.moe_reference(*args, k, True, logits=logits.cpu())
        bound = moe.moe_error_bound(*args, k, True, logits=logits.cpu())
        ratio = float(((y - ref).abs() / bound).max())
        print(f"T {T}: max err / bound {ratio:.3f}")
        assert float(ref.abs().max()) > 0.01 and ratio <= 1, T
    args[2] = torch.cat([args[2][:, I:], args[2][:, :I]], 1)
    assert float(((y - moe.moe_reference(*args, k, True, logits=logits.cpu())).abs() / bound).max()) > 100


@pytest.mark.parametrize("T", [300, 2048])
@pytest.mark.parametrize("E, k", [(8, 2), (128, 8)])
def test_grouped_routing_is_the_definition(E, k, T):
    """ids exactly, weights within 4 2^-23 relative ((k + 5) 2^-23 renormalised); 2048 rows of k = 8 are the most slots of a call."""
    x, router, gate_up, down = inputs(T, E, 64, 32, torch.bfloat16, T + E)
    logits = torch.nn.functional.linear(x, router)
    for renorm in (True, False):
        _, ids, w = run(x, logits, gate_up, down, k, renorm)
        want_ids, want_w = moe.route_reference(logits.cpu(), k, renorm)
        assert torch.equal(ids.cpu().long(), want_ids)
        rel = float(((w.cpu().double() - want_w).abs() / want_w).max())
        print(f"renormalize {renorm}: max relative weight error {rel * 2 ** 23:.2f} x 2^-23")
        assert rel <= ((k + 5) if renorm else 4) * 2.0 ** -23


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grouped_buffers_stay_intact_calls_repeat_and_rows_are_independent(dtype):
    T, E, k, H, I = 300, 8, 2, 192, 96
    x, router, gate_up, down = inputs(T, E, H, I, dtype, 5)
    need = int(_lib.load().hyd_moe_grouped_workspace_bytes(T, E, k, H, I, _lib.HYD_F16 if dtype == torch.float16 else _lib.HYD_BF16))

    def call(x):
        yb = torch.full((T + 2, H + 24), SENT16, dtype=dtype, device=DEV)
        wsb = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        moe.moe_rows_grouped(x, torch.nn.functional.linear(x, router), gate_up, down, k, False, yb[1:T + 1, 8:8 + H], workspace=wsb[GUARD:GUARD + need])
        torch.cuda.synchronize()
        assert bool((yb[0] == SENT16).all()) and bool((yb[T + 1] == SENT16).all()) and bool((yb[:, :8] == SENT16).all()) and bool((yb[:, 8 + H:] == SENT16).all())
        assert bool((wsb[:GUARD] == 0xA5).all()) and bool((wsb[GUARD + need:] == 0xA5).all()), "bytes around the workspace were written"
        return yb[1:T + 1, 8:8 + H].clone()

    y = call(x)
    assert torch.equal(y, call(x)) and bool(torch.isfinite(y).all())
    xn = x.clone()
    xn[5] = float("nan")
    yn = call(xn)
    keep = torch.arange(T, device=DEV) != 5
    assert torch.equal(yn[keep], y[keep]) and bool(torch.isnan(yn[5]).all())


def test_moe_mlp_takes_the_grouped_call_from_its_threshold_on():
    """16-bit experts: the grouped call from MOE_GROUPED_MIN_ROWS rows on, the 128-row calls below; fp8 experts: the 128-row calls
    at both sizes; the grouped route captured in a graph replays to the eager bits."""
    E, k, H, I = 8, 2, 64, 32
    long, short = moe.MOE_GROUPED_MIN_ROWS + 88, moe.MOE_GROUPED_MIN_ROWS - 1
    x, router, gate_up, down = inputs(long, E, H, I, torch.bfloat16, 11)
    logits = torch.nn.functional.linear(x, router)
    q = moe.quantize_experts(gate_up, down)

    def chunks(T, rows_fn):
        return torch.cat([rows_fn(x[r:min(T, r + moe.MOE_MAX_ROWS)], logits[r:min(T, r + moe.MOE_MAX_ROWS)]) for r in range(0, T, moe.MOE_MAX_ROWS)])

    rows16 = lambda xs, ls: moe.moe_rows(xs, ls, gate_up, down, k, True, torch.empty_like(xs))  # noqa: E731
    rows8 = lambda xs, ls: moe.moe_rows_w8(xs, ls, q[0], q[1], q[2], q[3], k, True, torch.empty_like(xs))  # noqa: E731
    eager = moe.moe_mlp(x, router, gate_up, down, k, True)
    assert torch.equal(eager, run(x, logits, gate_up, down, k, True)[0])
    assert torch.equal(moe.moe_mlp(x[:short], router, gate_up, down, k, True), chunks(short, rows16))
    for T in (long, short):
        assert torch.equal(moe.moe_mlp(x[:T], router, q[0], q[2], k, True, gate_up_scale=q[1], down_scale=q[3]), chunks(T, rows8))
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        moe.moe_mlp(x, router, gate_up, down, k, True)  # the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        out = moe.moe_mlp(x, router, gate_up, down, k, True)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
