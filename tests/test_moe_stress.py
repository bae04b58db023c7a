"""-m "not gpu": the conditions tests/test_moe_stress_gpu.py rests on -- the steps its deep shapes give every wave, the expert counts of
its route variants, the properties its hard routing rows are named for, an fp32 emulation of a kernel inside the bound on every one of
its MLP cases (a correct kernel can pass them) with a swapped layout far outside, and the cost of the float64 reference."""
import time
from functools import lru_cache

import pytest
import torch

from hydragen_amd import moe
from tests import moe_stress_cases as cs


def test_deep_shapes_give_the_waves_the_steps_the_gpu_test_is_about():
    """moe.hip (64-deep steps): some wave hands a prefetched step over in both products of every deep shape, at (576, 544) every wave does
    so in both products with an uneven split, and 288 and 544 end on a half step (the `kc + 16 g < K` guard of a prefetched step).  The
    bound tests of tests/test_moe_gpu.py reach no second step.  fp8 and 4-bit: every wave one unit at least, some wave two."""
    assert cs.waves_steps(192, 64) == [0, 1, 1, 1] and cs.waves_steps(64, 64) == [0, 0, 0, 1] and max(cs.waves_steps(96, 64)) == 1
    want = {(512, 288): ([2, 2, 2, 2], [1, 1, 1, 2]), (576, 544): ([2, 2, 2, 3], [2, 2, 2, 3])}
    for H, I in cs.DEEP["rows"]:
        assert (cs.waves_steps(H, 64), cs.waves_steps(I, 64)) == want[(H, I)]
        assert max(cs.waves_steps(H, 64)) >= 2 and max(cs.waves_steps(I, 64)) >= 2 and I % 64 == 32
    # the grouped call's waves split the tile, not K: every wave runs all 9 steps of either product, the down product's last a half step
    assert cs.DEEP["grouped"] == [(576, 544)] and cs.STEP["grouped"] is None and -(-576 // 64) == -(-544 // 64) == 9 and 544 % 64 == 32
    assert min(min(p) for p in want[(576, 544)]) >= 2 and len(set(want[(576, 544)][0])) > 1
    assert (cs.waves_steps(704, 128), cs.waves_steps(544, 128)) == ([1, 2, 1, 2], [1, 1, 1, 2]) and cs.DEEP["w8"] == [(704, 544)]
    assert (cs.waves_steps(1344, 128), cs.waves_steps(1056, 128)) == ([2, 3, 3, 3], [2, 2, 2, 3]) and cs.DEEP["w4"] == [(1344, 1056)]
    for call in ("w8", "w4"):
        for K in cs.DEEP[call][0]:
            assert min(cs.waves_steps(K, cs.STEP[call])) >= 1 and max(cs.waves_steps(K, cs.STEP[call])) >= 2 and K % 128


def _counts(c):
    return torch.bincount(moe.route_reference(cs.build(c).logits, c.k, c.renorm)[0].flatten(), minlength=c.E)


def test_route_variants_yield_the_expert_counts_they_are_named_for():
    seen = set()
    for c in cs.all_mlp_cases():
        if (c.dtype, c.T, c.E, c.k, c.H, c.variant) in seen:
            continue
        seen.add((c.dtype, c.T, c.E, c.k, c.H, c.variant))
        n = _counts(c)
        assert int(n.sum()) == c.T * c.k
        if isinstance(c.variant, int):
            assert int(n[1]) == c.variant, c.id
        elif c.variant == "same":
            assert n[: c.k].tolist() == [c.T] * c.k, c.id
        elif c.variant == "last":
            assert n[c.E - c.k:].tolist() == [c.T] * c.k, c.id
        elif c.variant == "one_each":
            assert n[: c.T * c.k].tolist() == [1] * (c.T * c.k) and (c.T * c.k == c.E or c.E // c.k > cs.MAX_ROWS[c.call]), c.id
    variants = {c.variant for c in cs.all_mlp_cases()}
    assert variants == {"random", "same", "last", "one_each", 32, 33, 48, 49, 64, 65}
    # the grouped call's table at (256, 8, 32): 256 one-row tiles of its ceil(256 / 64) + 256 entries
    assert any(c.call == "grouped" and (c.E, c.k, c.T, c.variant) == (256, 8, 32, "one_each") for c in cs.all_mlp_cases())
    assert [c.T * c.k <= 16 for c in cs.boundary_cases("bf16")] == [True, True, True, False, False]


@pytest.mark.parametrize("dtype", list(cs.DTYPES))
@pytest.mark.parametrize("E, k", cs.HARD_ROUTES)
def test_hard_routing_rows_have_the_properties_they_are_named_for(E, k, dtype):
    names, logits = cs.hard_rows(E, k, dtype)
    row = dict(zip(names, logits))
    assert logits.dtype == cs.DTYPES[dtype] and logits.shape == (len(names), E) and ("ties_one_lane" in row) == (E > 64)
    assert not bool(torch.isnan(logits).any()) and bool(torch.isfinite(logits.float().max(1).values).all())
    ids, w = moe.route_reference(logits, k, False)
    ids, w = dict(zip(names, ids)), dict(zip(names, w))
    assert not bool(torch.isnan(torch.stack(list(w.values()))).any())
    for name in ("masked", "masked_max_finite"):
        masked = int(torch.isinf(row[name]).sum())
        assert 0 < masked < E - k and bool(torch.isfinite(row[name][ids[name]]).all())
    top = float(torch.finfo(cs.DTYPES[dtype]).max)
    for name in ("max_finite", "masked_max_finite"):
        assert row[name][ids[name]].tolist() == [top] * (k - 1) + [0.0] and float(w[name][-1]) == 0.0
        low = float((row[name].float() - row[name].float().max()).min())  # `v - top` in fp32: bfloat16's overflows, float16's is 2^17 below
        assert low == (float("-inf") if dtype == "bf16" or name == "masked_max_finite" else -2 * top)
    assert int(ids["denormal_gap"][0]) == E - 1 and bool((w["denormal_gap"][1:] < 2.0 ** -126).all()) and bool((w["denormal_gap"][1:] > 0).all())
    gaps = -row["denormal_gap"][ids["denormal_gap"][1:]].double()
    assert float(gaps.min()) >= 88 and float(gaps.max()) <= 104
    sub = row["subnormal"].double().abs()
    assert float(sub.max()) < float(torch.finfo(cs.DTYPES[dtype]).tiny) and int((sub > 0).sum()) > E // 2
    assert bool(torch.signbit(row["subnormal"][sub == 0]).any()) and not bool(torch.signbit(row["subnormal"][sub == 0]).all())
    if E > 64:
        tied = (row["ties_one_lane"] == row["ties_one_lane"].max()).nonzero()[:, 0]
        assert len(tied) == -(-E // 64) >= 2 and len(set((tied % 64).tolist())) == 1 and ids["ties_one_lane"][: min(k, len(tied))].tolist() == tied[:k].tolist()
    assert int(ids["last_chunk_winner"][0]) == E - 1


def _unique_inputs():
    seen, out = set(), []
    for c in cs.all_mlp_cases():
        key = c._replace(call="rows") if c.call == "grouped" else c
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@lru_cache(maxsize=1)
def _survey():
    """(case, err / bound of the emulation, err / bound of the emulation against the swapped definition, max |ref|, finite) per input set"""
    out = []
    for c in _unique_inputs():
        b = cs.build(c)
        ref, bound = cs.reference_and_bound(c, b)
        y = cs.emulate_fp32(b.x, b.logits, b.gate_up, b.down, c.k, c.renorm, cs.STEP[c.call])
        miss = (y - cs.swapped_reference(c, b)).abs() / bound
        out.append((c, float(((y - ref).abs() / bound).max()), float(miss.max()), float(ref.abs().max()), bool(torch.isfinite(y).all())))
    return out


def test_the_one_walk_reference_and_bound_are_the_two_functions():
    cases = [cs.deep_cases("rows", "f16", 512, 288)[1], cs.deep_cases("grouped", "bf16", 576, 544)[0], cs.route_cases("grouped", "f16", 256, 8)[3]]
    cases += [cs.route_cases("rows", "bf16", 8, 8)[5]] + [cs.quantized_route_cases(call, dt)[0] for call, dt in (("w8", "f16"), ("w4", "bf16"))]
    assert {c.renorm for c in cases} == {True, False} and {c.call for c in cases} == set(cs.STEP)
    for c in cases:
        b = cs.build(c)
        ref, bound = cs.reference_and_bound(c, b)
        args = (b.x, b.router, b.gate_up, b.down, c.k, c.renorm)
        want_ref, want_bound = moe.moe_reference(*args, logits=b.logits), moe.moe_error_bound(*args, logits=b.logits)
        swapped = moe.moe_reference(b.x, b.router, torch.cat([b.gate_up[:, c.I:], b.gate_up[:, :c.I]], 1), b.down, c.k, c.renorm, logits=b.logits)
        assert float(((cs.swapped_reference(c, b) - swapped).abs() / want_bound).max()) <= 1e-12
        assert float(((ref - want_ref).abs() / want_bound).max()) <= 1e-12 and float((bound / want_bound - 1).abs().max()) <= 1e-12, c.id


def test_the_emulation_is_inside_the_bound_on_every_case():
    """No row left out: ratio <= 1 everywhere, so a correct kernel passes the GPU test's inputs."""
    for c, ratio, _, top, finite in _survey():
        assert top > 0.01 and finite and ratio <= 1, (c.id, ratio)
    for deep in (False, True):
        print(f"{'deep' if deep else 'shallow'} shapes: largest err / bound of the emulation {max(r for c, r, *_ in _survey() if (c.H > 192) == deep):.3f}")


@pytest.mark.parametrize("group", ["shallow", "rows", "grouped", "w8", "w4"])
def test_a_swapped_layout_is_more_than_100_bounds_outside(group):
    """Up rows in front of gate rows in the definition, on every case: 293 bounds (one row, E = k = 1, bfloat16) to several thousand; the
    deep shapes 720 (4-bit, (1344, 1056)) and more.  It is the probe channels of cs._weights that carry this at depth: over the dense
    channels alone the swap is 14 .. 157 bounds away at the deep shapes, since the bound's sums of absolute products grow like I and the
    output like sqrt(I)."""
    cases = [(c, miss) for c, _, miss, *_ in _survey() if (group == "shallow") == (c.H <= 192) and group in ("shallow", c.call)]
    print(f"{group}: {len(cases)} input sets, the swapped layout misses by {min(m for _, m in cases):.0f} .. {max(m for _, m in cases):.0f} bounds")
    for c, miss in cases:
        assert miss > 100, (c.id, miss)


@pytest.mark.parametrize("T, E, k, H, I", [(128, 8, 2, 512, 288), (64, 256, 8, 512, 32)])
def test_the_float64_reference_and_bound_are_cheap(T, E, k, H, I):
    c = cs.Case("rows", "bf16", T, E, k, H, I, "random")
    b = cs.build(c)
    dt = float("inf")
    for _ in range(2):  # (the first call also converts the weights to float64, once for all the cases that share them)
        t0 = time.perf_counter()
        cs.reference_and_bound(c, b)
        dt = min(dt, time.perf_counter() - t0)
    print(f"reference and bound: {dt:.3f} s")
    assert dt < 0.4
