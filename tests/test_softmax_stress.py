"""CPU companion of tests/test_softmax_stress_gpu.py: what the case builders of tests/softmax_stress_cases.py promise, checked
without a GPU.  Closed forms of the patterns that have one; the route table against the restated launcher rules; and, for every
(route, pattern, dtype), that the bounds the GPU tests hold the kernels to are ATTAINABLE on these inputs: the reference's own
rounding model (probabilities and the result rounded to the 16-bit dtype, everything else float64) stays within HALF of them.
That is a condition the inputs meet, not a tolerance to tune: a pattern that misses it is redesigned."""
import numpy as np
import pytest

from oracle import hydragen_oracle as O
from tests import softmax_stress_cases as S
from tests.gpu_util import ATOL, REL_L2, atol

NB = 8  # sequences per case here: the listed lengths, the empty one and one drawn at random

ROUND = {"f16": O.round_fp16, "bf16": O.round_bf16}


def err_over_bound(got, want, dt):
    """(max abs error / its bound, relative L2 / its bound) with the bounds of gpu_util.assert_close_l2"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = ATOL["f16"] * max(1.0, float(np.abs(want).max())) if dt == "f16" else atol(dt, want)
    l2 = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    return np.abs(got - want).max() / bound, l2 / REL_L2[dt]


def test_route_labels_follow_the_launcher_rules():
    for name, (B, Hq, Hkv, cap, D, nq, key, what) in S.SUFFIX_ROUTES.items():
        assert S.suffix_route(B, Hq, Hkv, cap, D, nq) == key, name
    for name, (B, Hq, Hkv, cap, lead, key, what) in S.PARTIAL_ROUTES.items():
        n_pre = min(lead, 2)
        assert S.suffix_route(B, Hq, Hkv, cap, 128, 1, n_pre) == key, name
    keys = {r[6] for r in S.SUFFIX_ROUTES.values()} | {r[5] for r in S.PARTIAL_ROUTES.values()}
    # every route the issue's table names: token-row 4 waves / TS = 2 / TS = 4 / n_pre = 2, one-unit-per-wave few_units / R = 2 /
    # R = 4 / packed, grouped-query one wave / four waves
    assert {"rows/4wps", "rows/ts2", "rows/ts4", "rows/npre2", "unit/R1/4-waves", "unit/R2/4-waves", "unit/R4/4-waves",
            "unit/R1/1-wave+packed", "gqa/1-wave", "gqa/4-waves"} <= keys
    for D in (64, 256):  # one row each for the token-row and the grouped-query kernel
        assert {r[6].split("/")[0] for r in S.SUFFIX_ROUTES.values() if r[4] == D} >= {"rows", "gqa"}
    assert set(S.DOT_PRODUCT_PARTIAL_ROUTES) | set(S.GQA_PARTIAL_ROUTES) == set(S.PARTIAL_ROUTES)


@pytest.mark.parametrize("route", list(S.SUFFIX_ROUTES))
def test_every_table_holds_the_listed_lengths(route):
    B, Hq, Hkv, cap = S.SUFFIX_ROUTES[route][:4]
    lens = S.score_case(route, "ties", "f16")["lens"]
    assert set(x for x in S.LISTED_LENS if x < cap) | {cap, 0} <= set(lens.tolist()) and lens.max() <= cap
    assert len(lens) == S.block_size(B) and len(lens) >= min(B, 6 + 1 + 1)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_ties_and_last_key_spike_have_their_closed_forms(dt):
    for route in ("gqa_1wave", "unit_r2", "rows_d64"):
        Hq, nq = S.SUFFIX_ROUTES[route][1], S.SUFFIX_ROUTES[route][5]
        c = S.score_case(route, "ties", dt, NB)
        out, lse = O.flash_attention_seqlen(c["q"], c["k"], c["v"], c["lens"])
        want, wlse = S.ties_closed_form(c["v"], c["lens"], Hq, nq)
        has = c["lens"] > 0
        assert np.abs(out[has] - want[has]).max() <= 1e-12 and np.abs(lse[has] - wlse[has]).max() <= 1e-12
        c = S.score_case(route, "last_key_spike", dt, NB)
        out, _ = O.flash_attention_seqlen(c["q"], c["k"], c["v"], c["lens"])
        g = Hq // c["v"].shape[2]
        for b, n in enumerate(c["lens"]):
            if n:
                assert np.abs(out[b] - np.repeat(c["v"][b, n - 1], g, axis=0)[None]).max() <= 1e-6, (route, b)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("pattern", S.SCORE_PATTERNS)
@pytest.mark.parametrize("route", list(S.SUFFIX_ROUTES))
def test_reference_rounding_model_meets_half_the_bounds_on_score_patterns(route, pattern, dt):
    c = S.score_case(route, pattern, dt, NB)
    has = c["lens"] > 0
    want, wlse = O.flash_attention_seqlen(c["q"], c["k"], c["v"], c["lens"])
    assert np.isfinite(want).all() and np.isfinite(wlse[has]).all()
    assert np.abs(wlse[has]).max() <= (S.MAX_SCORE + 8) * np.log(2.0)
    model, _ = O.flash_attention_seqlen(c["q"], c["k"], c["v"], c["lens"], round_p=ROUND[dt])
    ra, rl = err_over_bound(ROUND[dt](model)[has], want[has], dt)
    assert ra <= 0.5 and rl <= 0.5, f"{route} {pattern} {dt}: max abs at {ra:.2f} of its bound, relative L2 at {rl:.2f}"


def test_spike_behind_length_puts_finite_giants_behind_every_short_sequence():
    c = S.score_case("gqa_1wave", "spike_behind_length", "bf16", NB)
    D, p = c["D"], S.per(c["D"])
    s = np.einsum("bhd,bkgd->bhgk", c["q"][:, 0].reshape(NB, 8, 4, D)[:, :, 0], c["k"]) * D ** -0.5 * S.LOG2E
    for b, n in enumerate(c["lens"]):
        if n < c["cap"]:
            behind, inside = s[b, :, :, n:], s[b, :, :, :n]
            assert np.isfinite(behind).all() and behind.min() > 80.0 and (n == 0 or inside.max() < 12.0), (b, n, p)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("pattern", S.LSE_PATTERNS)
@pytest.mark.parametrize("route", ["rows_npre2", "gqa_4waves"])  # a dot-product route and a grouped-query route
def test_reference_rounding_model_meets_half_the_bounds_on_lse_patterns(route, pattern, dt):
    counts = S.TIES_COUNTS if pattern == "ties" else (None,)
    for n in counts:
        c = S.merge_case(route, pattern, dt, n, nb=NB)
        assert len(c["kinds"]) == (7 if n is None else n)
        model = ROUND[dt](np.where(c["ok"][..., None], O.combine_lse(c["outs"] + [c["suffix_out"]], c["lses"] + [c["suffix_lse"]]), 0.0))
        if pattern == "all_empty":
            assert not c["ok"].any() and not c["want"].any()
            continue
        ok = c["ok"]
        ra, rl = err_over_bound(model[ok], c["want"][ok], dt)
        assert ra <= 0.5 and rl <= 0.5, f"{route} {pattern} {dt} n={n}: {ra:.2f} {rl:.2f}"
        if pattern == "ties":  # the arithmetic mean of the partials and the suffix attention
            mean = (np.sum([o.astype(np.float64) for o in c["outs"]], 0) + c["suffix_out"]) / (len(c["outs"]) + 1)
            assert np.abs(c["want"] - mean).max() <= 1e-6  # (the partial LSEs are the suffix LSE rounded to fp32)
        if pattern == "partials_empty":
            assert np.array_equal(c["want"][ok], c["suffix_out"][ok])
        if pattern == "far_apart":  # the dominant partial's out, wherever it sits
            dom = np.argmax(np.stack(c["lses"]), 0)
            pick = np.take_along_axis(np.stack(c["outs"]), dom[None, ..., None], 0)[0]
            assert np.abs(c["want"] - pick).max() <= 1e-30 and len(np.unique(dom)) == 4


def test_far_apart_on_far_below_scores_makes_the_suffix_negligible():
    c = S.merge_case("gqa_1wave", "far_apart", "bf16", scores="far_below", nb=NB)
    has = c["lens"] > 0
    assert c["suffix_lse"][has].max() < -30.0 and np.isfinite(c["want"]).all()


@pytest.mark.parametrize("pattern", S.LSE_PATTERNS)
def test_fp32_merge_formula_meets_half_the_combine_tolerance(pattern):
    """_combine_many's tolerance (tests/test_edge_gpu.py: rtol 2e-5, atol 2e-6) against combine_lse's formula in numpy float32"""
    for n in (2, 5, 64, 70):
        for D in (63, 129):
            c = S.combine_case(pattern, n, D)
            got = S.combine_f32(c["outs"], c["lses"]).astype(np.float64)
            assert (np.abs(got - c["want"]) <= 0.5 * (2e-6 + 2e-5 * np.abs(c["want"]))).all(), (pattern, n, D)
            if pattern == "all_empty":
                assert not got.any()


def test_fp8_cases_are_exact_in_e4m3_and_their_scales_are_mixed():
    grid = np.asarray([0.0, 2.0 ** -9, 0.0625, 0.0703125, 1.0, 1.125, 240.0, 448.0])
    assert np.array_equal(S.round_e4m3(grid), grid) and S.round_e4m3(1e4) == 448.0 and S.round_e4m3(1.0625) == 1.0
    for route in S.FP8_ROUTES:
        c = S.fp8_score_case(route, "two_equal_spikes", "bf16")
        for x, sc in ((c["k8"], c["k_scale"]), (c["v8"], c["v_scale"])):
            assert np.array_equal(S.round_e4m3(x), x) and np.abs(x).max() <= 448.0
            assert ((sc >= 2.0 ** -4) & (sc <= 2.0 ** 4)).all()
            pow2 = np.log2(sc) == np.round(np.log2(sc))
            assert pow2.sum() == len(sc) // 2
            deq = x * sc[None, None, :, None]
            assert np.array_equal(O.round_bf16(deq), deq) and np.array_equal(O.round_fp16(deq), deq)  # exact in both q dtypes


@pytest.mark.parametrize("mass", S.OPERATOR_MASS)
def test_operator_cases_put_the_mass_where_they_say(mass):
    c = S.operator_case("decode_gqa", mass, 300, 150, "bf16", levels=2)
    _, pl = O.attention_lse(c["q"].reshape(1, -1, 16, 128), c["shared_ks"][0], c["shared_vs"][0])
    pl = pl.transpose(0, 2, 1).reshape(4, 1, 16)
    _, ul = O.flash_attention_seqlen(c["q"], c["k"], c["v"], c["lens"])
    d = pl - ul
    if mass == "prefix":
        assert d.min() > 40.0
    elif mass == "suffix":
        assert d.max() < -40.0
    else:
        assert np.abs(d).max() <= 1e-3


# ---- the causal tail ----------------------------------------------------------------------------------------------------------
def test_causal_route_labels_follow_the_launcher_rules():
    for name, row in S.CAUSAL_ROUTES.items():
        assert S.causal_route(*S.causal_shape(name)) == row[6], name
        B, _, _, cap, _, T = S.causal_shape(name)
        assert B == len(S.causal_lengths(T, cap)) or (B > 64 and S.block_size(B) >= len(S.causal_lengths(T, cap))), name
    by_key = {}
    for name, row in S.CAUSAL_ROUTES.items():
        by_key.setdefault(row[6], []).append(row)
    # the matrix-core kernel with 4 / 2 / 1 kv heads per workgroup and four waves per unit, the dot-product kernel R = 2 with one and
    # four waves, R = 4 and R = 8 (D = 256 only)
    assert {"gqa/1-wave/hpw4", "gqa/1-wave/hpw2", "gqa/1-wave/hpw1", "gqa/4-waves", "unit/R2/1-wave", "unit/R2/4-waves", "unit/R4/4-waves",
            "unit/R8/4-waves"} <= set(by_key)
    assert any(r[3] >= 128 for r in by_key["gqa/1-wave/hpw2"])  # one wave per unit on a cache four-wave units would take
    assert any(r[3] >= 256 for r in by_key["gqa/4-waves"])  # every wave walks several 32-key tiles
    assert {r[4] for r in S.CAUSAL_ROUTES.values() if r[6].startswith("gqa")} == {64, 128, 256}
    assert {r[6] for r in S.CAUSAL_ROUTES.values() if r[4] == 256} == {"unit/R2/4-waves", "unit/R4/4-waves", "unit/R8/4-waves", "gqa/1-wave/hpw2"}
    assert all(S.CAUSAL_ROUTES[r][6].endswith("4-waves") for r in S.CAUSAL_MERGE_ROUTES)
    # a token count outside 2..8 is refused, never run without the limit
    assert S.causal_route(8, 4, 4, 40, 128, 1) == "refused" and S.causal_route(8, 4, 4, 40, 128, 9) == "refused"


@pytest.mark.parametrize("route", list(S.CAUSAL_ROUTES))
def test_causal_tables_hold_the_listed_lengths(route):
    B, Hq, Hkv, cap, D, T = S.causal_shape(route)
    c = S.causal_case(route, "ties", "f16")
    lens = c["lens"].tolist()
    want = {0, -2, 1, T - 1, T, T + 1, cap - 1, cap, cap + 3} | {x for x in (25, 26, 31, 32, 33, 33 + T - 1, 63, 64, 65, 127, 128, 129, 128 + T - 1) if x <= cap + 3}
    assert want <= set(lens) and len(lens) == S.block_size(B)
    assert any(0 < n < T for n in lens)  # a sequence shorter than the step: tokens whose limit is <= 0 beside tokens that see keys
    lim = c["lim"]
    assert lim.min() == 0 and lim.max() == cap and (lim[:, -1] == np.clip(c["lens"], 0, cap)).all() and (np.diff(lim, axis=1) >= 0).all()
    for dst, src in c["twins"]:  # the clamps: the same data at length cap + 3 / cap and at -2 / 0
        assert all(np.array_equal(c[x][dst], c[x][src]) for x in "qkv") and (lim[dst] == lim[src]).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_causal_patterns_have_their_closed_forms(dt):
    for route in ("gqa_hpw2", "unit_r2_4waves", "gqa_4waves_tiles", "unit_d256_r8"):
        B, Hq, Hkv, cap, D, T = S.causal_shape(route)
        c = S.causal_case(route, "ties", dt)
        has = c["lim"] > 0
        out, lse = S.causal_reference(c["q"], c["k"], c["v"], c["lens"])
        want, wlse = S.causal_ties_closed_form(c["v"], c["lim"], Hq)
        assert np.abs(out - want).max() <= 1e-12 and np.abs(lse[has] - wlse[has]).max() <= 1e-12 and np.isneginf(lse[~has]).all()
        c = S.causal_case(route, "tail_staircase", dt)
        out, lse = S.causal_reference(c["q"], c["k"], c["v"], c["lens"])
        cf = S.staircase_closed_form(c["v"], c["lim"], Hq)
        assert np.abs(out - cf).max() <= 2e-4, (route, np.abs(out - cf).max())
        # an off-by-one limit in either direction returns another V row: the neighbours differ by far more than any bound
        for b, i in zip(*np.nonzero(c["lim"] > 1)):
            n = int(c["lim"][b, i])
            assert np.abs(c["v"][b, n - 1] - c["v"][b, n - 2]).max() > 0.5 and (n == cap or np.abs(c["v"][b, n - 1] - c["v"][b, n]).max() > 0.5)
        # the reference does not look behind a sequence's length, nor behind token 0's limit
        z = S.zero_behind_length(c["k"], np.clip(c["lens"], 0, cap))
        out0, lse0 = S.causal_reference(c["q"], z, c["v"], c["lens"])
        assert np.array_equal(out0, out) and np.array_equal(lse0, lse)
        c = S.causal_case(route, "giants_behind_row_limit", dt)
        out, lse = S.causal_reference(c["q"], c["k"], c["v"], c["lens"])
        out0, lse0 = S.causal_reference(c["q"], S.zero_from(c["k"], c["lim"][:, 0]), c["v"], c["lens"])
        assert np.array_equal(out0[:, 0], out[:, 0]) and np.array_equal(lse0[:, 0], lse[:, 0])
        assert T == 2 or not np.array_equal(out0[:, 1:], out[:, 1:])  # (the later tokens do see giants)


def test_causal_patterns_put_finite_giants_behind_the_limits():
    for route, pattern, low in (("gqa_hpw2", "giants_behind_row_limit", 80.0), ("gqa_hpw2", "tail_staircase", 180.0), ("unit_r2_4waves", "last_key_spike", 25.0)):
        B, Hq, Hkv, cap, D, T = S.causal_shape(route)
        c = S.causal_case(route, pattern, "bf16")
        g = Hq // Hkv
        s = np.einsum("bhd,bkhd->bhk", c["q"][:, 0].astype(np.float64), c["k"].astype(np.float64).repeat(g, 2)) * D ** -0.5 * S.LOG2E
        assert np.abs(s).max() <= S.MAX_SCORE
        seen = 0
        for b, n in enumerate(c["lim"][:, 0]):  # token 0: everything it sees is small, and a giant sits right behind its limit
            n_len = int(np.clip(c["lens"][b], 0, cap))
            if pattern == "last_key_spike":
                if n_len >= T:
                    assert s[b, :, n_len - 1].min() > low and s[b, :, :n].max() < 1.0
                    seen += 1
            elif n < cap:
                assert s[b, :, n:].min() > (low if pattern == "giants_behind_row_limit" else 20.0) and (n == 0 or s[b, :, :n].max() < 28.0)
                assert pattern != "tail_staircase" or n_len == cap or s[b, :, n_len:].min() > low
                seen += 1
        assert seen >= 10


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("pattern", S.CAUSAL_PATTERNS)
@pytest.mark.parametrize("route", list(S.CAUSAL_ROUTES))
def test_reference_rounding_model_meets_half_the_bounds_on_causal_cases(route, pattern, dt):
    c = S.causal_case(route, pattern, dt)
    has = c["lim"] > 0
    want, wlse = S.causal_reference(c["q"], c["k"], c["v"], c["lens"])
    assert np.isfinite(want).all() and np.isfinite(wlse[has]).all() and np.isneginf(wlse[~has]).all() and not want[~has].any()
    assert has.any() and (~has).any() and np.abs(wlse[has]).max() <= (S.MAX_SCORE + 8) * np.log(2.0)
    model, _ = S.causal_reference(c["q"], c["k"], c["v"], c["lens"], round_p=ROUND[dt])
    ra, rl = err_over_bound(ROUND[dt](model)[has], want[has], dt)
    print(f"model-ratio {route} {pattern} {dt}: {ra:.3f} {rl:.3f}")
    assert ra <= 0.5 and rl <= 0.5, f"{route} {pattern} {dt}: max abs at {ra:.2f} of its bound, relative L2 at {rl:.2f}"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("pattern", S.CAUSAL_LSE_PATTERNS)
@pytest.mark.parametrize("route", S.CAUSAL_MERGE_ROUTES)
def test_reference_rounding_model_meets_half_the_bounds_on_causal_merges(route, pattern, dt):
    c = S.causal_merge_case(route, pattern, dt)
    ok, fin = c["ok"], np.isfinite(c["suffix_lse"])
    model = ROUND[dt](np.where(ok[..., None], O.combine_lse(c["outs"] + [c["suffix_out"]], c["lses"] + [c["suffix_lse"]]), 0.0))
    if pattern == "all_empty":
        assert not ok.any() and not c["want"].any()
        return
    ra, rl = err_over_bound(model[ok], c["want"][ok], dt)
    assert ra <= 0.5 and rl <= 0.5, f"{route} {pattern} {dt}: {ra:.2f} {rl:.2f}"
    assert (fin == (c["lim"] > 0)[..., None]).all()
    if pattern == "partials_empty":
        assert np.array_equal(c["want"][ok], c["suffix_out"][ok]) and (ok == fin).all()
    else:  # tokens without a unique key (0 < len < T among them) that have finite partials: the merge of the partials alone
        lone = ok & ~fin
        assert lone.any() and (pattern == "suffix_empty" or (lone.any(1).any(1) & fin.any(1).any(1)).any())
        alone = O.combine_lse(c["outs"], c["lses"])
        assert np.abs(c["want"][lone] - alone[lone]).max() <= 1e-12
