"""CPU companion of tests/test_prefix_stress_gpu.py: what tests/prefix_stress_cases.py promises, checked without a GPU.  Every
PREFIX_ROUTES row reaches the body its key names, by `prefix_route` on the library's own plan; the closed forms agree with the
float64 oracle; the patterns put things where they say; and for every (route, pattern, dtype) the bounds the GPU tests use are
ATTAINABLE: the reference's own rounding model (probabilities and the result rounded to the 16-bit dtype, everything else float64)
stays within HALF of them.  That is a condition the inputs meet, not a tolerance to tune: a pattern that misses it is redesigned."""
import numpy as np
import pytest

from tests import prefix_stress_cases as P
from tests.softmax_stress_cases import MAX_SCORE
from tests.test_softmax_stress import err_over_bound

ROUTES = list(P.PREFIX_ROUTES)


def lse_over_bound(got, want):
    """|lse - want| over the GPU tests' bound 2e-3 + 1e-5 |want|"""
    return float((np.abs(got - want) / (2e-3 + 1e-5 * np.abs(want))).max()) if got.size else 0.0


# ---- the route table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_every_row_reaches_the_route_its_key_names(route):
    r, pl = P.PREFIX_ROUTES[route], P.route_plan(route)
    assert pl["key"] == r["key"], (route, pl)
    assert pl["persistent"] == (r["entry"] == "decode") and (not pl["persistent"] or not r["causal"])
    # the last workgroup is ragged and one of its waves has only SOME valid lanes
    assert pl["mrows"] % pl["wg_rows"] and pl["mrows"] % 32, (route, pl["mrows"])
    assert r["sb"] % r["nb"] == 0 and r["sb"] * r["Hkv"] * pl["row_blocks"] * pl["num_splits"] == pl["grid"]
    if r["splits"] == 3:
        assert pl["num_splits"] == 3
    if r["splits"] == 0:
        assert pl["num_splits"] > 1, "the planner does not split this row"
    if r["entry"] == "decode":  # 3 workgroups walk 3, 3 and 2 units
        assert pl["grid"] == 8 and r["wgs"] == 3


def test_the_table_holds_every_body_and_form():
    rows = P.PREFIX_ROUTES
    plans = {n: P.route_plan(n) for n in rows}
    keys = {r["key"] for r in rows.values()}
    assert {"w8/kg2", "w8/kg1", "w4/kg2", "w4/kg1", "w4/d256", "w4/persist", "w4/kg2+persist"} == keys
    assert {r["D"] for r in rows.values()} == {64, 128, 256}
    for D in (64, 128):  # both workgroup heights
        assert {plans[n]["wg_rows"] for n, r in rows.items() if r["D"] == D} == {128, 256}
    assert {plans[n]["wg_rows"] for n, r in rows.items() if r["D"] == 256} == {128}
    # a causal variant of every non-persistent row that has a causal form (cu_seqlens_k rows hold several sequences per group: none)
    for n, r in rows.items():
        if r["entry"] in ("flash", "split", "varlen") and not r["causal"]:
            twin = rows[n + "_causal"]
            assert twin["causal"] and {k: v for k, v in twin.items() if k not in ("causal", "rule")} == {k: v for k, v in r.items() if k not in ("causal", "rule")}
            assert plans[n + "_causal"]["key"] == plans[n]["key"] and plans[n + "_causal"]["num_splits"] == plans[n]["num_splits"]
    for key in ("w8/kg2", "w8/kg1", "w4/kg2", "w4/kg1", "w4/d256"):
        assert {r["causal"] for r in rows.values() if r["key"] == key and r["entry"] == "flash"} == {False, True}, key
    for key in ("w8/kg2", "w4/kg2", "w4/d256"):  # a forced and a planner-chosen split of a w8, a D = 64 and the D = 256 row, each causal and not
        assert {(r["splits"], r["causal"]) for r in rows.values() if r["key"] == key and r["entry"] == "split"} == {(0, False), (0, True), (3, False), (3, True)}, key
    # causal split rows with sq close to sk: a later split is EMPTY for the early tokens (whole workgroups of them), full for the late ones
    for n in ("w8_kg2_split3_deep_causal", "w4_kg2_split3_deep_causal"):
        r, pl = rows[n], plans[n]
        first = r["L"] - r["T"] + 1  # keys the first token sees
        empty = [sum(first + t <= s * pl["split_len"] for t in range(r["T"])) for s in range(pl["num_splits"])]  # tokens that see nothing of split s
        assert r["causal"] and pl["num_splits"] == 3 and empty[0] == 0 and empty[1] * (r["Hq"] // r["Hkv"]) > 2 * pl["wg_rows"] and empty[1] < empty[2] < r["T"], (n, empty)
    # ragged groups: cu_seqlens_k at D = 128 and 256 with a 1-key group, an end inside the first 32-key block and an empty later split
    for name, D in (("ragged_k_d128", 128), ("ragged_k_d256", 256)):
        r, pl = rows[name], plans[name]
        assert r["D"] == D and r["entry"] == "ragged_k" and pl["num_splits"] > 1
        assert 1 in r["klens"] and any(1 < n < 32 for n in r["klens"]) and any(32 < n < pl["split_len"] for n in r["klens"])
        assert max(r["klens"]) == r["L"] > pl["split_len"]
    r = rows["ragged_qk"]
    assert r["entry"] == "varlen" and len(set(r["qlens"])) > 2 and len(set(r["klens"])) > 2 and 1 in r["qlens"] and 1 in r["klens"]
    # the device divides by host-made magic numbers: non-powers of two in every divisor somewhere
    pow2 = lambda n: n & (n - 1) == 0  # noqa: E731
    assert not all(pow2(r["Hkv"]) for r in rows.values()) and not all(pow2(r["Hq"] // r["Hkv"]) for r in rows.values())
    assert not all(pow2(pl["num_splits"]) for pl in plans.values()) and not all(pow2(pl["row_blocks"]) for pl in plans.values())
    # no shape larger than the 256-row rule needs: units128 exceeds the chip by less than one group
    for n, r in rows.items():
        if plans[n]["wg_rows"] == 256:
            units128 = r["sb"] * r["Hkv"] * ((plans[n]["mrows"] + 127) // 128)
            assert 256 < units128 <= 256 + r["Hkv"] * ((plans[n]["mrows"] + 127) // 128) and r["nb"] == 1
    assert set(P.REPEAT_ROUTES) <= set(rows) and {rows[n]["key"] for n in P.REPEAT_ROUTES} >= keys - {"w8/kg2"}


def test_prefix_route_tells_the_workgroup_height_from_the_plan():
    # the same heads and rows at one group (52 units) and at five (260 units): only the plan's grid tells the two apart
    one = P.prefix_route(B=1, nq=265, Hq=24, Hkv=4, D=128, sb=1, kv_len=333)
    five = P.prefix_route(B=5, nq=265, Hq=24, Hkv=4, D=128, sb=5, kv_len=333)
    assert (one["wg_rows"], one["key"], five["wg_rows"], five["key"]) == (128, "w8/kg2", 256, "w8/kg1")
    assert P.prefix_route(B=5, nq=265, Hq=24, Hkv=4, D=256, sb=5, kv_len=333)["wg_rows"] == 128  # D = 256 never takes 256-row workgroups
    with pytest.raises(AssertionError):
        P.prefix_route(B=1, nq=7, Hq=6, Hkv=2, D=128, sb=1, kv_len=200)  # 21 folded rows: one row block either way
    assert not P.prefix_route(B=100, nq=1, Hq=6, Hkv=2, D=128, sb=2, kv_len=300, shared_max_workgroups=8)["persistent"]  # 8 workgroups for 8 units


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_closed_forms_agree_with_the_oracle(D, dt):
    split_len = P.lengths_split_len(D)
    assert split_len == 256 and {255, 256, 257, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129} <= set(P.listed_lengths(split_len))
    for causal in (False, True):
        c = dict(P.lengths_case("ties", D, dt, split_len), causal=causal)
        out, lse, valid, has = P.reference(c)
        cf, cl = P.ties_closed_form(c)
        lt, ct = lse.transpose(0, 2, 1), cl.transpose(0, 2, 1)
        assert has.all() != causal and (has == (P.visible_counts(c) > 0)).all()  # (causal: 40 query tokens on a group of 1 or 31 keys)
        assert np.abs(out - cf).max() <= 1e-9 and np.abs(lt[has] - ct[has]).max() <= 1e-9 and np.isneginf(lt[~has]).all() and np.isneginf(ct[~has]).all()
    c = P.lengths_case("last_key_spike", D, dt, split_len)
    out = P.reference(c)[0]
    assert np.abs(out - P.last_visible_closed_form(c)).max() <= 1e-6
    for i, n in enumerate(c["klens"]):  # a lost last key returns another row, not a 1 / L perturbation
        assert n == 1 or np.abs(c["v"][i, n - 1] - c["v"][i, n - 2]).max() > 0.5
    c = P.staircase_case(D, dt)
    out, lse, valid, has = P.reference(c)
    assert has.all() and np.abs(out - P.last_visible_closed_form(c)).max() <= 1e-6
    s = P.true_scores(c)
    assert np.abs(s).max() <= MAX_SCORE and (np.diff(s[:, :, -c["T"] - 1:], axis=2) > P.STAIRCASE_STEP - 1.0).all()


@pytest.mark.parametrize("sq,sk", [(100, 37), (300, 37), (70, 70), (40, 70)])
def test_causal_ties_count_every_rows_own_keys(sq, sk):
    """sq < sk, sq = sk and sq > sk: the leading sq - sk rows see nothing -- 0 / -inf by the oracle, which is the specification"""
    c = P.more_queries_than_keys_case(128, "bf16", sq, sk)
    c["q"] = np.zeros_like(c["q"])
    out, lse, valid, has = P.reference(c)
    cnt = P.visible_counts(c)
    assert (cnt[0] == np.clip(sk - sq + 1 + np.arange(sq), 0, sk)).all() and (has == (cnt > 0)).all() and cnt.max() < 500
    assert has.sum() == 2 * min(sq, sk) and not out[~has].any() and np.isneginf(lse.transpose(0, 2, 1)[~has]).all()
    cf, cl = P.ties_closed_form(c)
    assert np.abs(out - cf).max() <= 1e-9 and np.abs(lse.transpose(0, 2, 1)[has] - cl.transpose(0, 2, 1)[has]).max() <= 1e-9
    # one key more or fewer moves lse by 1 / n: above the lse bound (2e-3 + 1e-5 |lse|) for every count below 500
    n = cnt[has].astype(np.float64)
    assert (np.log1p(1.0 / n) > 2e-3 + 1e-5 * np.log(n + 1)).all()


# ---- the patterns put things where they say ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["w8_kg2", "w4_kg2", "w8_kg1", "w4_d256", "w4_persist", "w8_kg2_splitP"])
def test_spike_patterns_hit_the_rows_and_keys_they_name(route):
    r, pl = P.PREFIX_ROUTES[route], P.route_plan(route)
    T, Hq, Hkv, L = r["T"], r["Hq"], r["Hkv"], r["L"]
    rows = P.folded_rows(T, Hq, Hkv)
    assert sorted(rows[:, :Hq // Hkv].ravel()) == list(range(pl["mrows"]))  # a bijection onto the unit's rows, per kv head
    for pattern in ("one_query_block_spikes", "one_row_spikes"):
        c = P.route_case(route, pattern, "bf16")
        plain = ~c["anchor"][0]  # (the anchor token answers the last key as well: prefix_stress_cases.ANCHOR_LOG2)
        s = P.true_scores(c)[plain]
        js = L - 10
        carry = P.spike_carriers(pattern, T, Hq, Hkv, pl["wg_rows"])[plain]
        assert c["anchor"].sum() == len(c["klens"]) and (P.true_scores(c)[~plain][:, :, -1] > P.ANCHOR_LOG2 - 2.0).all()
        prow = rows[plain]
        assert s[carry][:, js].min() > P.SPIKE_LOG2 - 2.0 and np.abs(s[~carry]).max() < 2.0
        other = np.delete(s, js, axis=2)
        assert np.abs(other[carry]).max() < 2.0
        if pattern == "one_query_block_spikes":  # the odd 32-row blocks: in a 4-wave unit one of the two query blocks of EVERY wave
            blocks = np.unique(prow[carry] // 32)
            assert (blocks % 2 == 1).all() and len(blocks) == ((pl["mrows"] - 1) // 32 + 1) // 2
        else:  # one row per workgroup
            wgs = [b for b in range(pl["row_blocks"]) if b * pl["wg_rows"] + 37 < pl["mrows"]]  # (a last workgroup of fewer than 38 rows has none)
            assert sorted(prow[carry] // pl["wg_rows"]) == sorted(wgs * Hkv) and (prow[carry] % pl["wg_rows"] == 37).all() and wgs
        # where the spike is, MEASURED: the largest score of every carrier row -- late (the last 32-key block or the one before), in the key
        # half and the split the builder's L - 10 names, the last split of a split pass
        at = np.unique(s[carry].argmax(-1))
        assert len(at) == 1 and at[0] == js and at[0] // 32 >= (L - 1) // 32 - 1 and at[0] // pl["split_len"] == pl["num_splits"] - 1
        assert (at[0] % 128 >= 64) == {333: True, 300: False, 1100: True}[L], (L, at[0] % 128)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("route", ["w8_kg2", "w4_kg2", "w4_d256", "w8_kg1"])
def test_the_steps_straddle_the_bound(route, dt):
    """measured on the rounded inputs' true scores: the step over the largest score of the first 40 keys, row by row"""
    for pattern, lo, hi in (("step_just_under_tau", 7.7, 8.0), ("step_just_over_tau", 8.0, 8.3), ("plateau_just_under_the_bound", 7.3, 7.7)):
        c = P.route_case(route, pattern, dt)
        s = P.true_scores(c)[~c["anchor"][0]]
        step = s[:, :, 40:] - s[:, :, :40].max(2, keepdims=True)
        assert lo < step.min() and step.max() < hi, (pattern, step.min(), step.max())


@pytest.mark.parametrize("route", ["w8_kg2", "w4_kg2", "w8_kg2_split3", "w4_d256_splitP", "ragged_k_d128"])
def test_negligible_halves_and_splits_hold_no_mass(route):
    r, pl = P.PREFIX_ROUTES[route], P.route_plan(route)
    for pattern in ("key_half_negligible", "other_key_half_negligible") + (P.SPLIT_PATTERNS if pl["num_splits"] > 1 else ()):
        c = P.route_case(route, pattern, "bf16")
        for gi, n in enumerate(int(x) for x in c["klens"]):
            s = P.true_scores(c, gi)[~c["anchor"][gi]]
            j = np.arange(n)
            if pattern in P.SPLIT_PATTERNS:
                want = {"first": 0, "middle": pl["num_splits"] // 2, "last": pl["num_splits"] - 1}[pattern.rsplit("_", 1)[1]]
                low = j // pl["split_len"] != want
            else:
                low = (j % 128 >= 64) == (pattern == "key_half_negligible")
            assert (s[:, :, low] < -75.0).all() and (np.abs(s[:, :, ~low]) < 2.0).all(), (pattern, gi)
    if r["klens"]:  # split_empty: the short groups end before the second split begins
        assert sum(n <= pl["split_len"] for n in r["klens"]) >= 3 and pl["num_splits"] >= 2


@pytest.mark.parametrize("route", ROUTES)
def test_giants_sit_behind_every_length_and_nowhere_else(route):
    c = P.giants_case(route, "bf16")
    z = P.zero_behind(c)
    g = c["Hq"] // c["Hkv"]
    sc = c["D"] ** -0.5 * P.LOG2E
    nb = len(c["klens"])
    for i, n in enumerate(int(x) for x in c["klens"]):
        inside = P.true_scores(c, i)
        assert np.isfinite(inside).all() and inside.max() < 12.0
        if c["ragged"]:
            behind_k = c["k"][i + 1, :min(P.RAGGED_GIANTS, int(c["klens"][i + 1]))] if i + 1 < nb else c["tail_k"]
        else:
            behind_k = c["k"][i, n:]
            assert len(behind_k) == P.PAD_KEYS and not np.isfinite(c["v"][i, n:]).any() and not z["k"][i, n:].any() and not z["v"][i, n:].any()
        behind = np.einsum("thd,khd->thk", c["q"][i].astype(np.float64), behind_k.astype(np.float64).repeat(g, 1)) * sc
        assert np.isfinite(behind).all() and behind.min() > 80.0 and behind.max() <= MAX_SCORE
    # the reference does not look behind a length: the twin has the same result, bit for bit
    a, b = P.reference(c), P.reference(z)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if c["ragged"]:  # a giant scores exactly 0 against its own group, as the zeros of the twin do
        for i, lo, hi in c["giant_rows"]:
            assert hi > lo and not P.true_scores(c, i)[~c["anchor"][i]][:, :, lo:hi].any()
        kp, vp, cu = P.pack_keys(c)
        assert len(kp) == cu[-1] + P.RAGGED_GIANTS and np.isnan(vp[cu[-1]:]).all() and np.isfinite(vp[:cu[-1]]).all()


# ---- attainability ----------------------------------------------------------------------------------------------------------------
def _attainable(c, what):
    dt = c["dt"]
    want, wlse, valid, has = P.reference(c)
    wl = wlse.transpose(0, 2, 1)
    assert np.isfinite(want).all() and np.isfinite(wl[has]).all() and np.isneginf(wl[valid & ~has]).all() and not want[~has].any()
    model, mlse, _, _ = P.reference(c, round_p=P.ROUND[dt])
    ra, rl = err_over_bound(P.ROUND[dt](model)[has], want[has], dt)
    rs = lse_over_bound(mlse.transpose(0, 2, 1)[has], wl[has])
    print(f"model-ratio {what}: {ra:.3f} {rl:.3f} {rs:.3f}")
    assert ra <= 0.5 and rl <= 0.5 and rs <= 0.5, f"{what}: max abs at {ra:.2f} of its bound, relative L2 at {rl:.2f}, lse at {rs:.2f}"
    plain, ok = P.plain_rows_checkable(c, (want, wlse, valid, has))
    print(f"plain-rows-checkable {what}: {ok}")
    assert not ok or P.err_over_bounds(P.ROUND[dt](model)[plain], want[plain], dt) <= 0.5
    return wl[has]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("route", ROUTES)
def test_reference_rounding_model_meets_half_the_bounds(route, dt):
    for pattern in P.patterns_of(route):
        wl = _attainable(P.route_case(route, pattern, dt), f"{route} {pattern} {dt}")
        if pattern != "repeated_late_spikes":  # (standard normal data scaled by up to 40: the edge test's own construction)
            assert np.abs(wl).max() <= (MAX_SCORE + 10) * np.log(2.0)
    _attainable(P.giants_case(route, dt), f"{route} giants_behind_length {dt}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_reference_rounding_model_meets_half_the_bounds_on_the_special_shapes(D, dt):
    for pattern in ("ties", "last_key_spike"):
        for causal in ((False, True) if pattern == "ties" else (False,)):
            _attainable(dict(P.lengths_case(pattern, D, dt, 256), causal=causal), f"lengths {pattern} D={D} causal={causal} {dt}")
    _attainable(P.staircase_case(D, dt), f"staircase D={D} {dt}")
    for sq, sk in ((100, 37), (300, 37)):
        _attainable(P.more_queries_than_keys_case(D, dt, sq, sk), f"sq={sq} sk={sk} D={D} {dt}")
