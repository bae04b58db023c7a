"""Adversarial inputs for the prefix pass (csrc/prefix_unit_w64.h behind csrc/prefix_launch_w64.h), numpy only: importable without a
GPU.  The prefix pass is several bodies behind one launcher -- the 8-wave unit at D = 128 (a lane's SUM of a block's probabilities
tested against 2^8, two key halves merged through LDS), its 256-row form (every wave walks all keys, other ring layout), the
4-wave unit at D = 64 (two query blocks per wave, a maximum tree against a threshold, one cold branch for both blocks), the
one-block-per-wave unit at D = 256, and the 4-wave unit at D = 128 inside the unit loop of a persistent launch -- each causal or
not, split or unsplit, over fixed or ragged groups.  PREFIX_ROUTES has one row per body and form, `prefix_route` tells from the
library's own plan (hyd_prefix_plan) which body a shape reaches, and the builders give every key a CHOSEN score by the
construction of tests/softmax_stress_cases.py (q = unit + 0.01 noise, k = amp * unit + 0.01 noise, |score| <= 200 log2-units).

Every case is held in GROUP form: q [nb, T, Hq, D] (T query tokens per group: the queries of a sequence for flash_attention, the
sequences of a group for the decode entry), k / v [nb, Lbuf, Hkv, D], klens / qlens [nb]; `reference` is the float64 oracle per
group.  tests/test_prefix_stress.py checks the table, the closed forms, where the patterns put things and that the reference's own
rounding model meets HALF the GPU tests' bounds; tests/test_prefix_stress_gpu.py runs the cases through the kernels."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import hydragen_oracle as O
from tests.cases import _round
from tests.softmax_stress_cases import LOG2E, MAX_SCORE, _seed, per, unit_vector

ROUND = {"f16": O.round_fp16, "bf16": O.round_bf16}
# every length around the 32-key block, the 64-key half and the 128-key tile (the split boundaries are added per plan)
LISTED_LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
PAD_KEYS = 160  # keys behind the length of a fixed-group cache view: more than a 128-key tile and a 32-key block
RAGGED_GIANTS = 3  # leading keys of the NEXT ragged group that are giants to the group before it


def second_unit_vector(D: int) -> np.ndarray:
    """entries 16..31: orthogonal to unit_vector(D), the same score per unit of amplitude"""
    u = np.zeros(D, np.float32)
    u[16:32] = 1.0
    return u


def third_unit_vector(D: int) -> np.ndarray:
    u = np.zeros(D, np.float32)
    u[32:48] = 1.0
    return u


# ---- routes -----------------------------------------------------------------------------------------------------------------
def _route(entry, sb, T, Hq, Hkv, D, L, key, rule, *, nb=None, causal=False, splits=1, klens=None, qlens=None, wgs=0):
    """entry: "flash" (flash_attention: one sequence of T queries per group), "split" (flash.prefix_attention with num_splits =
    `splits`, 0 = the planner's; BQH LSE layout), "ragged_k" (prefix_attention with cu_seqlens_k: T sequences of one query per
    group), "varlen" (flash_attention_varlen: packed queries, ragged both ways), "decode" (the decode entry, empty unique cache,
    one shared level, `wgs` persistent workgroups).  sb groups repeat a built block of nb (default: all distinct)."""
    return dict(entry=entry, sb=sb, T=T, Hq=Hq, Hkv=Hkv, D=D, L=L, key=key, rule=rule, nb=nb or sb, causal=causal, splits=splits,
                klens=klens, qlens=qlens, wgs=wgs)


# 2 groups x 2 kv heads x 70 tokens x g = 3: 210 folded rows = one full 128-row workgroup and one of 82 rows (two full 32-row
# waves and one of 18 lanes; at D = 64 one full 64-row wave and one whose first query block has 18 lanes and whose second is empty)
_SMALL = dict(sb=2, T=70, Hq=6, Hkv=2)
# 5 groups (one built, repeated) x 4 kv heads x 265 tokens x g = 6: 1590 folded rows = 13 blocks of 128 -> 260 units > 256 CUs, so 7
# blocks of 256, the last with 54 rows (one full 32-row wave, one of 22 lanes)
_TALL = dict(sb=5, nb=1, T=265, Hq=24, Hkv=4)
_RAGGED_LENS = (1, 20, 300, 45, 700)  # one key; an end inside the first 32-key block; shorter than split_len (384): empty split

PREFIX_ROUTES = {
    "w8_kg2": _route("flash", D=128, L=333, key="w8/kg2", rule="D = 128, units128 = 8 <= kNumCU: 128-row workgroups of 8 waves, two key halves", **_SMALL),
    "w8_kg1": _route("flash", D=128, L=333, key="w8/kg1", rule="D = 128, units128 = 260 > kNumCU: 256-row workgroups, every wave walks all keys", **_TALL),
    "w4_kg2": _route("flash", D=64, L=333, key="w4/kg2", rule="D = 64: the 4-wave unit, two query blocks per wave, two key halves", **_SMALL),
    "w4_kg1": _route("flash", D=64, L=333, key="w4/kg1", rule="D = 64, units128 = 260 > kNumCU: 256-row workgroups, KG = 1", **_TALL),
    "w4_d256": _route("flash", D=256, L=333, key="w4/d256", rule="D = 256: one query block per wave, 128-row workgroups, KG = 1 only", **_SMALL),
    "w8_kg2_split3": _route("split", D=128, L=700, splits=3, key="w8/kg2", rule="num_splits = 3 forced: split_len 256, fp32 slices + combine.hip", **_SMALL),
    "w8_kg2_splitP": _route("split", D=128, L=1100, splits=0, key="w8/kg2", rule="plan_prefix splits 8 units x 1100 keys by its cost model", **_SMALL),
    "w4_kg2_split3": _route("split", D=64, L=700, splits=3, key="w4/kg2", rule="D = 64, num_splits = 3 forced", **_SMALL),
    "w4_kg2_splitP": _route("split", D=64, L=1100, splits=0, key="w4/kg2", rule="D = 64, the planner's split", **_SMALL),
    "w4_d256_split3": _route("split", D=256, L=700, splits=3, key="w4/d256", rule="D = 256, num_splits = 3 forced", **_SMALL),
    "w4_d256_splitP": _route("split", D=256, L=1100, splits=0, key="w4/d256", rule="D = 256, the planner's split", **_SMALL),
    "ragged_k_d128": _route("ragged_k", sb=5, T=70, Hq=6, Hkv=3, D=128, L=700, splits=0, klens=_RAGGED_LENS, key="w8/kg2",
                            rule="cu_seqlens_k, planner split: the groups of 1 / 20 / 45 / 300 keys leave the second split empty"),
    "ragged_k_d256": _route("ragged_k", sb=5, T=70, Hq=6, Hkv=3, D=256, L=700, splits=0, klens=_RAGGED_LENS, key="w4/d256",
                            rule="cu_seqlens_k at D = 256, planner split, empty second splits"),
    "ragged_qk": _route("varlen", sb=4, T=70, Hq=6, Hkv=2, D=128, L=333, klens=(1, 20, 333, 45), qlens=(3, 70, 1, 40), key="w8/kg2",
                        rule="cu_seqlens_q + cu_seqlens_k (packed queries): one split, row blocks by max_q_len"),
    "w4_persist": _route("decode", sb=2, T=50, Hq=6, Hkv=2, D=128, L=300, wgs=3, key="w4/persist",
                         rule="decode entry, shared_max_workgroups = 3 < 8 units: the 4-wave unit in the unit loop (3, 3 and 2 units)"),
    "w4_persist_d64": _route("decode", sb=2, T=50, Hq=6, Hkv=2, D=64, L=300, wgs=3, key="w4/kg2+persist",
                             rule="decode entry at D = 64, 3 workgroups for 8 units: the same 4-wave arithmetic as the one-unit launch"),
}
# 600 query tokens on 700 keys in 3 forced splits of 256: causal token i sees 101 + i keys, so the second split is empty for the first 155
# tokens and the third for the first 411 -- whole workgroups write 0 / -inf slices that combine.hip merges with real ones
_DEEP = dict(sb=2, T=600, Hq=6, Hkv=2)
PREFIX_ROUTES["w8_kg2_split3_deep"] = _route("split", D=128, L=700, splits=3, key="w8/kg2", rule="num_splits = 3 forced, sq close to sk (for its causal twin)", **_DEEP)
PREFIX_ROUTES["w4_kg2_split3_deep"] = _route("split", D=64, L=700, splits=3, key="w4/kg2", rule="D = 64, num_splits = 3 forced, sq close to sk (for its causal twin)", **_DEEP)
# a causal variant of every non-persistent row but the cu_seqlens_k ones (uniform queries of several sequences per group: the kernel's
# causal limit exists for one sequence per group only, `CAUSAL && a.per == 1`)
for _name in [n for n, r in PREFIX_ROUTES.items() if r["entry"] in ("flash", "split", "varlen")]:
    PREFIX_ROUTES[_name + "_causal"] = dict(PREFIX_ROUTES[_name], causal=True, rule=PREFIX_ROUTES[_name]["rule"] + "; causal")
SPLIT_ROUTES = tuple(n for n, r in PREFIX_ROUTES.items() if r["splits"] != 1)
REPEAT_ROUTES = ("w4_kg2", "w4_kg2_causal", "w4_d256", "w4_d256_splitP", "w8_kg1", "w4_kg1", "w4_kg1_causal", "w4_persist", "w4_persist_d64", "ragged_k_d256",
                 "w4_kg2_split3_deep_causal")


def plan_args(route: str) -> dict:
    """the hyd_prefix_params shape fields of a PREFIX_ROUTES row as its entry point marshals them"""
    r = PREFIX_ROUTES[route]
    kw = dict(Hq=r["Hq"], Hkv=r["Hkv"], D=r["D"], sb=r["sb"], kv_len=r["L"], causal=r["causal"], num_splits=r["splits"] if r["entry"] in ("split", "ragged_k") else 0)
    if r["entry"] in ("flash", "split"):
        return dict(kw, B=r["sb"], nq=r["T"])
    if r["entry"] == "varlen":
        return dict(kw, B=sum(r["qlens"]), nq=1, max_q_len=max(r["qlens"]))
    return dict(kw, B=r["sb"] * r["T"], nq=1, shared_max_workgroups=r["wgs"])


@functools.lru_cache(maxsize=None)
def _plan(B, nq, Hq, Hkv, D, sb, kv_len, causal, num_splits, max_q_len):
    from hydragen_amd import _lib

    p = _lib.PrefixParams()
    p.dtype = _lib.HYD_BF16
    p.B, p.nq, p.Hq, p.Hkv, p.D, p.sb, p.kv_len, p.causal, p.num_splits, p.max_q_len = B, nq, Hq, Hkv, D, sb, kv_len, int(causal), num_splits, max_q_len
    p.k_tok_stride = p.v_tok_stride = Hkv * D
    p.k_head_stride = p.v_head_stride = D
    dummy = (C.c_int32 * 2)(0, 0)  # the plan asks only WHETHER the queries are packed
    if max_q_len:
        p.cu_seqlens_q = C.cast(dummy, C.c_void_p)
    ns, grid, sl = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    _lib.check(_lib.load().hyd_prefix_plan(C.byref(p), C.byref(ns), C.byref(grid), C.byref(sl)))
    return ns.value, grid.value, sl.value


def prefix_route(B, nq, Hq, Hkv, D, sb, kv_len, causal=False, num_splits=0, max_q_len=0, shared_max_workgroups=0) -> dict:
    """The body a prefix pass of these shapes runs, read off the library's own plan (hyd_prefix_plan answers without a device):
    row_blocks = grid / (sb * Hkv * num_splits) tells 128- from 256-row workgroups (the folded rows must make the two differ), the
    launch is persistent iff 0 < shared_max_workgroups < grid, and 8 waves run iff D = 128 and the launch is not persistent."""
    ns, grid, split_len = _plan(B, nq, Hq, Hkv, D, sb, kv_len, bool(causal), num_splits, max_q_len)
    assert grid % (sb * Hkv * ns) == 0, (grid, sb, Hkv, ns)
    row_blocks = grid // (sb * Hkv * ns)
    mrows = (max_q_len if max_q_len else B // sb * nq) * (Hq // Hkv)
    rb128, rb256 = (mrows + 127) // 128, (mrows + 255) // 256
    assert rb128 != rb256 and row_blocks in (rb128, rb256), f"{mrows} folded rows do not tell the workgroup height ({row_blocks} row blocks)"
    wg_rows = 128 if row_blocks == rb128 else 256
    persistent = 0 < shared_max_workgroups < grid
    waves = 8 if D == 128 and not persistent else 4
    kg = 1 if D == 256 or wg_rows == 256 else 2
    key = "w4/d256" if D == 256 else "w4/persist" if persistent and D == 128 else f"w{waves}/kg{kg}"
    if persistent and D != 128:
        key += "+persist"
    return dict(key=key, num_splits=ns, split_len=split_len, grid=grid, row_blocks=row_blocks, wg_rows=wg_rows, mrows=mrows,
                persistent=persistent, waves=waves, kg=kg)


def lengths_split_len(D: int) -> int:
    """split_len of the length list's ragged launch (lengths_case) with LENGTHS_SPLITS forced splits, from the library's plan"""
    nb = len(LISTED_LENS) + 4
    ns, _, split_len = _plan(nb * LENGTHS_SHAPE["T"], 1, LENGTHS_SHAPE["Hq"], LENGTHS_SHAPE["Hkv"], D, nb, LENGTHS_KVLEN, False, LENGTHS_SPLITS, 0)
    assert ns == LENGTHS_SPLITS
    return split_len


def route_plan(route: str) -> dict:
    return prefix_route(**plan_args(route))


# ---- score patterns ---------------------------------------------------------------------------------------------------------
SUM_TESTED_KINDS = ("all_far_below_zero", "ramp_per_block", "ramp_per_key", "plateau_just_under_the_bound", "late_spike_after_plateau")
SCORE_PATTERNS = SUM_TESTED_KINDS + ("repeated_late_spikes", "step_just_under_tau", "step_just_over_tau", "one_query_block_spikes",
                                     "one_row_spikes", "key_half_negligible", "other_key_half_negligible", "last_key_spike", "ties")
# (`ties` pins a key count through lse = ln(n) only while 1 / n exceeds the lse bound, n < 500: on the rows of 700 and 1100 keys it
# cannot see a limit off by one key -- the length list (lengths_case) and the causal rows, whose tokens see fewer keys, do that)
SPLIT_PATTERNS = ("split_negligible_first", "split_negligible_middle", "split_negligible_last")
LAST_KEY_LOG2 = 40.0  # last_key_spike: 1100 older keys leak 2^-40 each, the closed form holds to 1e-6
SPIKE_LOG2 = 40.0  # the late giant of the *_spikes patterns, log2-units above the plateau at 0


def sum_tested_amplitudes(kind: str, sk: int, p: float, rng, max_score: float | None = None) -> np.ndarray:
    """amp [sk] (float32 where the formula is): key j scores amp[j] * p log2-units.  The five kinds of
    tests/test_edge_gpu.py::test_prefix_sum_tested_softmax_on_adversarial_scores, chosen against the 8-wave unit's sum test (LAZY):
    every score far below zero; maxima that climb by less than 2^8 per block / per key; a plateau just under the bound from key 40
    on; a spike 23 keys before the end behind that plateau.  max_score caps the ramps' end (the edge test's own shape is uncapped)."""
    j = np.arange(sk, dtype=np.float32)
    if kind == "all_far_below_zero":
        return np.full(sk, -60.0 / p) + rng.standard_normal(sk).astype(np.float32) * 0.5
    if kind == "ramp_per_block":
        step = 6.0 if max_score is None else min(6.0, max_score / max((sk - 1) // 32, 1))
        return (step * (j // 32)) / p
    if kind == "ramp_per_key":
        step = 0.35 if max_score is None else min(0.35, max_score / max(sk - 1, 1))
        return (step * j) / p
    if kind == "plateau_just_under_the_bound":
        return np.where(j < 40, 0.0, 7.5) / p
    if kind == "late_spike_after_plateau":
        amp = np.where(j < 40, 0.0, 7.5) / p
        amp[max(sk - 23, 0)] = 30.0 / p
        return amp
    raise KeyError(kind)


def sum_tested_case(kind: str, dt: str, shape=(1, 160, 1000, 4, 2, 128)) -> dict:
    """The inputs of test_prefix_sum_tested_softmax_on_adversarial_scores, array for array: seed by kind, q = unit + noise, amp, k
    noise, v, in that order of draws."""
    rng = np.random.default_rng(SUM_TESTED_KINDS.index(kind) + 1)
    b, sq, sk, hq, hkv, D = shape
    unit = np.zeros(D, np.float32)
    unit[:16] = 1.0
    p = 16 * D ** -0.5 * 1.4426950408889634
    q = np.broadcast_to(unit, (b, sq, hq, D)).copy() + 0.01 * rng.standard_normal((b, sq, hq, D)).astype(np.float32)
    amp = sum_tested_amplitudes(kind, sk, p, rng)
    k = (amp[:, None] * unit[None, :])[None, :, None, :].repeat(hkv, 2).astype(np.float32)
    k = k + 0.01 * rng.standard_normal(k.shape).astype(np.float32)
    q, k = _round(q, dt), _round(k, dt)
    v = _round(rng.standard_normal((b, sk, hkv, D), dtype=np.float32), dt)
    return dict(q=q, k=k, v=v)


REPEATED_SPIKES = ((0.070, 5.0), (0.333, 9.0), (0.334, 14.0), (0.640, 20.0), (0.959, 28.0), (0.999, 40.0))  # (position / sk, key factor)


def repeated_spike_positions(sk: int) -> list:
    """(key, factor): keys scaled far above every other score at several block positions, twice in a row; 70, 333, 334, 640, 959
    and 999 of 1000 keys"""
    return [(min(int(round(f * sk)), sk - 1), x) for f, x in REPEATED_SPIKES]


def repeated_late_spikes_case(dt: str, shape=(1, 160, 1000, 4, 2, 128), seed=23) -> dict:
    """The inputs of test_prefix_deferred_rescale_is_exact: standard normal q / k / v, six keys scaled by 5 .. 40 late in the
    sequence, and every row of head 0 aligned with the fifth of them (raw q . k far above every other score)."""
    rng = np.random.default_rng(seed)
    b, sq, sk, hq, hkv, D = shape
    rnd = lambda s: _round(rng.standard_normal(s, dtype=np.float32), dt)  # noqa: E731
    q = rnd((b, sq, hq, D))
    k, v = rnd((b, sk, hkv, D)), rnd((b, sk, hkv, D))
    spots = repeated_spike_positions(sk)
    for pos, f in {pos: f for pos, f in spots}.items():  # (a group shorter than the six positions: the last factor of a key counts)
        k[:, pos] = _round(k[:, pos] * f, dt)
    q[:, :, 0] = _round(np.abs(q[:, :, 0]) * np.sign(k[:, spots[4][0], 0])[:, None, :], dt)
    return dict(q=q, k=k, v=v)


def folded_rows(T: int, Hq: int, Hkv: int) -> np.ndarray:
    """[T, Hq]: the row of its (group, kv head) unit that query token t, head h is (prefix_unit_w64.h row_of: token * g + h % g)"""
    g = Hq // Hkv
    return np.arange(T)[:, None] * g + (np.arange(Hq) % g)[None, :]


def spike_carriers(pattern: str, T: int, Hq: int, Hkv: int, wg_rows: int) -> np.ndarray:
    """[T, Hq] bool: the rows that carry the second unit vector -- the odd 32-row blocks (in the 4-wave unit one of a wave's two
    query blocks), or row 37 of every workgroup (in wave 1 of an 8-wave unit, in the second block of wave 0 of a 4-wave one)."""
    r = folded_rows(T, Hq, Hkv)
    return (r // 32) % 2 == 1 if pattern == "one_query_block_spikes" else r % wg_rows == 37


def amplitudes(pattern: str, L: int, D: int, rng, split_len: int = 0, nsplit: int = 1):
    """(amp [L], amp2 [L]) in units of amplitude along the first / the second unit vector"""
    p = per(D)
    j = np.arange(L)
    amp, amp2 = np.zeros(L), np.zeros(L)
    if pattern in SUM_TESTED_KINDS:
        amp = np.asarray(sum_tested_amplitudes(pattern, L, p, rng, max_score=RAMP_MAX), np.float64)
    elif pattern in ("step_just_under_tau", "step_just_over_tau"):  # the threshold body and the sum body decide differently around 2^8
        amp = np.where(j < 40, 0.0, 7.9 if pattern == "step_just_under_tau" else 8.1) / p
    elif pattern in ("one_query_block_spikes", "one_row_spikes"):
        amp2[max(L - 10, 0)] = SPIKE_LOG2 / p
    elif pattern in ("key_half_negligible", "other_key_half_negligible"):  # one key half's (m, l, O) is negligible in the LDS merge
        amp = np.where((j % 128 >= 64) == (pattern == "key_half_negligible"), -80.0, 0.0) / p
    elif pattern in SPLIT_PATTERNS:
        s = {"first": 0, "middle": nsplit // 2, "last": nsplit - 1}[pattern.rsplit("_", 1)[1]]
        amp = np.where(j // max(split_len, 1) == s, 0.0, -80.0) / p
    elif pattern == "last_key_spike":
        amp[L - 1] = LAST_KEY_LOG2 / p
    elif pattern in ("ties", "giants_behind_length"):
        if pattern == "giants_behind_length":
            amp = np.where(j < 40, 0.0, 7.5) / p
            amp[L - 1] = 10.0 / p
    else:
        raise KeyError(pattern)
    assert max(np.abs(amp).max(), np.abs(amp2).max()) * p <= MAX_SCORE + 2.0, pattern
    return amp, amp2


# Every v row of a (group, kv head) shares a part of +-V_COMMON per column beside its standard normal one.  On a zero-mean result
# (a flat score pattern over N keys: elements of about N^-0.5) the bf16 rounding of the OUTPUT alone is 0.42 of the relative-L2
# bound (half an ulp of 2^-8 against 4e-3), and the rounding of the probabilities, which does not average out over keys with
# independent v rows, as much again: no kernel could stay within half the bound.  Against the common part the probabilities' rounding
# errors do average out (relative error N^-0.5 times smaller), while a wrong weight still moves the result by its standard normal part.
V_COMMON = 0.25
# The bf16 bound on |out - want| is 2^-7 of the LARGEST expected element, and rounding that element to bf16 alone can cost half of it
# (half an ulp is up to 2^-8 of a value): where the largest element is an inexact one, no kernel could promise half the bound.  So
# one query token per group, the last, is an ANCHOR: it carries a third unit vector (entries 32..47) that only the group's last key
# answers, ANCHOR_LOG2 above every other score, and returns that key's v row -- exact in the dtype and, a raw standard normal row,
# larger than every averaged element (the 1-key sequences do the same for the suffix cases of tests/softmax_stress_cases.py).
# THE COST: gpu_util.assert_close_l2 scales its max-abs bound by the largest expected element of the whole tensor, so beside an anchor row
# of elements up to about 4 the absolute bound on the averaged rows (elements of 0.25 to 0.3) is about tenfold looser, and on them only the
# relative L2 check and the lse check bite.  `plain_rows_checkable` says where the averaged rows ALONE also meet the half-bound condition;
# there the GPU tests hold them to the bounds a second time, without the anchor rows.
ANCHOR_LOG2 = 40.0
UNANCHORED = ("ties", "last_key_spike")  # q = 0; an exact result in every row
GIANTS_ANCHOR_LOG2, GIANTS_OTHERS_LOG2 = 11.5, -60.0  # giants_behind_length keeps every score inside below 12: its anchor token carries the
# third unit vector ALONE and sees the last key at 11.5 and, through a part of every other key that no other row sees, the rest at -60
RAMP_MAX = MAX_SCORE - 10.0 - ANCHOR_LOG2  # where a route's ramps end at the latest: the anchor stays within MAX_SCORE


def _group_lens(r):
    nb = r["nb"]
    klens = np.asarray(r["klens"] if r["klens"] else [r["L"]] * nb, np.int32)
    qlens = np.asarray(r["qlens"] if r["qlens"] else [r["T"]] * nb, np.int32)
    return klens, qlens


def build_case(pattern: str, dt: str, *, nb, T, Hq, Hkv, D, klens, qlens=None, causal=False, wg_rows=128, split_len=0, nsplit=1, seed=0,
               anchor=True) -> dict:
    """One block of groups in group form; k / v [nb, max klen, Hkv, D] are zero behind a group's length."""
    rng = np.random.default_rng(seed)
    klens = np.asarray(klens, np.int32)
    qlens = np.full(nb, T, np.int32) if qlens is None else np.asarray(qlens, np.int32)
    Lmax = int(klens.max())
    if pattern == "repeated_late_spikes":  # standard normal data, per group at its own length
        q, k, v = (np.zeros(s, np.float32) for s in ((nb, T, Hq, D), (nb, Lmax, Hkv, D), (nb, Lmax, Hkv, D)))
        for i, n in enumerate(int(x) for x in klens):
            c = repeated_late_spikes_case(dt, (1, T, n, Hq, Hkv, D), seed=seed + i)
            q[i], k[i, :n], v[i, :n] = c["q"][0], c["k"][0], c["v"][0]
        return dict(q=q, k=k, v=v, klens=klens, qlens=qlens, causal=causal, pattern=pattern, dt=dt, Hq=Hq, Hkv=Hkv, D=D, T=T,
                    anchor=np.zeros((nb, T), bool))
    unit, u2 = unit_vector(D), second_unit_vector(D)
    noise = lambda *s: 0.01 * rng.standard_normal(s, dtype=np.float32)  # noqa: E731
    q = np.broadcast_to(unit, (nb, T, Hq, D)) + noise(nb, T, Hq, D)
    q = np.ascontiguousarray(q)
    if pattern in ("one_query_block_spikes", "one_row_spikes"):
        q = q + spike_carriers(pattern, T, Hq, Hkv, wg_rows)[None, :, :, None] * u2
    anchored = anchor and pattern not in UNANCHORED
    u3 = third_unit_vector(D)
    if anchored:
        q[..., u3 > 0] = 0.0  # every other row is exactly blind to the anchor's part of the last key
    k = np.zeros((nb, Lmax, Hkv, D), np.float32)
    for i, n in enumerate(int(x) for x in klens):
        amp, amp2 = amplitudes(pattern, n, D, rng, split_len, nsplit)
        amp3 = np.zeros(n)
        if anchored and pattern == "giants_behind_length":
            amp3[:] = GIANTS_OTHERS_LOG2 / per(D)
            amp3[n - 1] = GIANTS_ANCHOR_LOG2 / per(D)
            q[i, int(qlens[i]) - 1] = u3
        elif anchored:  # the group's last query token carries the third unit vector, its last key ANCHOR_LOG2 above every other score
            amp3[n - 1] = amp.max() - amp[n - 1] + ANCHOR_LOG2 / per(D)
            q[i, int(qlens[i]) - 1] = q[i, int(qlens[i]) - 1] + u3
        k[i, :n] = ((amp[:, None] * unit + amp2[:, None] * u2 + amp3[:, None] * u3).astype(np.float32)[:, None, :].repeat(Hkv, 1) + noise(n, Hkv, D))
    if pattern == "ties":
        q = np.zeros_like(q)
    v = rng.standard_normal((nb, Lmax, Hkv, D), dtype=np.float32) + V_COMMON * np.where(rng.random((nb, 1, Hkv, D)) < 0.5, -1.0, 1.0).astype(np.float32)
    for i, n in enumerate(int(x) for x in klens):
        v[i, n:] = 0.0
    anchor = np.zeros((nb, T), bool)
    anchor[np.arange(nb), qlens - 1] = anchored
    return dict(q=_round(q, dt), k=_round(k, dt), v=_round(v, dt), klens=klens, qlens=qlens, causal=causal, pattern=pattern, dt=dt,
                Hq=Hq, Hkv=Hkv, D=D, T=T, anchor=anchor)


def route_case(route: str, pattern: str, dt: str) -> dict:
    """A PREFIX_ROUTES row's built block under a score pattern.  The causal variant of a route holds the same data."""
    r = PREFIX_ROUTES[route]
    pl = route_plan(route)
    klens, qlens = _group_lens(r)
    base = route[:-7] if route.endswith("_causal") else route
    return build_case(pattern, dt, nb=r["nb"], T=r["T"], Hq=r["Hq"], Hkv=r["Hkv"], D=r["D"], klens=klens, qlens=qlens, causal=r["causal"],
                      wg_rows=pl["wg_rows"], split_len=pl["split_len"], nsplit=pl["num_splits"], seed=_seed("prefix", base, pattern))


def patterns_of(route: str) -> tuple:
    """the score patterns that apply to a route: all of them, and the mass-in-one-split ones where the pass is split"""
    return SCORE_PATTERNS + (SPLIT_PATTERNS if route_plan(route)["num_splits"] > 1 else ())


def reference(c: dict, round_p=None):
    """float64 oracle per group: out [nb, T, Hq, D], lse [nb, Hq, T], and two masks [nb, T]: `valid` (a query token of the group)
    and `has` (valid and at least one visible key).  Rows without a visible key are 0 / -inf: the oracle is the specification."""
    q, k, v = c["q"], c["k"], c["v"]
    nb, T, Hq, D = q.shape
    out, lse = np.zeros((nb, T, Hq, D)), np.full((nb, Hq, T), -np.inf)
    valid, has = np.zeros((nb, T), bool), np.zeros((nb, T), bool)
    for i in range(nb):
        nq, nk = int(c["qlens"][i]), int(c["klens"][i])
        valid[i, :nq] = True
        if nq == 0:
            continue
        o, l = O.attention_lse(q[i:i + 1, :nq], k[i:i + 1, :nk], v[i:i + 1, :nk], causal=c["causal"], round_p=round_p)
        out[i, :nq], lse[i, :, :nq] = o[0], l[0]
        has[i, :nq] = np.isfinite(l[0]).all(0)
    return out, lse, valid, has


def err_over_bounds(got, want, dt) -> float:
    """the larger of (max abs error / its bound, relative L2 / its bound), bounds of gpu_util.assert_close_l2"""
    from tests.gpu_util import ATOL, REL_L2, atol

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not got.size:
        return 0.0
    bound = ATOL["f16"] * max(1.0, float(np.abs(want).max())) if dt == "f16" else atol(dt, want)
    return max(np.abs(got - want).max() / bound, np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30) / REL_L2[dt])


def plain_rows_checkable(c: dict, ref=None):
    """(mask [nb, T] of the rows with a visible key that are no anchor, whether the reference's rounding model stays within half the `out`
    bounds on THOSE rows alone): decided by the oracle's model, never by a kernel's result"""
    want, _, valid, has = ref if ref is not None else reference(c)
    plain = has & ~c["anchor"]
    if not c["anchor"].any() or not plain.any():
        return plain, False
    model = ROUND[c["dt"]](reference(c, round_p=ROUND[c["dt"]])[0])
    return plain, err_over_bounds(model[plain], want[plain], c["dt"]) <= 0.5


def visible_counts(c: dict) -> np.ndarray:
    """[nb, T]: keys a query token sees (bottom-right aligned causal mask: token i of nq sees the first klen - nq + i + 1)"""
    nb, T = c["q"].shape[:2]
    n = np.zeros((nb, T), np.int64)
    for i in range(nb):
        nq, nk = int(c["qlens"][i]), int(c["klens"][i])
        n[i, :nq] = np.clip(nk - nq + np.arange(nq) + 1, 0, nk) if c["causal"] else nk
    return n


def ties_closed_form(c: dict):
    """q = 0: out = the mean of the visible v rows, lse = ln(count); 0 / -inf without a visible key"""
    nb, T, Hq, D = c["q"].shape
    g = Hq // c["Hkv"]
    cnt = visible_counts(c)
    out, lse = np.zeros((nb, T, Hq, D)), np.full((nb, Hq, T), -np.inf)
    for i in range(nb):
        cs = np.cumsum(c["v"][i].astype(np.float64), 0)  # [L, Hkv, D]
        for t in range(T):
            n = int(cnt[i, t])
            if n:
                out[i, t] = np.repeat(cs[n - 1] / n, g, axis=0)
                lse[i, :, t] = np.log(n)
    return out, lse


def last_visible_closed_form(c: dict) -> np.ndarray:
    """last_key_spike (non-causal) and the staircase: every row returns the v row of its LAST visible key"""
    nb, T, Hq, D = c["q"].shape
    g = Hq // c["Hkv"]
    cnt = visible_counts(c)
    out = np.zeros((nb, T, Hq, D))
    for i in range(nb):
        for t in range(T):
            if cnt[i, t]:
                out[i, t] = np.repeat(c["v"][i, int(cnt[i, t]) - 1].astype(np.float64), g, axis=0)
    return out


def true_scores(c: dict, group: int = 0) -> np.ndarray:
    """[T, Hq, klen] log2-units, from the rounded inputs"""
    g = c["Hq"] // c["Hkv"]
    n = int(c["klens"][group])
    return np.einsum("thd,khd->thk", c["q"][group].astype(np.float64), c["k"][group, :n].astype(np.float64).repeat(g, 1)) * c["D"] ** -0.5 * LOG2E


# ---- the length list and the staircase ----------------------------------------------------------------------------------------
LENGTHS_SHAPE = dict(T=40, Hq=6, Hkv=2)  # 120 folded rows: one workgroup, its last wave (or query block) with 24 lanes
LENGTHS_KVLEN, LENGTHS_SPLITS = 700, 3  # the ragged launch's longest group and forced split count: split_len = 256


def listed_lengths(split_len: int) -> tuple:
    return tuple(dict.fromkeys(LISTED_LENS + (split_len - 1, split_len, split_len + 1)))


def lengths_case(pattern: str, D: int, dt: str, split_len: int) -> dict:
    """One group per listed length and one of LENGTHS_KVLEN keys (it fixes the ragged launch's kv_len, hence split_len): run as ONE
    cu_seqlens_k launch, unsplit and with LENGTHS_SPLITS splits (the groups of split_len - 1 and split_len keys leave the later
    splits empty, the one of split_len + 1 leaves one key in the second), and group by group as fixed-length launches."""
    lens = listed_lengths(split_len) + (LENGTHS_KVLEN,)
    return build_case(pattern, dt, nb=len(lens), D=D, klens=lens, seed=_seed("prefix lengths", pattern, D), **LENGTHS_SHAPE)


# log2-units: the first step over the L - sq flat keys (200 of them leak 2^-30 each) and every further step (the key before leaks
# 2^-24), so that the closed form holds to 1e-6; the ramp ends at 174
STAIRCASE_BASE, STAIRCASE_STEP = 30.0, 24.0


def staircase_case(D: int, dt: str, sq: int = 7, L: int = 200, Hq: int = 6, Hkv: int = 2, nb: int = 2) -> dict:
    """causal_last_rows_staircase: sq rows over L keys (the shape of tests/test_primitives_gpu.py), the last sq keys a ramp of
    STAIRCASE_BASE + i * STAIRCASE_STEP log2-units: causal row i returns v[L - sq + i].  An off-by-one limit returns a neighbouring row."""
    rng = np.random.default_rng(_seed("staircase", D))
    p = per(D)
    unit = unit_vector(D)
    amp = np.zeros(L)
    amp[L - sq:] = (STAIRCASE_BASE + STAIRCASE_STEP * np.arange(sq)) / p
    assert amp.max() * p <= MAX_SCORE
    q = np.broadcast_to(unit, (nb, sq, Hq, D)) + 0.01 * rng.standard_normal((nb, sq, Hq, D), dtype=np.float32)
    k = (amp[None, :, None, None] * unit).astype(np.float32).repeat(nb, 0).repeat(Hkv, 2) + 0.01 * rng.standard_normal((nb, L, Hkv, D), dtype=np.float32)
    v = rng.standard_normal((nb, L, Hkv, D), dtype=np.float32)
    return dict(q=_round(q, dt), k=_round(k, dt), v=_round(v, dt), klens=np.full(nb, L, np.int32), qlens=np.full(nb, sq, np.int32), causal=True,
                pattern="causal_last_rows_staircase", dt=dt, Hq=Hq, Hkv=Hkv, D=D, T=sq, anchor=np.zeros((nb, sq), bool))


def more_queries_than_keys_case(D: int, dt: str, sq: int, sk: int, Hq: int = 6, Hkv: int = 2, nb: int = 2) -> dict:
    """causal with sq > sk: the leading sq - sk rows see no key at all"""
    c = build_case("plateau_just_under_the_bound", dt, nb=nb, T=sq, Hq=Hq, Hkv=Hkv, D=D, klens=[sk] * nb, causal=True,
                   seed=_seed("sq > sk", D, sq, sk), anchor=False)
    rng = np.random.default_rng(_seed("sq > sk q", D, sq, sk))
    c["q"] = _round(rng.standard_normal(c["q"].shape, dtype=np.float32), dt)  # rows differ: standard normal queries
    return c


# ---- finite giants behind the length ------------------------------------------------------------------------------------------
def giants_case(route: str, dt: str) -> dict:
    """giants_behind_length.  Fixed groups: k / v are PAD_KEYS longer than the length the kernel is told ([:, :L] views of them are
    handed over); behind it K holds finite giants (90 log2-units against every query), V NaN and Inf.  Ragged groups are packed
    without a gap, so the giants are the NEXT group's first RAGGED_GIANTS keys (and RAGGED_GIANTS pad rows behind the last group):
    groups alternate between the two unit vectors, a group's queries are exactly zero on the other vector's entries and the giants
    exactly zero off them, so a giant scores 90 against the group before it and exactly 0 against its own.  The anchor tokens
    (GIANTS_ANCHOR_LOG2) alternate likewise between entries 32..47 and 48..63: a giant scores 90 against the anchor token of the group
    before it and -60, like every key but the last, against its own group's.  `zero_behind` is the twin."""
    r = PREFIX_ROUTES[route]
    base = route[:-7] if route.endswith("_causal") else route
    klens, qlens = _group_lens(r)
    nb, T, Hq, Hkv, D = r["nb"], r["T"], r["Hq"], r["Hkv"], r["D"]
    c = build_case("giants_behind_length", dt, nb=nb, T=T, Hq=Hq, Hkv=Hkv, D=D, klens=klens, qlens=qlens, causal=r["causal"],
                   seed=_seed("prefix giants", base))
    rng = np.random.default_rng(_seed("prefix giants behind", base))
    p = per(D)
    units = (unit_vector(D), second_unit_vector(D))
    ragged = r["klens"] is not None
    c["ragged"] = ragged
    if not ragged:
        L = int(klens[0])
        kb = (np.full((nb, PAD_KEYS, 1, 1), 90.0 / p) * (units[0] + third_unit_vector(D))).astype(np.float32).repeat(Hkv, 2) + 0.01 * rng.standard_normal((nb, PAD_KEYS, Hkv, D), dtype=np.float32)
        vb = np.where(np.arange(PAD_KEYS)[None, :, None, None] % 2 == 0, np.nan, np.inf) * np.ones((nb, 1, Hkv, D))
        c["k"] = np.concatenate([c["k"][:, :L], _round(kb, dt)], 1)
        c["v"] = np.concatenate([c["v"][:, :L], vb.astype(np.float32)], 1)
        c["giant_rows"] = [(i, L, L + PAD_KEYS) for i in range(nb)]
        return c
    # ragged: group i lives on unit vector i % 2; its first keys are giants along unit vector (i - 1) % 2
    G = RAGGED_GIANTS
    u4 = np.zeros(D, np.float32)
    u4[48:64] = 1.0
    anchors = (third_unit_vector(D), u4)
    c["own"] = [_round(np.float32(GIANTS_OTHERS_LOG2 / p) * anchors[i % 2], dt) for i in range(nb)]  # what group i's anchor token sees of a giant
    q, k = c["q"].copy(), c["k"].copy()
    for i in range(nb):
        if i % 2:  # move the group to the second unit vector and its anchor to entries 48..63: swap the 16-entry blocks
            for x in (q, k):
                x[i][..., :16], x[i][..., 16:32] = x[i][..., 16:32].copy(), x[i][..., :16].copy()
                x[i][..., 32:48], x[i][..., 48:64] = x[i][..., 48:64].copy(), x[i][..., 32:48].copy()
        q[i][..., units[1 - i % 2] > 0] = 0.0
        qi = q[i]
        qi[~c["anchor"][i], :, 32:64] = 0.0  # every other row is blind to both anchor vectors
        qi[c["anchor"][i]] = anchors[i % 2]
        if i:
            n = min(G, int(klens[i]))
            k[i, :n] = _round(np.float32(90.0 / p) * (units[1 - i % 2] + anchors[1 - i % 2]), dt) + c["own"][i]
    c["q"], c["k"] = q, k
    last = (nb - 1) % 2
    c["tail_k"] = _round((np.float32(90.0 / p) * (units[last] + anchors[last]))[None, None, :].repeat(G, 0).repeat(Hkv, 1), dt)  # [G, Hkv, D] behind the last group
    c["tail_v"] = np.full((G, Hkv, D), np.nan, np.float32)
    c["giant_rows"] = [(i, 0, min(G, int(klens[i]))) for i in range(1, nb)]
    return c


def zero_behind(c: dict) -> dict:
    """the twin of a giants_case with zeros where the giants (and NaN / Inf) are"""
    z = dict(c, k=c["k"].copy(), v=c["v"].copy())
    for i, a, b in c["giant_rows"]:
        z["k"][i, a:b] = c["own"][i] if c["ragged"] else 0.0  # (ragged: they stay the group's own keys, at -60 for its anchor token)
        if not c["ragged"]:
            z["v"][i, a:b] = 0.0
    if c["ragged"]:
        z["tail_k"], z["tail_v"] = np.zeros_like(c["tail_k"]), np.zeros_like(c["tail_v"])
    return z


def pack_keys(c: dict):
    """(k, v [total + tail, Hkv, D], cu_seqlens_k [nb + 1]) of a ragged case: the groups back to back, tail_k / tail_v (if any) behind"""
    ks = [c["k"][i, :int(n)] for i, n in enumerate(c["klens"])] + ([c["tail_k"]] if "tail_k" in c else [])
    vs = [c["v"][i, :int(n)] for i, n in enumerate(c["klens"])] + ([c["tail_v"]] if "tail_v" in c else [])
    cu = np.concatenate([[0], np.cumsum(c["klens"])]).astype(np.int32)
    return np.concatenate(ks, 0), np.concatenate(vs, 0), cu
