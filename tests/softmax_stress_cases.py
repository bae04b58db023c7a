"""Adversarial softmax inputs for the suffix kernels and the LSE merges (numpy only: importable without a GPU).

Random normal data leaves the online softmax unobserved: the running maximum settles in the first chunk, every worker (wave, lane
group, token-split slice) holds about the same mass, no weight underflows and a `-inf` guard is met by empty sequences only.  The
builders here give every key a CHOSEN score -- the exact-score construction of
tests/test_edge_gpu.py::test_prefix_sum_tested_softmax_on_adversarial_scores: `unit` is D zeros with the first 16 entries 1,
q = unit + 0.01 noise, k[b, j] = amp[b, j] * unit + 0.01 noise, so that q . k * D^-0.5 * log2(e) = amp * PER(D) log2-units -- and
every partial of a merge a chosen LSE.  |score| stays at or below 200 log2-units: the fp32 rounding of a score (|s| 2^-23, a few
times) then stays below 1e-4 of a probability and every amplitude fits fp16.

Tables: SUFFIX_ROUTES / FP8_ROUTES (which kernel a shape reaches, by the launcher rule `suffix_route` restates), PARTIAL_ROUTES
(hand-made partials into hyd_suffix_attn_fwd), SCORE_PATTERNS, LSE_PATTERNS.  tests/test_softmax_stress.py shows on the CPU that the
reference's own rounding model meets the GPU tests' bounds on these inputs with twofold room; tests/test_softmax_stress_gpu.py runs
them through the kernels."""
from __future__ import annotations

import zlib

import numpy as np

from oracle import hydragen_oracle as O
from tests.cases import _round

LOG2E = 1.4426950408889634
MAX_SCORE = 200.0  # log2-units
LISTED_LENS = (1, 31, 32, 33, 64)  # + the full capacity: in every table (those that fit the cache)
BLOCK = 24  # sequences built (and given to the oracle) for a batch of more than 64: the batch repeats this block, see `block_index`


def per(D: int) -> float:
    """log2-units of score per unit of amplitude"""
    return 16 * D ** -0.5 * LOG2E


def unit_vector(D: int) -> np.ndarray:
    u = np.zeros(D, np.float32)
    u[:16] = 1.0
    return u


# ---- routes -----------------------------------------------------------------------------------------------------------------
def suffix_route(B, Hq, Hkv, cap, D=128, nq=1, n_pre=0) -> str:
    """The kernel hyd_suffix_attn_fwd picks for 16-bit caches, restated from the launchers (shapes only, as there):
    suffix_attn.hip `launch_suffix` -> suffix_attn_gqa.hip `suffix_gqa_eligible` (rows >= 3; not D = 256 with gqa_few_units) and
    suffix_gqa_common.h `gqa_few_units` (units * chunks < 1024 and kv_len >= 128: four waves per unit);
    suffix_attn.hip `launch_suffix_t` (token-row kernel: suffix_rows.h `suffix_rows_shape_ok`, not (units < 2048 and kv_len >= 64),
    kv_len <= 1024), suffix_rows.h `launch_suffix_rows` (waves per sequence, token split TS = 2 / 4 when one wave covers a token's
    heads, n_pre < 2 and kv_len >= 32; the NPRE = 2 instantiation); suffix_attn.hip `launch_suffix_r` (R = 1 / 2 / 4 / 8 rows per
    unit, four waves per unit when units * row_chunks < 2048 and kv_len >= 64) and `suffix_packed_eligible` (lengths <= 12 of an
    R = 1 one-wave unit take the packed lane-group body)."""
    g = Hq // Hkv
    rows, units = nq * g, B * Hkv
    chunks = (rows + 15) // 16
    gqa_few = units * chunks < 256 * 4 and cap >= 128
    if rows >= 3 and not (D == 256 and gqa_few):
        return "gqa/4-waves" if gqa_few else "gqa/1-wave"
    hpi = 64 // (D // 8)
    if rows == 1 and nq == 1 and g == 1 and Hkv % hpi == 0 and n_pre <= 2 and not (units < 2048 and cap >= 64) and cap <= 1024:
        wps = Hkv // hpi
        if n_pre == 2:
            return "rows/npre2"
        if wps == 1 and cap >= 32:
            return "rows/ts2" if B <= 2048 else "rows/ts4"
        return f"rows/{min(wps, 4)}wps"
    R = 1 if rows <= 1 else 2 if rows <= 2 else 4 if rows <= 4 else 8
    few = units * ((rows + R - 1) // R) < 2 * 256 * 4 and cap >= 64
    packed = R == 1 and not few and D == 128 and nq == 1 and g == 1 and Hkv >= hpi
    return f"unit/R{R}/" + ("4-waves" if few else "1-wave+packed" if packed else "1-wave")


# name -> (B, Hq, Hkv, cap, D, nq, route key, what the route is and the rule that selects it)
SUFFIX_ROUTES = {
    "rows_4wps": (130, 16, 16, 40, 128, 1, "rows/4wps",
                  "token-row kernel, 4 waves per sequence (launch_suffix_t: 2080 units; launch_suffix_rows: wps = Hkv / 4)"),
    "rows_ts2": (520, 4, 4, 40, 128, 1, "rows/ts2",
                 "token-row kernel, token split TS = 2 (launch_suffix_rows: wps = 1, kv_len >= 32, B <= 2048)"),
    "rows_ts4": (2100, 4, 4, 40, 128, 1, "rows/ts4",
                 "token-row kernel, token split TS = 4 (launch_suffix_rows: wps = 1, kv_len >= 32, B > 2048)"),
    # (50, 4, 4, 20) is the row tests/test_seq_order_gpu.py calls the lane-group path; by launch_suffix_t it is the token-row kernel
    # (suffix_rows_shape_ok holds and kv_len < 64 keeps it off the few-units exception), four sequences per workgroup
    "rows_unsplit": (50, 4, 4, 20, 128, 1, "rows/1wps",
                     "token-row kernel, one wave per sequence, no token split (launch_suffix_rows: kv_len < 32)"),
    "unit_few": (37, 8, 8, 300, 128, 1, "unit/R1/4-waves",
                 "one-unit-per-wave kernel, few_units: 4 waves per unit (launch_suffix_r: 296 units < 2048, kv_len >= 64)"),
    "unit_packed": (50, 6, 6, 20, 128, 1, "unit/R1/1-wave+packed",
                    "one-unit-per-wave kernel, one wave per unit; lengths <= 12 take the packed lane-group body, two idle lane "
                    "groups (launch_suffix_t: Hkv % 4 != 0 fails suffix_rows_shape_ok; suffix_packed_eligible: Hkv >= 4)"),
    # two / four rows per unit: with the shipped rules R = 2 needs nq * g = 2, and R = 4 only runs where the grouped-query kernel
    # refuses 3..4 rows -- D = 256 with few units (suffix_gqa_eligible)
    "unit_r2": (40, 4, 4, 70, 128, 2, "unit/R2/4-waves",
                "one-unit-per-wave kernel, R = 2 rows per unit (nq = 2, Hq = Hkv), 4 waves per unit (launch_suffix_r)"),
    "unit_r4": (8, 4, 1, 300, 256, 1, "unit/R4/4-waves",
                "one-unit-per-wave kernel, R = 4 rows per unit at D = 256 (suffix_gqa_eligible refuses D = 256 with gqa_few_units)"),
    "gqa_1wave": (90, 32, 8, 70, 128, 1, "gqa/1-wave",
                  "grouped-query kernel, one wave per unit, 4 kv heads per workgroup (suffix_gqa_eligible; gqa_launch_plan)"),
    "gqa_4waves": (9, 8, 1, 300, 128, 1, "gqa/4-waves",
                   "grouped-query kernel, 4 waves per unit (gqa_few_units: 9 units, kv_len >= 128)"),
    "rows_d64": (260, 8, 8, 50, 64, 1, "rows/ts2", "token-row kernel at D = 64: 8 heads per wave instruction, token split TS = 2"),
    "rows_d256": (513, 4, 4, 18, 256, 1, "rows/2wps", "token-row kernel at D = 256: 2 heads per wave instruction, 2 waves per sequence"),
    "gqa_d64": (128, 8, 2, 70, 64, 1, "gqa/1-wave", "grouped-query kernel at D = 64 (two tile sets), one wave per unit"),
    "gqa_d256": (256, 8, 1, 70, 256, 1, "gqa/1-wave", "grouped-query kernel at D = 256, one wave per unit"),
}

# fp8 unique caches, D = 128: (B, Hq, Hkv, cap, what) -- shapes of tests/test_fp8_kv_gpu.py (B = 1024 / 7, Hkv = 4 / 8, S = 48 / 160)
# and of tests/test_fp8_gqa_gpu.py SHAPES
FP8_ROUTES = {
    "fp8_rows_ts2": (1024, 4, 4, 48, "fp8 token-row kernel (suffix_attn_fp8.hip), token split TS = 2"),
    "fp8_rows_2wps": (7, 8, 8, 160, "fp8 token-row kernel, 2 waves per sequence (the fp8 launcher has no few-units exception)"),
    "fp8_gqa_1wave": (128, 32, 8, 96, "suffix_attn_gqa_fp8.hip, one wave per unit, 4 kv heads per workgroup"),
    "fp8_gqa_4waves": (8, 8, 2, 160, "suffix_attn_gqa_fp8.hip, four waves per unit (gqa_few_units; 8 sequences, not 4, for the listed lengths)"),
}

# hand-made partials into hyd_suffix_attn_fwd: name -> (B, Hq, Hkv, cap, leading 16-bit partials, route key, what); shapes from the
# rows of tests/test_suffix_partials_gpu.py and tests/test_token_row_gpu.py whose comments name the route
PARTIAL_ROUTES = {
    "unit_few": (200, 4, 4, 90, 0, "unit/R1/4-waves", "dot-product (one-unit-per-wave) kernel: finish_row with NBATCH = 4, nothing prefetched"),
    "rows_npre1": (66, 32, 32, 72, 1, "rows/4wps", "token-row kernel, one prefetched 16-bit partial; finish_row with NBATCH = 2"),
    "rows_npre2": (66, 32, 32, 40, 2, "rows/npre2", "token-row kernel, two prefetched 16-bit partials (NPRE = 2 instantiation)"),
    "gqa_1wave": (300, 8, 2, 100, 1, "gqa/1-wave", "grouped-query kernel, one wave per unit: partials folded under the K/V stream"),
    "gqa_4waves": (9, 8, 1, 300, 1, "gqa/4-waves", "grouped-query kernel, 4 waves per unit: partials dealt over the waves, wave merge"),
}
DOT_PRODUCT_PARTIAL_ROUTES = ("unit_few", "rows_npre1", "rows_npre2")
GQA_PARTIAL_ROUTES = ("gqa_1wave", "gqa_4waves")

SCORE_PATTERNS = ("far_below", "far_above", "ramp_up", "ramp_down", "last_key_spike", "spike_behind_length", "two_equal_spikes",
                  "first_half_negligible", "ties")
FP8_SCORE_PATTERNS = ("last_key_spike", "spike_behind_length", "two_equal_spikes")
LSE_PATTERNS = ("far_apart", "all_low", "all_high", "ties", "near_ties", "suffix_empty", "partials_empty", "all_empty")
TIES_COUNTS = (1, 2, 3, 5, 6, 7)  # the last batch of finish_row (NBATCH 2 and 4) is partial for most of them


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


def block_size(B: int) -> int:
    return B if B <= 64 else BLOCK  # 24: the 6 listed lengths, the empty sequence and 17 others


def block_index(B: int) -> np.ndarray:
    """Sequence b of a batch of B holds the data of sequence b % block_size(B) of the built block: batches are large only to reach
    a route, so the oracle runs on one block and still stands for every row the kernel returns."""
    return np.arange(B) % block_size(B)


def lengths(B: int, cap: int, seed: int, empty: bool = True) -> np.ndarray:
    """Ragged lengths of a block: the listed ones that fit, the capacity, one empty sequence, the rest drawn from 1..cap."""
    rng = np.random.default_rng(seed)
    nb = block_size(B)
    listed = [x for x in LISTED_LENS if x < cap] + [cap]
    assert nb > len(listed), (B, cap)
    sl = rng.integers(1, cap + 1, nb).astype(np.int32)
    sl[:len(listed)] = listed
    if empty:
        sl[len(listed)] = 0
    return sl


def amplitudes(pattern: str, lens: np.ndarray, cap: int, D: int, rng) -> np.ndarray:
    """amp [nb, cap] (float64, in units of amplitude): key j of sequence b scores amp[b, j] * per(D) log2-units."""
    p = per(D)
    nb = len(lens)
    j = np.arange(cap, dtype=np.float64)
    amp = np.zeros((nb, cap))
    if pattern in ("far_below", "far_above"):
        amp[:] = (-60.0 if pattern == "far_below" else 60.0) / p + 0.5 * rng.standard_normal((nb, cap)) / p  # +- 0.5 log2-units
    elif pattern in ("ramp_up", "ramp_down"):
        step = min(2.8, MAX_SCORE / max(cap - 1, 1))  # 2.8 per key; flatter on long caches, where 2.8 would pass MAX_SCORE
        amp[:] = (step if pattern == "ramp_up" else -step) * j / p
    elif pattern == "ties":
        pass  # q = 0: the keys do not matter
    else:
        for b, n in enumerate(int(x) for x in lens):
            if pattern == "spike_behind_length":
                amp[b, n:] = 90.0 / p  # finite keys behind the length: never to be looked at
            if n == 0:
                continue
            if pattern == "last_key_spike":
                amp[b, n - 1] = 30.0 / p
            elif pattern == "spike_behind_length":
                amp[b, n - 1] = 10.0 / p
            elif pattern == "two_equal_spikes":
                amp[b, 0] = amp[b, n - 1] = 25.0 / p
            elif pattern == "first_half_negligible":
                amp[b, : n // 2] = -80.0 / p
    assert np.abs(amp).max() * p <= MAX_SCORE + 2.0, pattern
    return amp


def score_case(route: str, pattern: str, dt: str, nb: int | None = None) -> dict:
    """One block of a SUFFIX_ROUTES row: q [nb, nq, Hq, D], k / v [nb, cap, Hkv, D] (float32, rounded to dt), lens [nb]."""
    B, Hq, Hkv, cap, D, nq = SUFFIX_ROUTES[route][:6]
    return _score_case(B, Hq, Hkv, cap, D, nq, pattern, dt, _seed(route, pattern), nb)


def _score_case(B, Hq, Hkv, cap, D, nq, pattern, dt, seed, nb=None) -> dict:
    rng = np.random.default_rng(seed)
    lens = lengths(B, cap, seed)
    if nb is not None:
        lens = lens[:nb]
    nb = len(lens)
    unit = unit_vector(D)
    amp = amplitudes(pattern, lens, cap, D, rng)
    noise = lambda *s: 0.01 * rng.standard_normal(s, dtype=np.float32)  # noqa: E731
    q = np.broadcast_to(unit, (nb, nq, Hq, D)) + noise(nb, nq, Hq, D)
    k = (amp[:, :, None, None] * unit).astype(np.float32).repeat(Hkv, 2) + noise(nb, cap, Hkv, D)
    if pattern == "ties":
        q = np.zeros_like(q)
    v = rng.standard_normal((nb, cap, Hkv, D), dtype=np.float32)
    return dict(q=_round(q, dt), k=_round(k, dt), v=_round(v, dt), lens=lens, B=B, cap=cap, D=D, pattern=pattern, dt=dt)


def zero_behind_length(k: np.ndarray, lens: np.ndarray) -> np.ndarray:
    z = k.copy()
    for b, n in enumerate(lens):
        z[b, int(n):] = 0.0
    return z


def ties_closed_form(v: np.ndarray, lens: np.ndarray, Hq: int, nq: int = 1):
    """q = 0: out = the mean of v[:len], lse = ln(len) (rows of empty sequences: 0 / -inf)."""
    nb, _, Hkv, D = v.shape
    out = np.zeros((nb, nq, Hq, D))
    lse = np.full((nb, nq, Hq), -np.inf)
    for b, n in enumerate(int(x) for x in lens):
        if n:
            out[b] = np.repeat(v[b, :n].astype(np.float64).mean(0), Hq // Hkv, axis=0)[None]
            lse[b] = np.log(n)
    return out, lse


# ---- fp8 caches -------------------------------------------------------------------------------------------------------------
def round_e4m3(x: np.ndarray) -> np.ndarray:
    """Round to the nearest float8_e4m3fn value (ties to even), saturating at 448: 3 mantissa bits, normals from 2^-6, subnormal
    step 2^-9."""
    x = np.asarray(x, dtype=np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -6)))
    step = 2.0 ** (e - 3)
    return np.clip(np.round(x / step) * step, -448.0, 448.0)


def fp8_scales(Hkv: int, rng) -> np.ndarray:
    """Per-head scales in 2^-4 .. 2^4 with 4 significant bits (fp8 value x scale is then exact in bf16 and f16, as in
    tests/test_fp8_kv_gpu.py `_caches`); odd heads are no power of two."""
    frac = np.where(np.arange(Hkv) % 2 == 1, rng.integers(1, 8, Hkv), 0)
    return ((1 + frac / 8) * 2.0 ** rng.integers(-4, 4, Hkv)).astype(np.float32)


def fp8_score_case(route: str, pattern: str, dt: str) -> dict:
    """As score_case, with caches given as e4m3-representable values k8 / v8 (float32; the cache holds exactly these) and per-head
    scales: the dequantized key is k8 * k_scale.  A key's amplitude is what its e4m3 value times the scale makes of the pattern's
    (spikes move by up to 6 %, equal spikes stay equal; the +90 behind the length saturates at 448 * k_scale, 57 log2-units or more)."""
    B, Hq, Hkv, cap = FP8_ROUTES[route][:4]
    D, seed = 128, _seed(route, pattern)
    rng = np.random.default_rng(seed)
    lens = lengths(B, cap, seed)
    nb = len(lens)
    unit = unit_vector(D)
    amp = amplitudes(pattern, lens, cap, D, rng)
    ks, vs = fp8_scales(Hkv, rng), fp8_scales(Hkv, rng)
    q = np.broadcast_to(unit, (nb, 1, Hq, D)) + 0.01 * rng.standard_normal((nb, 1, Hq, D), dtype=np.float32)
    k = (amp[:, :, None, None] * unit).astype(np.float32).repeat(Hkv, 2) + 0.01 * rng.standard_normal((nb, cap, Hkv, D), dtype=np.float32)
    v = rng.standard_normal((nb, cap, Hkv, D), dtype=np.float32)
    k8 = round_e4m3(k / ks[None, None, :, None]).astype(np.float32)
    v8 = round_e4m3(v / vs[None, None, :, None]).astype(np.float32)
    return dict(q=_round(q, dt), k8=k8, v8=v8, k_scale=ks, v_scale=vs, lens=lens, B=B, cap=cap, D=D, pattern=pattern, dt=dt)


# ---- LSE patterns -----------------------------------------------------------------------------------------------------------
def partial_layout(route: str, n: int) -> list:
    """n partials for a PARTIAL_ROUTES row as [(kind, count)] in the layout of tests/test_suffix_partials_gpu.py ("h": one 16-bit
    partial, "f": one fp32 partial, "s": count stacked fp32 slices): the route's leading 16-bit partials, one fp32 partial, slices."""
    lead = min(max(PARTIAL_ROUTES[route][4], 0), n)
    parts = [("h", 1)] * lead
    rest = n - lead
    if rest >= 3:
        parts.append(("f", 1))
        rest -= 1
    if rest:
        parts.append(("s", rest))
    return parts


def layout_kinds(parts) -> list:
    """is_f32 of every single partial of a layout, in order"""
    return [kind != "h" for kind, cnt in parts for _ in range(cnt)]


def partial_lses(pattern: str, n: int, shape, slse: np.ndarray, rng) -> list:
    """n partial LSEs (natural log, float32, `shape` = [B, nq, Hq]) of an LSE pattern; slse: the suffix pass's own LSE (float64)."""
    rows = int(np.prod(shape))
    if pattern == "far_apart":
        # the dominant partial per output row in turn: slot 0, slot 1 (the prefetched ones), a batch-fetched slot, the last index
        slots = np.asarray(sorted({0, min(1, n - 1), n // 2, n - 1}))
        dom = slots[np.arange(rows) % len(slots)].reshape(shape)
        return [np.where(dom == i, 90.0, -90.0).astype(np.float32) for i in range(n)]
    if pattern in ("all_low", "all_high"):
        base = -200.0 if pattern == "all_low" else 200.0
        return [(base + rng.uniform(-1.0, 1.0, shape)).astype(np.float32) for _ in range(n)]
    if pattern == "ties":
        assert np.isfinite(slse).all()
        return [slse.astype(np.float32) for _ in range(n)]
    if pattern == "near_ties":
        base = np.where(np.isfinite(slse), slse, 0.0)
        return [(base + 1e-3 * (i + 1)).astype(np.float32) for i in range(n)]
    if pattern == "suffix_empty":
        return [(3.0 + 2.0 * rng.standard_normal(shape)).astype(np.float32) for _ in range(n)]
    if pattern in ("partials_empty", "all_empty"):
        return [np.full(shape, -np.inf, np.float32) for _ in range(n)]
    raise KeyError(pattern)


def partial_outs(pattern: str, kinds, shape, lses, dt: str, rng) -> list:
    """distinct outs, standard normal (16-bit partials rounded to dt); zero where the partial covers no key"""
    outs = []
    for f32, l in zip(kinds, lses):
        o = rng.standard_normal(shape, dtype=np.float32)
        o = o if f32 else _round(o, dt)
        o[~np.isfinite(l)] = 0.0
        outs.append(o)
    return outs


def merge_lens(pattern: str, lens: np.ndarray) -> np.ndarray:
    """the suffix lengths an LSE pattern runs on"""
    if pattern in ("suffix_empty", "all_empty"):
        return np.zeros_like(lens)
    if pattern == "ties":
        return np.maximum(lens, 1)  # every row has a suffix LSE to tie with
    return lens


def merge_case(route: str, pattern: str, dt: str, n: int | None = None, scores: str | None = None, nb: int | None = None) -> dict:
    """A PARTIAL_ROUTES block: standard normal q / k / v (or a score pattern: `scores`) with ragged lengths, n hand-made partials of
    an LSE pattern, and what the merge must give: `want` = O.combine_lse(partials + the oracle's suffix attention)."""
    B, Hq, Hkv, cap = PARTIAL_ROUTES[route][:4]
    D, seed = 128, _seed(route, pattern, n, scores)
    rng = np.random.default_rng(seed)
    if scores is None:
        lens = lengths(B, cap, seed)
        rnd = lambda *s: _round(rng.standard_normal(s, dtype=np.float32), dt)  # noqa: E731
        q, k, v = rnd(len(lens), 1, Hq, D), rnd(len(lens), cap, Hkv, D), rnd(len(lens), cap, Hkv, D)
    else:
        c = _score_case(B, Hq, Hkv, cap, D, 1, scores, dt, seed)
        q, k, v, lens = c["q"], c["k"], c["v"], c["lens"]
    if nb is not None:
        q, k, v, lens = q[:nb], k[:nb], v[:nb], lens[:nb]
    lens = merge_lens(pattern, lens)
    parts = partial_layout(route, 7 if n is None else n)
    kinds = layout_kinds(parts)
    so, slse = O.flash_attention_seqlen(q, k, v, lens)
    so = np.where(np.isfinite(slse)[..., None], so, 0.0)
    lses = partial_lses(pattern, len(kinds), slse.shape, slse, rng)
    outs = partial_outs(pattern, kinds, so.shape, lses, dt, rng)
    want = O.combine_lse(outs + [so], lses + [slse])
    ok = np.isfinite(np.stack(lses + [slse]).max(0))  # rows where at least one partial or one key exists
    want = np.where(ok[..., None], want, 0.0)  # nothing to attend to anywhere: out = 0 (the convention tests/test_fuzz_gpu.py states)
    return dict(q=q, k=k, v=v, lens=lens, parts=parts, kinds=kinds, outs=outs, lses=lses, suffix_out=so, suffix_lse=slse, want=want,
                ok=ok, B=B, dt=dt, pattern=pattern)


def combine_case(pattern: str, n: int, D: int, seed: int = 0) -> dict:
    """n fp32 partials [3, 2, 4, D] for combine_lse / _combine_many; the last one plays the suffix pass's part in the patterns that
    name it (ties: all equal; suffix_empty: the last is -inf; partials_empty: all but the last)."""
    rng = np.random.default_rng(_seed("combine", pattern, n, D, seed))
    shape = (3, 2, 4, D)
    last = (1.5 + rng.standard_normal(shape[:-1])).astype(np.float32)
    if pattern in ("suffix_empty", "all_empty"):
        last = np.full(shape[:-1], -np.inf, np.float32)
    lses = partial_lses(pattern, n - 1, shape[:-1], last.astype(np.float64), rng) + [last]
    if pattern == "far_apart":
        lses = partial_lses(pattern, n, shape[:-1], None, rng)
    outs = partial_outs(pattern, [True] * n, shape, lses, "f16", rng)
    ok = np.isfinite(np.stack(lses).max(0))
    want = np.where(ok[..., None], O.combine_lse(outs, lses), 0.0)
    return dict(outs=outs, lses=lses, want=want, ok=ok)


def combine_f32(outs, lses) -> np.ndarray:
    """attention.py:21-43 in numpy float32: the rounding model of an fp32 merge"""
    o = np.stack(outs).astype(np.float32)
    l = np.stack(lses).astype(np.float32)
    m = l.max(0)
    m = np.where(np.isfinite(m), m, np.float32(0))
    w = np.exp(l - m[None], dtype=np.float32)
    den = w.sum(0, dtype=np.float32)
    num = (o * w[..., None]).sum(0, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den[..., None] > 0, num / den[..., None], np.float32(0))


# ---- the whole operator: real LSEs ----------------------------------------------------------------------------------------------
OPERATOR_MASS = ("prefix", "suffix", "equal")
OPERATOR_SHAPES = {"decode_gqa": (4, 16, 4, 40), "mha": (4, 8, 8, 40)}  # (B, Hq, Hkv, unique capacity), D = 128


def operator_case(shape: str, mass: str, P: int, hot_at: int, dt: str, levels: int = 1) -> dict:
    """One shared level of P keys (plus, for levels = 2, a second one of 24 keys per pair of sequences whose keys are negligible)
    and ragged unique keys, by the `amp` mechanism.  The level's mass sits in 5 keys from `hot_at` on; its other keys score 100
    log2-units lower (69 in natural log: the other slices of a split prefix pass end 60 or more below the hot one).
    mass = "prefix": hot prefix keys +40, unique keys -40; "suffix": -40 / +40; "equal": ONE hot prefix key at 0 whose row is also
    every sequence's unique key 0, the other unique keys at -100 -- the two LSEs then agree to 2^-100 x the key counts."""
    B, Hq, Hkv, cap = OPERATOR_SHAPES[shape]
    D, p = 128, per(128)
    rng = np.random.default_rng(_seed(shape, mass, P, hot_at, levels))
    lens = lengths(B + len(LISTED_LENS) + 2, cap, 1, empty=False)[:B]  # 1, 31, 32, 33 at capacity 40
    lens[-1] = cap
    unit = unit_vector(D)
    hot_p, hot_u = {"prefix": (40.0, -40.0), "suffix": (-40.0, 40.0), "equal": (0.0, 0.0)}[mass]
    nhot = 1 if mass == "equal" else 5
    amp_p = np.full(P, (hot_p - 100.0) / p)
    amp_p[hot_at:hot_at + nhot] = hot_p / p
    amp_u = np.full((B, cap), hot_u / p)
    if mass == "equal":
        amp_u[:, 1:] = -100.0 / p
    noise = lambda *s: 0.01 * rng.standard_normal(s, dtype=np.float32)  # noqa: E731
    q = _round(np.broadcast_to(unit, (B, 1, Hq, D)) + noise(B, 1, Hq, D), dt)
    sk = _round((amp_p[None, :, None, None] * unit).astype(np.float32).repeat(Hkv, 2) + noise(1, P, Hkv, D), dt)
    k = _round((amp_u[:, :, None, None] * unit).astype(np.float32).repeat(Hkv, 2) + noise(B, cap, Hkv, D), dt)
    if mass == "equal":
        k[:, 0] = sk[0, hot_at]
    sv = _round(rng.standard_normal((1, P, Hkv, D), dtype=np.float32), dt)
    v = _round(rng.standard_normal((B, cap, Hkv, D), dtype=np.float32), dt)
    sks, svs = [sk], [sv]
    if levels == 2:
        low = (min(hot_p, hot_u) - 100.0) / p
        sks.append(_round((np.full((2, 24, 1, 1), low) * unit).astype(np.float32).repeat(Hkv, 2) + noise(2, 24, Hkv, D), dt))
        svs.append(_round(rng.standard_normal((2, 24, Hkv, D), dtype=np.float32), dt))
    return dict(q=q, k=k, v=v, lens=lens, shared_ks=sks, shared_vs=svs, dt=dt)


# ---- the causal tail (hyd_suffix_attn_causal_fwd): a per-row key limit in the score mask ------------------------------------------
def causal_route(B, Hq, Hkv, cap, D, T) -> str:
    """The kernel hyd_suffix_attn_causal_fwd picks, restated from suffix_attn_causal.hip (shapes only, as there):
    `suffix_causal_eligible` (2..8 tokens; the matrix-core kernel's shapes, 2-row units, or D = 256), `launch_causal_t` ->
    suffix_attn_gqa.hip `suffix_gqa_eligible` (rows >= 3; not D = 256 with gqa_few_units) -> `launch_causal_gqa_t` with
    suffix_gqa_common.h `gqa_launch_plan` (gqa_few_units: units * chunks < 1024 and kv_len >= 128 -> four waves per unit; else 4 / 2 / 1
    kv heads per workgroup, at most 2 at D = 256); what is left -> `launch_causal_unit_r` with R = 2 (rows <= 2), 4 or 8 (D = 256),
    four waves per unit when units * row_chunks < 2048 and kv_len >= 64."""
    g = Hq // Hkv
    rows, units = T * g, B * Hkv
    chunks = (rows + 15) // 16
    few = units * chunks < 256 * 4 and cap >= 128
    gqa = rows >= 3 and not (D == 256 and few)
    if not (2 <= T <= 8) or D not in (64, 128, 256) or not (gqa or rows <= 2 or D == 256):
        return "refused"
    if gqa:
        if few:
            return "gqa/4-waves"
        hpw = (4 if Hkv % 4 == 0 else 2 if Hkv % 2 == 0 else 1) if Hkv <= 8 else 1
        return f"gqa/1-wave/hpw{min(hpw, 2) if D == 256 else hpw}"
    R = 2 if rows <= 2 else 4 if rows <= 4 else 8
    few = units * ((rows + R - 1) // R) < 2 * 256 * 4 and cap >= 64
    return f"unit/R{R}/" + ("4-waves" if few else "1-wave")


# name -> (B, Hq, Hkv, cap, D, T, route key, what); B = 0: one sequence per listed length (causal_lengths), no more
CAUSAL_ROUTES = {
    "gqa_hpw4": (0, 8, 4, 40, 64, 3, "gqa/1-wave/hpw4", "matrix-core kernel, one wave per unit, 4 kv heads per workgroup (kv_len < 128)"),
    "gqa_hpw2": (0, 6, 2, 70, 128, 8, "gqa/1-wave/hpw2",
                 "matrix-core kernel, one wave per unit, 2 kv heads per workgroup; g = 3: a 16-row chunk boundary falls inside a token"),
    "gqa_hpw1": (0, 8, 1, 40, 128, 4, "gqa/1-wave/hpw1", "matrix-core kernel, one wave per unit, 1 kv head per workgroup"),
    "gqa_4waves": (0, 8, 1, 132, 128, 5, "gqa/4-waves", "matrix-core kernel, four waves per unit (gqa_few_units), three row chunks"),
    "gqa_4waves_tiles": (0, 8, 2, 300, 128, 8, "gqa/4-waves", "matrix-core kernel, four waves per unit, every wave walks several tiles"),
    "gqa_1wave_long": (520, 8, 2, 132, 128, 3, "gqa/1-wave/hpw2",
                       "matrix-core kernel, one wave per unit on a cache of >= 128 keys (1040 units x 1 chunk >= 1024): a repeated block"),
    "unit_r2_1wave": (0, 4, 4, 40, 64, 2, "unit/R2/1-wave", "dot-product kernel, R = 2, one wave per unit (kv_len < 64)"),
    "unit_r2_4waves": (0, 4, 4, 132, 128, 2, "unit/R2/4-waves", "dot-product kernel, R = 2, four waves per unit"),
    "unit_d256_r2": (0, 4, 4, 132, 256, 2, "unit/R2/4-waves", "dot-product kernel at D = 256, R = 2, four waves per unit"),
    "unit_d256_r4": (0, 4, 4, 132, 256, 3, "unit/R4/4-waves", "dot-product kernel at D = 256, R = 4 (3 rows; the matrix-core kernel refuses D = 256 with few units)"),
    "unit_d256_r8": (0, 8, 2, 132, 256, 3, "unit/R8/4-waves", "dot-product kernel at D = 256, R = 8 in two row chunks (12 rows)"),
    "gqa_d256": (0, 8, 2, 40, 256, 3, "gqa/1-wave/hpw2", "matrix-core kernel at D = 256, one wave per unit (kv_len < 128)"),
}
CAUSAL_PATTERNS = SCORE_PATTERNS + ("tail_staircase", "giants_behind_row_limit")
CAUSAL_MERGE_ROUTES = ("gqa_4waves", "unit_r2_4waves")  # one matrix-core and one dot-product route, four waves per unit
CAUSAL_LSE_PATTERNS = ("far_apart", "suffix_empty", "partials_empty", "all_empty", "near_ties")


def causal_lengths(T: int, cap: int) -> list:
    """Lengths at which a token's limit lands on a tile or wave boundary, just before and just after it; 0 and a negative length;
    0 < len < T (rows whose limit is <= 0); the capacity and a length beyond it.  33 with T = 8 is the kernel header's own example:
    wave 1 starts beyond row 0's limit."""
    want = [0, -2, 1, T - 1, T, T + 1, 25, 26, 31, 32, 33, 33 + T - 1, 63, 64, 65, 127, 128, 129, 128 + T - 1, cap - 1, cap, cap + 3]
    return list(dict.fromkeys(x for x in want if x <= cap + 3))


def causal_shape(route: str):
    """(B, Hq, Hkv, cap, D, T) with B resolved"""
    B, Hq, Hkv, cap, D, T = CAUSAL_ROUTES[route][:6]
    return (B or len(causal_lengths(T, cap))), Hq, Hkv, cap, D, T


def causal_block_lens(route: str, seed: int) -> np.ndarray:
    """the block's lengths as given to the kernel (unclamped): the listed ones, filled up to BLOCK for a repeated block"""
    B, _, _, cap, _, T = causal_shape(route)
    lens = causal_lengths(T, cap)
    nb = block_size(B)
    assert nb >= len(lens), (route, nb, len(lens))
    lens += np.random.default_rng(seed).integers(1, cap + 1, nb - len(lens)).tolist()
    return np.asarray(lens, np.int32)


def causal_limits(lens: np.ndarray, cap: int, T: int) -> np.ndarray:
    """[nb, T]: keys token i of each sequence sees -- max(0, clamp(len, 0, cap) - (T - 1 - i))"""
    n = np.clip(np.asarray(lens, np.int64), 0, cap)
    return np.maximum(0, n[:, None] - (T - 1 - np.arange(T))[None, :])


def causal_amplitudes(pattern: str, lens: np.ndarray, cap: int, D: int, T: int, rng) -> np.ndarray:
    """`amplitudes` laid out by the sequence's (clamped) length, plus the two patterns that only a per-row limit gives a meaning."""
    n_of = np.clip(lens, 0, cap)
    if pattern in SCORE_PATTERNS:
        return amplitudes(pattern, n_of, cap, D, rng)
    p = per(D)
    amp = np.zeros((len(lens), cap))
    for b, n in enumerate(int(x) for x in n_of):
        if pattern == "tail_staircase":  # token i's newest visible key outweighs everything older by 2^24: out = v[len - T + i]
            amp[b, n:] = 196.0 / p
            for i in range(T):
                if n - T + i >= 0:
                    amp[b, n - T + i] = 24.0 * (i + 1) / p
        elif pattern == "giants_behind_row_limit":  # this step's draft keys and the stale keys behind the length: token 0 sees none
            amp[b, max(n - (T - 1), 0):] = 90.0 / p
            if n - T >= 0:
                amp[b, n - T] = 10.0 / p
        else:
            raise KeyError(pattern)
    assert np.abs(amp).max() * p <= MAX_SCORE, pattern
    return amp


def causal_case(route: str, pattern: str, dt: str) -> dict:
    """One block of a CAUSAL_ROUTES row: q [nb, T, Hq, D], k / v [nb, cap, Hkv, D] (float32, rounded to dt), lens [nb] as given to
    the kernel.  The sequence of length cap + 3 holds the data of the one of length cap, the one of length -2 that of length 0: the
    clamps must give the same bits."""
    B, Hq, Hkv, cap, D, T = causal_shape(route)
    seed = _seed("causal", route, pattern)
    rng = np.random.default_rng(seed)
    lens = causal_block_lens(route, seed)
    nb = len(lens)
    unit = unit_vector(D)
    amp = causal_amplitudes(pattern, lens, cap, D, T, rng)
    noise = lambda *s: 0.01 * rng.standard_normal(s, dtype=np.float32)  # noqa: E731
    q = np.broadcast_to(unit, (nb, T, Hq, D)) + noise(nb, T, Hq, D)
    k = (amp[:, :, None, None] * unit).astype(np.float32).repeat(Hkv, 2) + noise(nb, cap, Hkv, D)
    if pattern == "ties":
        q = np.zeros_like(q)
    v = rng.standard_normal((nb, cap, Hkv, D), dtype=np.float32)
    twins = [(list(lens).index(cap + 3), list(lens).index(cap)), (list(lens).index(-2), list(lens).index(0))]
    for dst, src in twins:
        q[dst], k[dst], v[dst] = q[src], k[src], v[src]
    return dict(q=_round(q, dt), k=_round(k, dt), v=_round(v, dt), lens=lens, lim=causal_limits(lens, cap, T), twins=twins, B=B, cap=cap,
                D=D, T=T, Hq=Hq, pattern=pattern, dt=dt)


def causal_reference(q, k, v, lens, round_p=None):
    """float64: per token i, O.flash_attention_seqlen over max(0, clamp(len, 0, cap) - (T - 1 - i)) keys; zeros and -inf where that
    count is 0 (the rule tests/test_speculative.py::dense_causal_tail states)."""
    nb, T, Hq, D = q.shape
    lim = causal_limits(lens, k.shape[1], T)
    out, lse = np.zeros((nb, T, Hq, D)), np.full((nb, T, Hq), -np.inf)
    for i in range(T):
        has = lim[:, i] > 0
        if has.any():
            o, l = O.flash_attention_seqlen(q[has, i:i + 1], k[has], v[has], lim[has, i], round_p=round_p)
            out[has, i], lse[has, i] = o[:, 0], l[:, 0]
    return out, lse


def zero_from(k: np.ndarray, first: np.ndarray) -> np.ndarray:
    """k with the keys from first[b] on zeroed"""
    z = k.copy()
    for b, n in enumerate(first):
        z[b, max(int(n), 0):] = 0.0
    return z


def causal_ties_closed_form(v: np.ndarray, lim: np.ndarray, Hq: int):
    """q = 0: token i returns the mean of v[:lim_i] with lse = ln(lim_i) -- every token's key count, exactly"""
    nb, _, Hkv, D = v.shape
    T = lim.shape[1]
    out, lse = np.zeros((nb, T, Hq, D)), np.full((nb, T, Hq), -np.inf)
    for b in range(nb):
        for i in range(T):
            n = int(lim[b, i])
            if n:
                out[b, i] = np.repeat(v[b, :n].astype(np.float64).mean(0), Hq // Hkv, axis=0)
                lse[b, i] = np.log(n)
    return out, lse


def staircase_closed_form(v: np.ndarray, lim: np.ndarray, Hq: int) -> np.ndarray:
    """tail_staircase: token i returns v[lim_i - 1] = v[len - T + i], to the 2^-24 every older key leaks"""
    nb, _, Hkv, D = v.shape
    out = np.zeros((nb, lim.shape[1], Hq, D))
    for b in range(nb):
        for i in range(lim.shape[1]):
            if lim[b, i]:
                out[b, i] = np.repeat(v[b, int(lim[b, i]) - 1].astype(np.float64), Hq // Hkv, axis=0)
    return out


CAUSAL_MERGE_LAYOUT = [("h", 1), ("f", 1), ("s", 5)]  # one 16-bit partial (prefetched), one fp32 partial, five stacked fp32 slices


def causal_merge_case(route: str, pattern: str, dt: str) -> dict:
    """merge_case through the causal entry point: standard normal q / k / v at the route's listed lengths (0 < len < T among them: a
    token without a unique key), seven hand-made partials of an LSE pattern, `want` = O.combine_lse(partials + causal_reference)."""
    B, Hq, Hkv, cap, D, T = causal_shape(route)
    seed = _seed("causal merge", route, pattern)
    rng = np.random.default_rng(seed)
    lens = causal_block_lens(route, seed)
    nb = len(lens)
    rnd = lambda *s: _round(rng.standard_normal(s, dtype=np.float32), dt)  # noqa: E731
    q, k, v = rnd(nb, T, Hq, D), rnd(nb, cap, Hkv, D), rnd(nb, cap, Hkv, D)
    lens = merge_lens(pattern, lens)
    kinds = layout_kinds(CAUSAL_MERGE_LAYOUT)
    so, slse = causal_reference(q, k, v, lens)
    lses = partial_lses(pattern, len(kinds), slse.shape, slse, rng)
    outs = partial_outs(pattern, kinds, so.shape, lses, dt, rng)
    ok = np.isfinite(np.stack(lses + [slse]).max(0))
    want = np.where(ok[..., None], O.combine_lse(outs + [so], lses + [slse]), 0.0)
    return dict(q=q, k=k, v=v, lens=lens, lim=causal_limits(lens, cap, T), parts=CAUSAL_MERGE_LAYOUT, kinds=kinds, outs=outs, lses=lses,
                suffix_out=so, suffix_lse=slse, want=want, ok=ok, B=B, dt=dt, pattern=pattern)
