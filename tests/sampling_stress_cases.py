"""Adversarial logit rows for the sampling kernels, shared by tests/test_sampling_stress.py (the CPU conditions) and
tests/test_sampling_stress_gpu.py: every case is built on the CPU from its name's seed, so the float64 definition
(hydragen_amd/sampling.py) runs on the very rows the kernels are given.

`randn * 3` leaves the select of csrc/sample_filter.hip / csrc/sample_select.h unobserved: the k-th logit never falls into the last
distance bin (31.875 and more below the maximum), no fixed-point mass underflows (floor(exp(l - max) 2^40) is 0 below max - 27.7),
no threshold sits on a plateau or on a +0 / -0 pair, +inf never occurs and a row always has thousands of valid columns.  The
patterns here put a CHOSEN structure at the threshold, and the cuts of a case are chosen so that the structure decides the kept
count.  Every cut is also placed so that the DEFINITION's kept count does not move when top_p / min_p move by SLACK (asserted in
tests/test_sampling_stress.py): the kernels' fixed-point masses are far more exact than that, so the GPU test demands the float64
count with no allowance.

Most cases give every row the same multiset of values in an independent random permutation: the thresholds are then one
computation on the base row (`top_p_in_group` / `min_p_between` place a cut in the middle of a gap and assert the gap), and the rows
differ in where the chunk loop, the lanes and the waves meet the structure."""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SLACK = 1e-5  # = tests/test_sampling_filters_gpu.py SLACK
ROOM = 3 * SLACK  # the least distance of a chosen top_p / min_p from the next value at which the definition's count changes
MAX_FINITE = {"bf16": 3e38, "f16": 65504.0, "f32": 3e38}  # "at the type's largest finite magnitude" (3e38 rounds to a finite bf16)
TINY = {"bf16": 2.0 ** -133, "f16": 2.0 ** -24, "f32": 2.0 ** -149}  # the smallest denormal
PAD_FILL = {"bf16": 1e30, "f16": 60000.0, "f32": 1e30}  # behind a padded row: a kernel that read it would draw a token >= n

# name -> pattern, n, dtype, rows, pad, pattern parameters.  pad "vec": the row stride is n rounded up to a multiple of 8 (16-byte loads
# and, for an odd n, the scalar tail; rows of 16 columns and fewer stay packed); "odd": an odd row stride, so no 16-byte loads
CASES = {
    "far_tail_bf16": dict(pattern="far_tail", n=2049, dtype="bf16", rows=20, pad="vec"),
    "far_tail_f16_strided": dict(pattern="far_tail", n=8221, dtype="f16", rows=20, pad="odd"),
    "far_tail_f32_128k": dict(pattern="far_tail", n=128256, dtype="f32", rows=10, pad="vec"),
    "underflow_f32": dict(pattern="underflow", n=128256, dtype="f32", rows=6, pad="vec"),
    "underflow_bf16_strided": dict(pattern="underflow", n=128256, dtype="bf16", rows=6, pad="odd"),
    "plateau2_bf16": dict(pattern="plateau", n=2049, dtype="bf16", rows=24, pad="vec", width=2),
    "plateau100_f16": dict(pattern="plateau", n=8221, dtype="f16", rows=24, pad="vec", width=100),
    "plateau100_f32_strided": dict(pattern="plateau", n=31997, dtype="f32", rows=16, pad="odd", width=100),
    "flat_bf16_1": dict(pattern="flat", n=1, dtype="bf16", rows=24, pad="vec"),
    "flat_f16_7": dict(pattern="flat", n=7, dtype="f16", rows=24, pad="vec"),
    "flat_f32_8": dict(pattern="flat", n=8, dtype="f32", rows=24, pad="vec"),
    "flat_bf16_9_strided": dict(pattern="flat", n=9, dtype="bf16", rows=24, pad="odd"),
    "flat_f16_2049": dict(pattern="flat", n=2049, dtype="f16", rows=24, pad="vec"),
    "flat_f32_8221": dict(pattern="flat", n=8221, dtype="f32", rows=24, pad="vec"),
    "signed_zero_bf16": dict(pattern="plateau", n=2049, dtype="bf16", rows=24, pad="vec", width=100, value=0.0, signed_zero=True),
    "signed_zero_f32_strided": dict(pattern="plateau", n=8221, dtype="f32", rows=24, pad="odd", width=100, value=0.0, signed_zero=True),
    "signed_zero_max_f16": dict(pattern="plateau", n=2049, dtype="f16", rows=24, pad="vec", width=4, value=0.0, signed_zero=True, above=0),
    "signed_zero_max_f32_9": dict(pattern="plateau", n=9, dtype="f32", rows=24, pad="vec", width=4, value=0.0, signed_zero=True, above=0),
    "top_p_max_plateau2_bf16": dict(pattern="plateau", n=8221, dtype="bf16", rows=24, pad="vec", width=2, value=3.0, above=0),
    "top_p_max_plateau4_f32": dict(pattern="plateau", n=2049, dtype="f32", rows=24, pad="vec", width=4, value=3.0, above=0),
    "all_negative_bf16": dict(pattern="plateau", n=2049, dtype="bf16", rows=24, pad="vec", width=2, value=-30.0),
    "all_negative_f32": dict(pattern="plateau", n=8221, dtype="f32", rows=24, pad="vec", width=2, value=-30.0),
    "few_valid_f32_9": dict(pattern="few_valid", n=9, dtype="f32", rows=24, pad="vec"),
    "few_valid_f16": dict(pattern="few_valid", n=2049, dtype="f16", rows=24, pad="vec"),
    "few_valid_bf16_strided": dict(pattern="few_valid", n=31997, dtype="bf16", rows=16, pad="odd"),
    "pos_inf_bf16": dict(pattern="pos_inf", n=2049, dtype="bf16", rows=24, pad="vec"),
    "pos_inf_f16_7": dict(pattern="pos_inf", n=7, dtype="f16", rows=24, pad="vec"),
    "pos_inf_f32": dict(pattern="pos_inf", n=8221, dtype="f32", rows=24, pad="vec"),
    "extreme_f16": dict(pattern="extreme", n=2049, dtype="f16", rows=24, pad="vec"),
    "extreme_bf16_strided": dict(pattern="extreme", n=2049, dtype="bf16", rows=24, pad="odd"),
    "extreme_f32": dict(pattern="extreme", n=2049, dtype="f32", rows=24, pad="vec"),
    "denormal_f32": dict(pattern="denormal", n=2049, dtype="f32", rows=24, pad="vec"),
    "denormal_f16": dict(pattern="denormal", n=2049, dtype="f16", rows=24, pad="vec"),
    "denormal_bf16_9": dict(pattern="denormal", n=9, dtype="bf16", rows=24, pad="vec"),  # bf16 has 127 denormals per sign: a small row
    "n_le_top_k_f32_1": dict(pattern="n_le_top_k", n=1, dtype="f32", rows=24, pad="vec"),
    "n_le_top_k_bf16_7": dict(pattern="n_le_top_k", n=7, dtype="bf16", rows=24, pad="vec"),
    "n_le_top_k_f16_8": dict(pattern="n_le_top_k", n=8, dtype="f16", rows=24, pad="vec"),
    "n_le_top_k_f32_9_strided": dict(pattern="n_le_top_k", n=9, dtype="f32", rows=24, pad="odd"),
}
HAS_POS_INF = ("pos_inf",)  # patterns whose rows have no log-prob by the definition


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _round(x64: np.ndarray, dtype: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x64)).to(DT[dtype])


def _permuted(base: torch.Tensor, rows: int, rng) -> torch.Tensor:
    """[rows, n]: independent permutations of the base row (the bits move with the values: -0 stays -0)"""
    n = base.shape[0]
    idx = np.stack([rng.permutation(n) for _ in range(rows)])
    return base[torch.from_numpy(idx)]


def _strided(x: torch.Tensor, pad: int, dtype: str) -> torch.Tensor:
    if not pad:
        return x.contiguous()
    buf = torch.full((x.shape[0], x.shape[1] + pad), PAD_FILL[dtype], dtype=x.dtype)
    buf[:, : x.shape[1]] = x
    return buf[:, : x.shape[1]]


def masses(row64: np.ndarray, top_k=None):
    """(w, survivors) of the definition for one float64 row: w = exp(l - max) (1 at the max, 0 at invalid columns), survivors = the
    valid columns top_k keeps."""
    valid = ~np.isnan(row64) & (row64 != -np.inf)
    xm = np.where(valid, row64, -np.inf)
    m = xm.max()
    with np.errstate(invalid="ignore"):
        w = np.where(valid, np.where(xm == m, 1.0, np.exp(xm - m)), 0.0)
    surv = valid
    if top_k and top_k < valid.sum():
        surv = valid & (xm >= np.sort(xm)[-top_k])
    return w, surv


def top_p_in_group(row64: np.ndarray, value: float, top_k=None) -> float:
    """A top_p whose crossing falls inside the tie group of `value`: the middle between the survivors' mass share above the group and
    the share with it, both at least ROOM away."""
    w, surv = masses(row64, top_k)
    total = w[surv].sum()
    lo, hi = w[surv & (row64 > value)].sum() / total, w[surv & (row64 >= value)].sum() / total
    assert hi - lo > 2 * ROOM, (lo, hi)
    return float(np.float32(0.5 * (lo + hi)))


def min_p_between(row64: np.ndarray, keep_value: float, drop_value: float) -> float:
    """A min_p that keeps keep_value and drops drop_value, both p / p_max at least ROOM away"""
    m = row64[~np.isnan(row64)].max()
    hi, lo = math.exp(keep_value - m), math.exp(drop_value - m)
    assert hi - lo > 2 * ROOM, (lo, hi)
    return float(np.float32(0.5 * (lo + hi)))


# ---- the patterns: (spec, rng) -> (x [rows, n] in the case's dtype, cuts [(top_k, top_p, min_p)], info) -------------------------------
def _grid(count: int, top: float = 4.0) -> np.ndarray:
    """top, top - 1/2, ...: exact in every type; masses 1, .607, .368, .223, .135, .082, ... (shares of a head of h such values:
    h = 2: .622; 3: .506 .813; 4: .455 .731 .899; 5: .429 .689 .846 .942; 6: .414 .665 .818 .910 .966; 7: .406 .652 .801 .892 ...;
    8: .401 .644 .792 .881 ...; 9: .398 .639 .786 .875 ... -- the grid cuts .95 / .8 / .7 keep 1e-3 and more from all of them)"""
    return top - 0.5 * np.arange(count)


def far_tail(c, rng):
    """1..5 head columns on the grid from 4.0 down, everything else 32 to 60 below the maximum: with top_k beyond the head the k-th
    logit lies in distance bin 255 (counted as `total - the other bins`: pick_bin(fill_last)) and is resolved by the radix levels."""
    rows, n = c["rows"], c["n"]
    x = 4.0 - rng.uniform(32.0, 60.0, (rows, n))
    heads = []
    for r in range(rows):
        h = 1 + r % 5
        x[r, rng.choice(n, h, replace=False)] = _grid(h)
        heads.append(h)
    return _round(x, c["dtype"]), [(8, None, None), (None, 0.95, None), (None, None, 0.5), (8, 0.7, None)], dict(heads=heads, top_k=8)


def underflow(c, rng):
    """The maximum 2.0, a second column 8 below it, 10^5 columns 20 to 27.7 below (masses of 2000 down to 1 fixed-point units; three
    fifths of them within 0.5 of max - 20, so that together they hold about 1e-4 of the row) and the rest 28.5 to 40 below (mass 0).
    top_p sits between the maximum's share WITH the small masses and its share WITHOUT them: the definition keeps 2 columns, a select
    that lost the 10^5 small masses would keep 1."""
    rows, n = c["rows"], c["n"]
    base = 2.0 - rng.uniform(28.5, 40.0, n)
    small = rng.choice(n, 100000, replace=False)
    base[small] = 2.0 - (20.0 + 7.7 * rng.uniform(0.0, 1.0, small.size) ** 6)
    rest = np.setdiff1d(np.arange(n), small)
    base[rest[0]], base[rest[1]] = 2.0, -6.0
    base_t = _round(base, c["dtype"])
    b64 = base_t.double().numpy()

    def top_p_counting_small(top_k):
        w, surv = masses(b64, top_k)
        total = w[surv].sum()
        t = w[surv & (b64 <= 2.0 - 19.0)].sum()
        assert t / total > 2 * ROOM, t / total  # the small masses matter
        return float(np.float32(1.0 / (total - 0.5 * t)))  # the maximum's share is 1 / total with them, 1 / (total - t) without

    cuts = [(50000, None, None), (None, top_p_counting_small(None), None), (None, None, 2e-4), (50000, top_p_counting_small(50000), None)]
    return _permuted(base_t, rows, rng), cuts, dict(base=b64)


def plateau(c, rng):
    """`above` columns over a plateau of `width` columns at `value`, everything else at least 1/2 below it: top_k = above + 1 makes
    the plateau the k-th value, top_p crosses inside it, min_p falls between it and the next value below.  signed_zero: value 0
    with +0 and -0 mixed (equal values: all kept together; the key fold of key16 / key32).  above = 0: the plateau is the maximum."""
    rows, n, width = c["rows"], c["n"], c["width"]
    value, above = c.get("value", 1.0), c.get("above", 9)
    base = value - 0.5 - np.minimum(np.abs(rng.standard_normal(n)) * 2.0, 12.0)
    base[:above] = value + 0.25 * np.arange(1, above + 1)
    base[above : above + width] = value
    if c.get("signed_zero"):
        base[above : above + width : 2] = -0.0
    base_t = _round(base, c["dtype"])
    b64 = base_t.double().numpy()
    below = b64[b64 < value].max()
    k = above + 1
    tp, mp = top_p_in_group(b64, value), min_p_between(b64, value, below)
    cuts = [(k, None, None), (None, tp, None), (None, None, mp), (k, top_p_in_group(b64, value, k), mp)]
    return _permuted(base_t, rows, rng), cuts, dict(base=b64, width=width, above=above, value=value)


def flat(c, rng):
    """Every column of a row holds the same value (0, -3.5, 7, -0, 2^-10 by row): every cut keeps the whole row."""
    values = np.array([0.0, -3.5, 7.0, -0.0, 2.0 ** -10])
    x = np.repeat(values[np.arange(c["rows"]) % 5][:, None], c["n"], axis=1)
    return _round(x, c["dtype"]), [(3, None, None), (None, 0.5, None), (None, None, 0.5), (3, 0.5, 0.5)], dict()


def few_valid(c, rng):
    """NaN and -inf everywhere but nvalid = 1, k - 1, k, k + 1 columns (k = top_k = 5, by row), which hold the grid from 2.0 down."""
    rows, n = c["rows"], c["n"]
    x = np.where(rng.random((rows, n)) < 0.5, np.nan, -np.inf)
    nvalid = []
    for r in range(rows):
        nv = (1, 4, 5, 6)[r % 4]
        x[r, rng.choice(n, nv, replace=False)] = _grid(nv, 2.0)
        nvalid.append(nv)
    return _round(x, c["dtype"]), [(5, None, None), (None, 0.8, None), (None, None, 0.3), (5, 0.8, 0.3)], dict(nvalid=nvalid, top_k=5)


def pos_inf(c, rng):
    """One (even rows) or three (odd rows) +inf columns over randn * 3: the maximum is +inf, every finite column is infinitely far
    below it (bin 255, mass 0) and the +inf columns share the whole mass."""
    rows, n = c["rows"], c["n"]
    x = rng.standard_normal((rows, n)) * 3.0
    ninf = []
    for r in range(rows):
        k = 1 if r % 2 == 0 else 3
        x[r, rng.choice(n, k, replace=False)] = np.inf
        ninf.append(k)
    return _round(x, c["dtype"]), [(2, None, None), (None, 0.5, None), (None, None, 0.1), (4, 0.5, None)], dict(ninf=ninf)


def _next_below(t: torch.Tensor) -> torch.Tensor:
    """the next representable value below a positive one"""
    bits = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return (bits - 1).view(t.dtype)


def extreme(c, rng):
    """Two columns at the type's largest magnitude, three at the next value below it (one ulp: 2^120 and more in bf16 / fp32, 32 in
    f16 -- bin 255 either way), three at the negative extreme, randn * 3 elsewhere: m - l overflows to +inf in fp32."""
    n, dt = c["n"], c["dtype"]
    base_t = _round(rng.standard_normal(n) * 3.0, dt)
    big = _round(np.full(1, MAX_FINITE[dt]), dt)
    base_t[0:2] = big
    base_t[2:5] = _next_below(big)
    base_t[5:8] = -big
    cuts = [(4, None, None), (None, 0.5, None), (None, None, 0.5), (20, 0.9, None)]
    return _permuted(base_t, c["rows"], rng), cuts, dict(base=base_t.double().numpy())


def denormal(c, rng):
    """Distinct denormals of both signs and zeros: j * the type's smallest denormal for j = -J .. J.  Every mass is 1 to 1e-38; the
    order is in the low bits of the keys alone."""
    n, dt = c["n"], c["dtype"]
    J = (n - 1) // 2
    j = np.concatenate([np.arange(-J, J + 1), np.zeros(n - 2 * J - 1)]).astype(np.float64)
    base_t = _round(j * TINY[dt], dt)
    cuts = [(5, None, None), (None, 0.3, None), (None, None, 0.5), (5, 0.3, None)]
    return _permuted(base_t, c["rows"], rng), cuts, dict(base=base_t.double().numpy(), J=J)


def n_le_top_k(c, rng):
    """n = 1, 7, 8, 9 columns on the grid from 2.0 down, top_k = n and beyond (no cut), rows narrower than one 8-element chunk."""
    n = c["n"]
    base_t = _round(_grid(n, 2.0), c["dtype"])
    cuts = [(n, None, None), (50, None, None), (None, 0.8, None), (None, None, 0.3), (50, 0.8, 0.3)]
    return _permuted(base_t, c["rows"], rng), cuts, dict(base=base_t.double().numpy())


PATTERNS = dict(far_tail=far_tail, underflow=underflow, plateau=plateau, flat=flat, few_valid=few_valid, pos_inf=pos_inf,
                extreme=extreme, denormal=denormal, n_le_top_k=n_le_top_k)


def pad_of(n: int, kind: str) -> int:
    if kind == "odd":
        return 2 if n % 2 else 1
    return (-n) % 8 if n > 16 else 0


def build(name: str) -> dict:
    """-> dict(x [rows, n] CPU tensor in the case's dtype (a strided view where pad > 0), cuts [(top_k, top_p, min_p)], pattern,
    info: what the pattern claims about itself, for tests/test_sampling_stress.py)"""
    c = CASES[name]
    pad = pad_of(c["n"], c["pad"])
    x, cuts, info = PATTERNS[c["pattern"]](c, _rng(name))
    assert x.shape == (c["rows"], c["n"]) and x.dtype == DT[c["dtype"]]
    return dict(x=_strided(x, pad, c["dtype"]), cuts=cuts, pattern=c["pattern"], info=info, name=name, n=c["n"], dtype=c["dtype"], pad=pad)


def on_device(x: torch.Tensor, dtype: str, device) -> torch.Tensor:
    """The case's rows on `device` with the SAME row stride (a plain .to() would pack a strided view) and the fill behind padded rows."""
    rows, n = x.shape
    stride = x.stride(0) if rows > 1 else n
    if x.is_contiguous() or stride == n:
        return x.contiguous().to(device)
    buf = torch.full((rows, stride), PAD_FILL[dtype], dtype=x.dtype, device=device)
    buf[:, :n] = x.to(device)
    return buf[:, :n]


# ---- rows for the mirror draws (tests/sampler_mirror.py): plain randn * 3 at vocabulary size --------------------------------------
MIRROR_ROWS = 64
MIRROR_SHAPES = [(31997, 2), (128256, 0)]  # (V, pad): 31997 + 2 is an odd row stride (no 16-byte loads); 128256 takes them
MIRROR_TEMPERATURES = (0.7, 1.0)
# bits set in both halves of the seed and of the offset; KEY_VARIANTS differ from MIRROR_KEY in exactly one 32-bit half each
MIRROR_KEY = (0x9E3779B97F4A7C15, 0x0000000500000008)
KEY_VARIANTS = [(MIRROR_KEY[0] ^ 0x00010000, MIRROR_KEY[1]), (MIRROR_KEY[0] ^ (0x00010000 << 32), MIRROR_KEY[1]),
                (MIRROR_KEY[0], MIRROR_KEY[1] ^ 0x00000010), (MIRROR_KEY[0], MIRROR_KEY[1] ^ (0x00000002 << 32))]


def mirror_rows(V: int, pad: int, dtype: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(V + 7 * pad)
    return _strided((torch.randn(MIRROR_ROWS, V, generator=g) * 3.0).to(DT[dtype]), pad, dtype)


# ---- thresholds of the structural statistics: the 1 - 1e-6 quantiles, beside their parameters -------------------------------------
# (tests/test_sampling_stress.py recomputes them with scipy where it imports.)  The tests run at fixed keys: a threshold that a
# correct sampler passes with probability 1 - 1e-6 is a constant of the suite, not a source of flakes.
CHI2_Q = {1: 23.928127, 3: 30.664850, 4: 33.376842, 7: 40.521831, 15: 56.493442}  # degrees of freedom -> chi-square quantile
UNIFORM_ROWS, UNIFORM_V = 16384, 8221
FLAT_ROWS = 4096  # of them, compared with the mirror token by token
POISSON_Q = {UNIFORM_ROWS / UNIFORM_V: 12}  # mean number of coincidences (rows x sum p^2, p = 1 / V) -> Poisson quantile


def chi_square(counts, expected) -> float:
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())
