"""-m "not gpu": the conditions that keep tests/test_sampling_stress_gpu.py honest, checked without a device.

  * the host mirror (tests/sampler_mirror.py) is Philox4x32-10 (the published known-answer vectors) and its uniform variate is the
    kernels' (tests/test_sampler_noise._u);
  * on every (case, cut) of tests/sampling_stress_cases.py the float64 definition's kept count does not move when top_p / min_p
    move by SLACK, so the GPU test may demand equality; and the patterns hit what they claim (bin 255, underflow, plateaus, ...);
  * on the mirror-draw rows at most 1 % of the rows have a margin in (0, EPS]: the comparison is conclusive nearly everywhere;
  * the mutations the GPU tests are meant to catch change the mirror's tokens (a swapped Philox word order, a dropped high half
    of the offset or seed, the highest instead of the lowest tied index);
  * the chi-square / Poisson thresholds hard-coded beside their parameters are the 1 - 1e-6 quantiles."""
import math

import numpy as np
import pytest
import torch

from hydragen_amd import sampling
from tests import sampler_mirror as M
from tests import sampling_stress_cases as C
from tests.test_sampler_noise import _u


def test_philox_known_answer_vectors():
    # Random123 kat_vectors, philox4x32 10 rounds
    assert [int(w) for w in M.philox4x32_10((0, 0, 0, 0), (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(w) for w in M.philox4x32_10((f, f, f, f), (f, f))] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised calls equal one call per counter
    ctr = (np.arange(5, dtype=np.uint64)[None, :], np.arange(3, dtype=np.uint64)[:, None], 7, 9)
    many = M.philox4x32_10(ctr, (11, 13))
    for r in range(3):
        for c in range(5):
            assert [int(w[r, c]) for w in many] == [int(w) for w in M.philox4x32_10((c, r, 7, 9), (11, 13))]


def test_mirror_uniform_is_the_kernels_and_the_noise_is_bounded():
    edge = np.array([0, 1, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.uint32)
    rnd = np.random.default_rng(1).integers(0, 2 ** 32, size=1 << 18, dtype=np.uint64).astype(np.uint32)
    for bits in (edge, rnd):
        assert np.array_equal(M.uniform(bits), _u(bits).astype(np.float64))
        g = M.gumbel(bits)
        assert (g >= M.G_MIN).all() and (g <= M.G_MAX).all()
    assert M.G_MAX - M.G_MIN < 20.3  # what the decisive-logit test of the GPU file rests on
    # layout: column j of row r is word j % 4 of the call with counter (j // 4, r, offset lo, offset hi), key (seed lo, seed hi)
    seed, off = C.MIRROR_KEY
    g, k = M.noise(np.array([0, 5]), 11, seed, off)
    for r, row in enumerate((0, 5)):
        for j in range(11):
            w = M.philox4x32_10((j // 4, row, off & 0xFFFFFFFF, off >> 32), (seed & 0xFFFFFFFF, seed >> 32))[j % 4]
            assert int(k[r, j]) == int(w) >> 9 and g[r, j] == M.gumbel(np.uint32(int(w)))


def _counts(xd, top_k, top_p, min_p):
    """Kept counts of the definition with every threshold tightened / at its value / loosened by SLACK
    (tests/test_sampling_filters_gpu.py `_bounds`)."""
    def cnt(tp, mp):
        return sampling.kept_mask(xd, top_k, tp, mp).sum(-1)
    tp_lo = None if top_p is None else max(top_p - C.SLACK, 1e-6)
    tp_hi = None if top_p is None else min(top_p + C.SLACK, 1.0)
    mp_lo = None if min_p is None else min(min_p + C.SLACK, 1.0)
    mp_hi = None if min_p is None else max(min_p - C.SLACK, 0.0)
    return cnt(tp_lo, mp_lo), cnt(top_p, min_p), cnt(tp_hi, mp_hi)


def _kth_distance(row, k):
    """max - the k-th largest valid value of a float64 row"""
    v = row[~np.isnan(row) & (row != -np.inf)]
    return v.max() - np.sort(v)[-k]


@pytest.mark.parametrize("name", list(C.CASES))
def test_select_is_exact_and_the_pattern_is_what_it_claims(name):
    case = C.build(name)
    x, info, pattern, n = case["x"], case["info"], case["pattern"], case["n"]
    stride = x.stride(0) if x.shape[0] > 1 else n
    assert stride == n + case["pad"] and (stride % 2 == 1 if C.CASES[name]["pad"] == "odd" else stride % 8 == 0 or n <= 16)
    xd = x.double()
    X = xd.numpy()
    assert len(case["cuts"]) >= 4
    kinds = set()
    for top_k, top_p, min_p in case["cuts"]:
        kinds.add((bool(top_k), top_p is not None, min_p is not None))
        lo, exact, hi = _counts(xd, top_k, top_p, min_p)
        assert torch.equal(lo, exact) and torch.equal(hi, exact), (name, top_k, top_p, min_p, lo, exact, hi)
        assert (exact >= 1).all()
    assert {(True, False, False), (False, True, False), (False, False, True)} <= kinds and len(kinds) >= 4  # each alone + a combination

    valid = ~np.isnan(X) & (X != -np.inf)
    if pattern == "far_tail":
        for r, h in enumerate(info["heads"]):
            assert _kth_distance(X[r], info["top_k"]) >= 31.875 and _kth_distance(X[r], h) <= 2.0 and _kth_distance(X[r], h + 1) >= 31.875
    elif pattern == "underflow":
        d = X.max(-1, keepdims=True) - X
        units = np.exp(-d) * 2.0 ** 40  # fixed-point mass
        small = (d >= 19.5) & (d <= 27.75)
        assert (small.sum(-1) >= 99000).all() and ((units < 1.0).sum(-1) >= 20000).all()
        assert units[small].max() < 4000 and units[small].min() > 0.9
        share = np.where(small, np.exp(-d), 0.0).sum(-1) / np.exp(-d).sum(-1)
        assert (share > 2 * C.ROOM).all()  # together they matter: more than the room the cuts keep
        # the top_p cut keeps 2 columns with the small masses and would keep 1 without them
        top_p = case["cuts"][1][1]
        assert (sampling.kept_mask(xd, None, top_p, None).sum(-1) == 2).all()
        assert (sampling.kept_mask(xd.masked_fill(torch.from_numpy(small), -math.inf), None, top_p, None).sum(-1) == 1).all()
    elif pattern == "plateau":
        v, k = info["value"], info["above"] + 1
        for r in range(X.shape[0]):
            assert (X[r] == v).sum() == info["width"] and (X[r] > v).sum() == info["above"] and np.sort(X[r])[-k] == v
        if C.CASES[name].get("signed_zero"):
            sign = np.signbit(X) & (X == 0)
            assert (sign.sum(-1) >= 2).all() and (((X == 0) & ~sign).sum(-1) >= 2).all()  # both zeros on the plateau
        if name.startswith("all_negative"):
            assert (X < 0).all()
        for top_k, top_p, min_p in case["cuts"]:
            assert (sampling.kept_mask(xd, top_k, top_p, min_p).sum(-1) == info["above"] + info["width"]).all()
    elif pattern == "flat":
        assert (X == X[:, :1]).all()
        for top_k, top_p, min_p in case["cuts"]:
            assert (sampling.kept_mask(xd, top_k, top_p, min_p).sum(-1) == n).all()
    elif pattern == "few_valid":
        assert valid.sum(-1).tolist() == info["nvalid"] and set(info["nvalid"]) == {1, info["top_k"] - 1, info["top_k"], info["top_k"] + 1}
        assert np.isnan(X).any() and (X == -np.inf).any()
    elif pattern == "pos_inf":
        assert (X == np.inf).sum(-1).tolist() == info["ninf"] and set(info["ninf"]) == {1, 3}
    elif pattern == "extreme":
        big = float(C._round(np.full(1, C.MAX_FINITE[case["dtype"]]), case["dtype"]).double())
        assert math.isfinite(big) and ((X == big).sum(-1) == 2).all() and ((X == -big).sum(-1) == 3).all()
        assert (np.sort(X, -1)[:, -5:-2] < big).all() and (_kth_distance(X[0], 4) >= 31.875)
    elif pattern == "denormal":
        smallest_normal = {"bf16": 2.0 ** -126, "f16": 2.0 ** -14, "f32": 2.0 ** -126}[case["dtype"]]
        assert (np.abs(X) <= smallest_normal).all() and len(np.unique(X[0])) == 2 * info["J"] + 1
    elif pattern == "n_le_top_k":
        assert all(k is None or k >= n for k, _, _ in case["cuts"])


def _mirror_census(V, pad, dtype, T):
    x = C.mirror_rows(V, pad, dtype).double().numpy()
    win, margin, lowest = M.mirror_draw(x, T, *C.MIRROR_KEY)
    e = M.eps(M.max_abs(x), T)
    return win, margin, lowest, e


@pytest.mark.parametrize("V, pad", C.MIRROR_SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_mirror_is_mostly_conclusive(V, pad, dtype):
    for T in C.MIRROR_TEMPERATURES:
        win, margin, lowest, e = _mirror_census(V, pad, dtype, T)
        assert e < 5e-5  # EPS for |logit| <= 16 at T >= 0.7: sampler_mirror's docstring
        unsure = int(((margin > 0) & (margin <= e)).sum())
        assert unsure <= 0.01 * len(win), (unsure, float(margin.min()))
        assert np.array_equal(win, lowest)


def test_flat_rows_tie_on_k_and_the_lowest_index_is_expected():
    n, rows = C.UNIFORM_V, C.FLAT_ROWS
    lowest, highest = M.flat_row_tokens(rows, n, *C.MIRROR_KEY)
    win, margin, low = M.mirror_draw(np.zeros((256, n)), 1.0, *C.MIRROR_KEY)
    assert np.array_equal(win, lowest[:256]) and np.array_equal(low, lowest[:256])  # g is increasing in k: the largest k wins
    tied = lowest != highest
    # exact ties exist (about n / 2^23 of the rows) and are not excluded: `oi < besti` turned into `oi > besti` changes these rows
    # (and every flat, plateau-of-the-maximum and +inf row of the stress cases at T = 0)
    assert 1 <= tied.sum() < 0.02 * rows


def test_the_targeted_faults_change_the_mirrors_tokens():
    """What the GPU tests compare against moves under each one-line fault on a quarter of the rows and more (not on all: the draw
    is peaked at T = 0.7, and a word swap leaves half of the columns their noise); the GPU test demands every conclusive row, so a
    kernel with the fault cannot pass it."""
    V, pad = C.MIRROR_SHAPES[0]
    x = C.mirror_rows(V, pad, "bf16").double().numpy()
    seed, off = C.MIRROR_KEY
    base = M.mirror_draw(x, 0.7, seed, off)[0]
    rows = len(base)
    swapped = M.mirror_draw(x, 0.7, seed, off, word_order=(1, 0, 2, 3))[0]
    assert (swapped != base).mean() > 0.25
    assert (M.mirror_draw(x, 0.7, seed, off & 0xFFFFFFFF)[0] != base).mean() > 0.25  # `offset >> 32` dropped
    assert (M.mirror_draw(x, 0.7, seed & 0xFFFFFFFF, off)[0] != base).mean() > 0.25  # `seed >> 32` dropped
    for s, o in C.KEY_VARIANTS:  # one 32-bit half each
        assert (s != seed) + (o != off) == 1 and bin((s ^ seed) | (o ^ off)).count("1") == 1
        assert (M.mirror_draw(x, 0.7, s, o)[0] != base).mean() > 0.25


def test_thresholds_are_the_quantiles():
    stats = pytest.importorskip("scipy.stats")
    for dof, q in C.CHI2_Q.items():
        assert abs(stats.chi2.isf(1e-6, dof) - q) < 1e-5
    for mean, q in C.POISSON_Q.items():
        assert stats.poisson.isf(1e-6, mean) == q  # P(X > q) <= 1e-6
