"""-m "not gpu": what tests/test_scoring_stress_gpu.py rests on, checked without a device.

  1. `classify`: DESIGN.md 4.12's narrowing of the N-th largest (value, index), restated in counts alone -- which of the four paths
     a row takes at a given N, with how many candidates, through which distance bin, with how many logits above the tie and where
     the index cut falls.  Every case of tests/scoring_stress_cases.py takes the path it is named for, on every row.
  2. The hand-made rows of tests/test_scoring_gpu.py (`_rows`, drawn here on the CPU from the same text) reach the index path
     only with nothing above the tie and a cut below index 256: the gap the new cases close, kept on record.
  3. `scoring.token_logprobs_reference` -- the reference of every device test -- against a per-row ranking in plain Python
     (sorted (-value, index), math.fsum) on the new cases and on the samplers' cases."""
import math

import numpy as np
import pytest
import torch

from hydragen_amd import scoring
from tests import sampling_stress_cases as SC
from tests import scoring_stress_cases as C


# ---- 1. the host classifier ----------------------------------------------------------------------------------------------------------
def classify(row: torch.Tensor, N: int) -> dict:
    """The select of DESIGN.md 4.12 for one row (a 1-D tensor in its own dtype) and N >= 1, as counts:
      path   "all"   no more than N valid logits (neither NaN nor -inf): all of them are candidates;
             "bin"   the distance-to-max bin that holds the N-th largest value, and the bins above it, hold <= 1024 logits;
             "key"   else, the N-th largest value and the values above it occur <= 1024 times;
             "index" else: the logits above the N-th value, and the lowest-index N - above of those equal to it;
      count  the candidates;  bin  the crossing bin;  above  the valid logits above the N-th value;  cut  the last index taken
             on the index path.
    Bins are fp32 arithmetic on the logits as fp32: d = max - l (0 where l == max), bin = int(8 d) below 31.875, else 255.
    +0 and -0 are one value: every comparison here is on values."""
    v = row.float().numpy()
    ok = ~np.isnan(v) & (v != -np.inf)
    idx = np.flatnonzero(ok)
    v = v[ok]
    if v.size <= N:
        return dict(path="all", count=int(v.size), bin=None, above=None, cut=None)
    m = v.max()
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(v == m, np.float32(0), m - v).astype(np.float32)
        bins = np.where(d < np.float32(31.875), (d * np.float32(8)).astype(np.int64), 255)
    per_bin = np.bincount(bins, minlength=256)
    upto = np.cumsum(per_bin)
    b = int(np.searchsorted(upto, N))  # the first bin with upto >= N
    nth = np.sort(v)[-N]
    above, ties = int((v > nth).sum()), int((v == nth).sum())
    out = dict(bin=b, above=above, cut=None)
    if upto[b] <= C.KCAP:
        return dict(out, path="bin", count=int(upto[b]))
    if above + ties <= C.KCAP:
        return dict(out, path="key", count=above + ties)
    return dict(out, path="index", count=N, cut=int(idx[v == nth][N - above - 1]))


def test_classifier_on_hand_made_rows():
    f = torch.tensor
    assert classify(f([1.0, float("nan"), -math.inf, 2.0]), 2)["path"] == "all"
    got = classify(f([0.0, 3.0, 2.95, 1.0, -40.0]), 2)
    assert (got["path"], got["bin"], got["count"], got["above"]) == ("bin", 0, 2, 1)
    assert classify(f([0.0, 3.0, 2.95, 1.0, -40.0]), 4)["bin"] == 24 and classify(f([0.0, 3.0, 2.95, 1.0, -40.0, -50.0]), 5)["bin"] == 255
    assert classify(f([0.0, 3.0, 2.95, 1.0, -40.0]), 5) == dict(path="all", count=5, bin=None, above=None, cut=None)
    wide = torch.cat([f([5.0, 0.9]), torch.full((2000,), 0.9), f([0.95])])  # 2001 ties and 0.95 in one bin: 4.05 and 4.1 below 5.0
    assert classify(wide, 1)["path"] == "bin"
    got = classify(wide, 2)
    assert (got["path"], got["count"], got["above"]) == ("key", 2, 1)
    got = classify(wide, 4)
    assert (got["path"], got["count"], got["above"], got["cut"], got["bin"]) == ("index", 4, 2, 2, 32)
    zeros = torch.zeros(3000)
    zeros[::2] = -0.0
    assert classify(zeros, 7) == dict(path="index", count=7, bin=0, above=0, cut=6)


@pytest.fixture(scope="module", params=list(C.CASES))
def case(request):
    return C.build(request.param)


def test_every_case_takes_the_path_it_is_named_for(case):
    x = case["x"]
    for N in case["ns"]:
        cuts = set()
        want = case["expect"][N]
        for r in range(x.shape[0]):
            got = classify(x[r], N)
            where = (case["name"], N, r, got)
            assert got["path"] == want["path"], where
            for k in ("bin", "count", "above", "cut"):
                if k in want:
                    assert got[k] == want[k], where
            if "tie" in want:  # the cut moves with the row: the (N - above)-th lowest index that holds the tie's value
                held = torch.nonzero(x[r].double() == want["tie"])[:, 0]
                assert want["above"] + len(held) > C.KCAP and got["cut"] == int(held[N - want["above"] - 1]), where
                cuts.add(got["cut"])
        # permuted rows put the cut in different places (spike_flat moves the spike, not the ties)
        assert not cuts or len(cuts) > 1 or case["pattern"] == "spike_flat", (case["name"], N, cuts)


def test_the_tie_cut_cases_put_a_cut_in_every_index_byte():
    cuts = {name: sorted(e["cut"] for e in C.build(name)["expect"].values()) for name in C.CASES if name.startswith("tie_cut")}
    small = cuts["tie_cut_bf16_a1"]
    assert small[:5] == [5, 300, 65543, 66305, 70000] and small[5] == 70000 + 3 * (20 - 1 - 5)
    assert {c >> 16 for c in small} == {0, 1} and {(c >> 8) & 255 for c in small[:4]} == {0, 1, 3} and small[2] & 255 == 7
    big = cuts["tie_cut_f16_256k_strided"]
    assert big[:3] == [9, 131585, 200000] and {c >> 16 for c in big} == {0, 2, 3}
    # the count carried from one index level to the next is non-zero: ties lie under a smaller first byte, and first two bytes
    S = np.asarray(C.TIE_S_128K)
    into_2nd = [int((S >> 16 < cut >> 16).sum()) for cut in small]
    into_3rd = [int((S >> 8 < cut >> 8).sum()) for cut in small]
    assert into_2nd == [0, 0, 2, 2, 2, 2] and into_3rd == [0, 1, 2, 3, 4, 4]


# ---- 2. the rows the device tests had ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V, pad", [(32000, 0), (128256, 0)])
def test_the_existing_rows_reach_the_index_path_only_without_a_logit_above_and_below_index_256(monkeypatch, dtype, V, pad):
    from tests import test_scoring_gpu as G

    monkeypatch.setattr(G, "DEV", "cpu")  # the same recipe, drawn by the CPU generator
    x = G._rows(48, V, dtype, seed=V + pad, pad=pad)
    paths = {}
    for N in (1, 5, 20):
        for r in range(x.shape[0]):
            got = classify(x[r], N)
            paths.setdefault(got["path"], []).append(got)
            if got["path"] == "index":
                assert got["above"] == 0 and got["cut"] < 256, (r, N, got)
    assert "index" in paths and "key" in paths and "bin" in paths  # (the recipe does reach every stage: only never decisively)
    assert max(g["count"] for g in paths["key"]) < 64 and all(g["bin"] == 0 for g in paths["key"])
    assert max(g["count"] for g in paths["bin"]) < 64


# ---- 3. the reference against a plain ranking -----------------------------------------------------------------------------------------
def rank_row(row64):
    """The row's ranking, made once: (the valid columns' (-value, index) in order, the maximum, ln of the denominator), or None for a
    row without a valid logit"""
    valid = [(-v, i) for i, v in enumerate(row64) if not math.isnan(v) and v != -math.inf]
    if not valid:
        return None
    ranked = sorted(valid)  # (-value, index): value descending, index ascending; -0.0 == 0.0 as tuples compare by value
    m = -ranked[0][0]
    # the denominator is 1 (the first maximum's own term) + the exactly rounded sum of the others; ln of it through log1p, so that
    # a denominator of 1 + 1e-12 keeps its digits (log(fsum(all)) holds 4 of them: the sum is rounded to 2^-52 first)
    lse = math.log1p(math.fsum(1.0 if -nv == m else math.exp(-nv - m) for nv, _ in ranked[1:]))
    return ranked[: scoring.TOP_LOGPROBS_MAX], m, lse


def brute_force(ranking, row64, target, N):
    """(logprob, greedy, ids [N], logprobs [N]) of the definition (hydragen_amd/scoring.py) for one row of Python floats"""
    if ranking is None:
        return math.nan, False, [-1] * N, [-math.inf] * N
    ranked, m, lse = ranking

    def lp(v):
        return (0.0 if v == m else v - m) - lse

    top = ranked[:N]
    ids = [i for _, i in top] + [-1] * (N - len(top))
    lps = [lp(-nv) for nv, _ in top] + [-math.inf] * (N - len(top))
    if not 0 <= target < len(row64):
        return math.nan, False, ids, lps
    return lp(row64[target]), target == ranked[0][1], ids, lps


def _f32(v):
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def _close(got, want):
    """identical NaN / +-inf; finite values within 1e-12 relative"""
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return math.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)


def _targets_for(row64, r):
    n = len(row64)
    m = max((v for v in row64 if not math.isnan(v)), default=0.0)
    at_max = [i for i, v in enumerate(row64) if v == m]
    return [at_max[0] if at_max else 0, at_max[-1] if at_max else 0, n - 1, -1, n, (7919 * (r + 1)) % n]


ALL_CASES = [("scoring", k) for k in C.CASES] + [("sampling", k) for k in SC.CASES]


@pytest.mark.parametrize("lib, name", ALL_CASES)
def test_reference_equals_a_brute_force_ranking(lib, name):
    built = (C if lib == "scoring" else SC).build(name)
    x = built["x"][:3]
    ns = sorted({1, 5, 20} | set(built.get("ns", ())))
    rows = [x[r].double().tolist() for r in range(x.shape[0])]
    tsets = [_targets_for(row, r) for r, row in enumerate(rows)]
    rankings = [rank_row(row) for row in rows]
    nans = 0
    for k in range(len(tsets[0])):
        t = torch.tensor([ts[k] for ts in tsets])
        for N in ns if k == 0 else ns[-1:]:
            lp, greedy, ids, tlp = scoring.token_logprobs_reference(x, t, N)
            assert ids.shape == tlp.shape == (x.shape[0], N) and lp.dtype == tlp.dtype == torch.float32
            for r, row in enumerate(rows):
                wlp, wgreedy, wids, wtlp = brute_force(rankings[r], row, int(t[r]), N)
                where = (name, N, r, int(t[r]))
                assert ids[r].tolist() == wids, where
                assert bool(greedy[r]) == wgreedy, where
                assert _close(float(lp[r]), _f32(wlp)), (where, float(lp[r]), wlp)
                for j in range(N):
                    assert _close(float(tlp[r, j]), _f32(wtlp[j])), (where, j, float(tlp[r, j]), wtlp[j])
                nans += sum(math.isnan(v) for v in tlp[r].tolist())
    assert nans == 0  # no NaN among the top-N log-probs, +inf and the types' extremes included
