"""Logit rows built for the top-N select of hyd_token_logprobs (csrc/token_logprob.hip), shared by
tests/test_scoring_stress.py (a host classifier asserts, without a device, which path of the select every case takes) and
tests/test_scoring_stress_gpu.py (the kernel against the float64 definition of hydragen_amd/scoring.py on these rows and on the
samplers' rows of tests/sampling_stress_cases.py).

The select narrows the N-th largest (value, index) in four ways: every valid logit is a candidate ("all"); the distance-to-max
histogram's crossing bin and the bins above it hold at most 1024 logits ("bin"); radix levels over the key inside that bin
("key"); radix levels over the index among more than 1024 logits tied at the N-th key ("index").  `randn * 3` takes the "bin"
path with a few dozen candidates, and the hand-made rows of tests/test_scoring_gpu.py reach "index" only with no logit above the
tie and a cut below index 256 (tests/test_scoring_stress.py keeps that on record).  The patterns here put a chosen structure at
the N-th value:

  tie_cut           `a` logits above a tie group on a FIXED index set: the cut falls into every index byte, the count carried
                    between the index levels is non-zero, and N - a, not N, ties are taken
  capacity          1023 / 1024 / 1025 candidates at the bin stage and at the key stage: a full LDS buffer, and one more
  close_keys        fp32 keys that differ in their last two bytes only
  spike_flat        one logit 40 above a flat row: the N-th value lies in distance bin 255, under thousands of ties
  signed_zero_wide  a tie group at the maximum that exists only because -0 and +0 are one value
  negative_ties     a tie group of negative values (inverted keys) below one logit

Every row is built on the CPU from its name's seed in the case's dtype (so every value is exact there); rows of one case are
independent re-draws or permutations, so the threads, waves and loop trips that own the decisive columns vary.  A case states the
N values it is built for (`ns`) and what the select must do at each (`expect`): the path, and where they are decisive the crossing
bin, the candidate count, the number of logits above the tie and the cut index (`cut`, or `tie`: the cut is the (N - above)-th
lowest index holding that value, which moves with the row's permutation)."""
from __future__ import annotations

import numpy as np
import torch

from tests.sampling_stress_cases import DT, _permuted, _rng, _round, _strided, on_device, pad_of  # noqa: F401 (on_device: re-export)

KCAP = 1024  # candidates the select may gather (LDS slots)
COMMON_NS = (0, 1, 2, 5, 19, 20)  # every case runs these and its own `ns`

TIE_S_128K = [5, 300, 65543, 66305] + [70000 + 3 * j for j in range(1500)]  # index bytes (0,0,5) (0,1,44) (1,0,7) (1,3,1) (1,17,112)...
TIE_S_256K = [9, 131585] + [200000 + 5 * j for j in range(1200)]            # top index byte 0, 2 and 3


def _tie_cut(dtype, n, a, S, rows, pad, ks=(1, 2, 3, 4, 5)):
    return dict(pattern="tie_cut", n=n, dtype=dtype, rows=rows, pad=pad, a=a, S=S, ks=ks)  # ks: the N - a that are cases of their own


def _cases():
    c = {}
    for dt in ("bf16", "f32"):
        for a in (0, 1, 4):
            c[f"tie_cut_{dt}_a{a}"] = _tie_cut(dt, 128256, a, TIE_S_128K, 8, "vec")
    c["tie_cut_f16_256k_strided"] = _tie_cut("f16", 262147, 2, TIE_S_256K, 6, "odd", ks=(1, 2, 3))
    for dt in ("bf16", "f16", "f32"):
        for cnt in (KCAP - 1, KCAP, KCAP + 1):
            c[f"capacity_bin{cnt}_{dt}"] = dict(pattern="capacity_bin", n=8221, dtype=dt, rows=12, pad="vec", cnt=cnt)
        for t in (KCAP - 4, KCAP - 3):
            c[f"capacity_key{t}_{dt}"] = dict(pattern="capacity_key", n=8221, dtype=dt, rows=12, pad="odd" if dt == "f16" else "vec", t=t)
    c["close_keys_f32"] = dict(pattern="close_keys", n=8221, dtype="f32", rows=12, pad="vec")
    c["spike_flat_bf16_2049"] = dict(pattern="spike_flat", n=2049, dtype="bf16", rows=24, pad="vec")
    c["spike_flat_f16_600"] = dict(pattern="spike_flat", n=600, dtype="f16", rows=24, pad="vec")
    c["signed_zero_wide_bf16"] = dict(pattern="signed_zero_wide", n=8221, dtype="bf16", rows=12, pad="vec")
    c["signed_zero_wide_f32_strided"] = dict(pattern="signed_zero_wide", n=8221, dtype="f32", rows=12, pad="odd")
    c["negative_ties_f16"] = dict(pattern="negative_ties", n=8221, dtype="f16", rows=12, pad="vec")
    c["negative_ties_f32_strided"] = dict(pattern="negative_ties", n=8221, dtype="f32", rows=12, pad="odd")
    return c


CASES = _cases()


# ---- the patterns: (spec, rng) -> (x [rows, n] in the case's dtype, ns, expect {N: dict}) ---------------------------------------------
def tie_cut(c, rng):
    """`a` head columns on the grid 4.0, 3.5, ... at random positions off S, 1.0 on the index set S (more than 1024 columns), uniform
    [-9, 0.5] elsewhere.  With N - a = k the cut is the k-th index of S: one per value of every index byte for k = 1..5, and deep
    inside the run of S for N = 20."""
    rows, n, a, S = c["rows"], c["n"], c["a"], np.asarray(c["S"])
    assert len(S) > KCAP and S.max() < n and (np.diff(S) > 0).all()
    x = rng.uniform(-9.0, 0.5, (rows, n))
    x[:, S] = 1.0
    free = np.setdiff1d(np.arange(n), S)
    for r in range(rows):
        x[r, rng.choice(free, a, replace=False)] = 4.0 - 0.5 * np.arange(a)
    ns = sorted({a + k for k in c["ks"]} | {20})
    expect = {N: dict(path="index", above=a, cut=int(S[N - a - 1]), count=N) for N in ns}
    return _round(x, c["dtype"]), ns, expect


def capacity_bin(c, rng):
    """`cnt` logits within 1/8 of the maximum 4.0 (distance bin 0), everything else 2.9 and below: the bin stage sees exactly cnt
    candidates.  1024 fills the buffer; 1025 is one too many and goes to the key levels."""
    n, cnt = c["n"], c["cnt"]
    base = rng.uniform(-9.0, 2.9, n)
    base[:cnt] = rng.uniform(3.9, 4.0, cnt)
    base[0] = 4.0
    base_t = _round(base, c["dtype"])
    assert int((base_t.double() > 3.875).sum()) == cnt and float(base_t.double()[cnt:].max()) < 3.0
    e = dict(path="bin", bin=0, count=cnt) if cnt <= KCAP else dict(path="key", bin=0)
    return _permuted(base_t, c["rows"], rng), [5, 20], {5: e, 20: e}


CAP_TIE = 3.96875


def capacity_key(c, rng):
    """Two tied pairs (4.0, 4.0, 3.984375, 3.984375) over `t` ties at 3.96875 and 3000 logits at 3.953125, all in distance bin 0:
    at N = 5 and 20 the N-th key is the tie's.  4 + 1020 candidates fill the buffer on the key path; 4 + 1021 go to the index levels
    with four logits above the tie."""
    n, t = c["n"], c["t"]
    base = rng.uniform(-9.0, 2.9, n)
    base[:4] = [4.0, 4.0, 3.984375, 3.984375]
    base[4 : 4 + t] = CAP_TIE
    base[4 + t : 3004 + t] = 3.953125
    base_t = _round(base, c["dtype"])
    assert int((base_t.double() == CAP_TIE).sum()) == t and int((base_t.double() == 3.953125).sum()) == 3000
    if 4 + t <= KCAP:
        expect = {N: dict(path="key", bin=0, above=4, count=4 + t) for N in (5, 20)}
    else:
        expect = {N: dict(path="index", bin=0, above=4, tie=CAP_TIE, count=N) for N in (5, 20)}
    return _permuted(base_t, c["rows"], rng), [5, 20], expect


def close_keys(c, rng):
    """5000 columns hold 4 - j 2^-22, j < 5000 (consecutive fp32 values below 4.0: keys 0x407fffff down, apart from 4.0 itself equal in
    their first two bytes), the rest 2 and below: the N-th key is told apart by the third and fourth radix levels alone."""
    n = c["n"]
    base = rng.uniform(-9.0, 2.0, n)
    base[:5000] = 4.0 - np.arange(5000) * 2.0 ** -22
    base_t = _round(base, c["dtype"])
    assert torch.unique(base_t[:5000]).numel() == 5000 and torch.equal(base_t[:5000].double(), torch.from_numpy(base[:5000]))
    ns = [1, 2, 5, 19, 20]
    return _permuted(base_t, c["rows"], rng), ns, {N: dict(path="key", bin=0, above=N - 1, count=N) for N in ns}


def spike_flat(c, rng):
    """One column at 40.0 over zeros: the zeros lie in distance bin 255 (counted as the valid logits less the other bins).  n = 2049:
    more than 1024 of them, so N >= 2 walks the key levels INSIDE bin 255 and cuts the tie by index with one logit above it.
    n = 600: bin 255 and the spike are 600 candidates, taken by the bin stage."""
    rows, n = c["rows"], c["n"]
    x = np.zeros((rows, n))
    x[np.arange(rows), rng.choice(n, rows, replace=n < rows)] = 40.0
    ns = [1, 2, 5, 20]
    expect = {1: dict(path="bin", bin=0, count=1)}
    for N in ns[1:]:
        expect[N] = dict(path="index", bin=255, above=1, tie=0.0, count=N) if n > KCAP else dict(path="bin", bin=255, count=n)
    return _round(x, c["dtype"]), ns, expect


def signed_zero_wide(c, rng):
    """3000 columns at +0 / -0 (alternating) over a background in [-9, -1]: the maximum is a tie group of 3000 only because the two
    zeros are one value (one key); the cut by index is the N-th zero of either sign."""
    n = c["n"]
    base = rng.uniform(-9.0, -1.0, n)
    base[:3000] = 0.0
    base[:3000:2] = -0.0
    base_t = _round(base, c["dtype"])
    assert int(torch.signbit(base_t[:3000]).sum()) == 1500
    ns = [1, 2, 5, 20]
    return _permuted(base_t, c["rows"], rng), ns, {N: dict(path="index", bin=0, above=0, tie=0.0, count=N) for N in ns}


def negative_ties(c, rng):
    """-29.5 over 2000 columns at -30.0 over a background in [-45, -31]: the radix levels run on the inverted keys of negative
    values, and the index cut takes N - 1 of the ties."""
    n = c["n"]
    base = rng.uniform(-45.0, -31.0, n)
    base[0] = -29.5
    base[1:2001] = -30.0
    base_t = _round(base, c["dtype"])
    assert int((base_t.double() == -30.0).sum()) == 2000
    ns = [1, 2, 5, 20]
    expect = {1: dict(path="bin", bin=0, count=1)}
    expect.update({N: dict(path="index", bin=4, above=1, tie=-30.0, count=N) for N in ns[1:]})
    return _permuted(base_t, c["rows"], rng), ns, expect


PATTERNS = dict(tie_cut=tie_cut, capacity_bin=capacity_bin, capacity_key=capacity_key, close_keys=close_keys, spike_flat=spike_flat,
                signed_zero_wide=signed_zero_wide, negative_ties=negative_ties)


def build(name: str) -> dict:
    """-> dict(x [rows, n] CPU tensor in the case's dtype (a strided view where pad > 0), ns, expect, pattern, name, n, dtype, pad)"""
    c = CASES[name]
    assert c["rows"] <= 24
    pad = pad_of(c["n"], c["pad"])
    x, ns, expect = PATTERNS[c["pattern"]](c, _rng(name))
    assert x.shape == (c["rows"], c["n"]) and x.dtype == DT[c["dtype"]] and set(ns) == set(expect)
    return dict(x=_strided(x, pad, c["dtype"]), ns=ns, expect=expect, pattern=c["pattern"], name=name, n=c["n"], dtype=c["dtype"], pad=pad)
