"""-m gpu: hyd_token_logprobs (csrc/token_logprob.hip) on rows built for its top-N select (tests/scoring_stress_cases.py: what each
pattern pins; tests/test_scoring_stress.py asserts without a device that every case takes the path it is named for) and on the
samplers' adversarial rows (tests/sampling_stress_cases.py, +inf rows included: hydragen_amd/scoring.py defines them), against the
float64 definition on the same bits.

No row and no column is left out: the composite (value, index) is unique, so `top_ids` and `greedy` are compared exactly, NaN and
+-inf must sit where the definition puts them, and every finite log-prob lies within TOL(want) = 1e-5 + 2^-23 |want|:

  * a mass is floor(exp2((l - m) log2e) 2^40), non-zero only for m - l < 27.73.  The fp32 product (l - m) log2e is rounded once:
    its error moves the mass by at most 27.73 log2e 2^-24 ln2 = 1.7e-6 relative.  The hardware exp2 (v_exp_f32) is specified to
    1 ulp, 1.2e-7.  Truncation to a whole unit and masses below one unit lose at most 2 n 2^-40 = 5e-7 of the sum at n = 2^18 (the
    maximum alone weighs 2^40).  So |ln sum - float64| <= 2.3e-6, and l - m is exact in double: 1e-5, the bar of
    tests/test_scoring_gpu.py, holds with a factor of 4 to spare;
  * 2^-23 |want| is two half-ulps: kernel and definition each round a double to fp32 once (the types' extremes: |log-prob| 2^120).

The worst |log-prob - float64| of every case is printed (profiles/scoring.md keeps the table)."""
import math

import pytest
import torch

from hydragen_amd import layer_ops, scoring
from tests import sampling_stress_cases as SC
from tests import scoring_stress_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_CASES = [("scoring", k) for k in C.CASES] + [("sampling", k) for k in SC.CASES]
KINDS = 9  # target kinds of `_target_sets`


def _same(a, b):
    """Bitwise equal, NaN where the other has NaN."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a[~a.isnan()], b[~b.isnan()])


def _target_sets(xc):
    """KINDS target vectors [rows] for the CPU rows xc.  Each row has a list of the targets it can have -- the lowest-index maximum,
    the highest-index column tied with it, a NaN, a -inf, a +inf and a -0 column where the row has one, column n - 1, -1 and n
    (padding) -- and takes them in turn: set k gives row r entry (r + k) of its list, so the KINDS sets give every row each of its
    targets.  -> (sets, tied [rows] bool: the row has more than one maximum, last_max [rows]: the highest-index one)"""
    rows, n = xc.shape
    xd = xc.double()
    lists, tied = [], []
    for r in range(rows):
        v = xd[r]
        ok = ~(v.isnan() | (v == -math.inf))
        at_max = torch.nonzero(ok & (v == v[ok].max()))[:, 0].tolist() if ok.any() else [0]
        own = [at_max[0], at_max[-1]]
        for mask in (v.isnan(), v == -math.inf, v == math.inf, (v == 0) & torch.signbit(v)):
            where = torch.nonzero(mask)[:, 0]
            if len(where):
                own.append(int(where[len(where) // 2]))
        lists.append(own + [n - 1, -1, n])
        tied.append(len(at_max) > 1)
    sets = [torch.tensor([own[(r + k) % len(own)] for r, own in enumerate(lists)]) for k in range(KINDS)]
    last_max = torch.tensor([own[1] for own in lists])
    return sets, torch.tensor(tied), last_max


def _compare(got, want, where):
    """Everything equal as the module docstring says; -> (the largest |log-prob - float64|, the largest share of TOL used)"""
    lp, greedy, ids, tlp = (g.cpu() for g in got)
    rlp, rgreedy, rids, rtlp = want
    assert lp.shape == rlp.shape and ids.shape == rids.shape == tlp.shape and greedy.dtype == torch.bool, where
    assert torch.equal(ids, rids), (where, torch.nonzero(ids != rids)[:8].tolist())
    assert torch.equal(greedy, rgreedy), (where, greedy, rgreedy)
    worst = share = 0.0
    for a, b in ((lp, rlp), (tlp, rtlp)):
        a, b = a.double(), b.double()
        assert torch.equal(a.isnan(), b.isnan()), where
        assert torch.equal(a == math.inf, b == math.inf) and torch.equal(a == -math.inf, b == -math.inf), where
        fin = torch.isfinite(b)
        if fin.any():
            diff, tol = (a[fin] - b[fin]).abs(), 1e-5 + 2.0 ** -23 * b[fin].abs()
            worst, share = max(worst, diff.max().item()), max(share, (diff / tol).max().item())
            assert (diff <= tol).all(), (where, diff.max().item(), (diff / tol).max().item())
    return worst, share


@pytest.mark.parametrize("lib, name", ALL_CASES)
def test_kernel_equals_the_definition_on_adversarial_rows(lib, name):
    built = (C if lib == "scoring" else SC).build(name)
    xc, n = built["x"], built["n"]
    x = SC.on_device(xc, built["dtype"], DEV)
    rows = x.shape[0]
    assert (x.stride(0) if rows > 1 else n) == n + built["pad"]
    ns = sorted(set(C.COMMON_NS) | set(built.get("ns", ())))
    sets, tied, last_max = _target_sets(xc)
    worst = share = 0.0
    for i in range(max(len(ns), KINDS)):  # every N and every target set at least once
        N, tc = ns[i % len(ns)], sets[i % KINDS]
        t = tc.to(DEV)
        got = layer_ops.token_logprobs(x, t, N)
        w, s = _compare(got, scoring.token_logprobs_reference(xc, tc, N), (name, N, i))
        worst, share = max(worst, w), max(share, s)
        # a target on a later column of a tied maximum is not the greedy token
        later = tied & (tc == last_max)
        assert not got[1].cpu()[later].any(), (name, N, i)
        if N > 0:  # N = 0 is another instantiation: the same log-probs and flags
            n0 = layer_ops.token_logprobs(x, t, 0)
            assert _same(n0[0], got[0]) and _same(n0[1], got[1]), (name, N, i)
    # a row launched alone gives the bits it gives in the batch
    t = sets[0].to(DEV)
    full = layer_ops.token_logprobs(x, t, 20)
    for r in sorted({0, min(1, rows - 1), rows - 1}):
        one = layer_ops.token_logprobs(x[r : r + 1], t[r : r + 1], 20)
        for a, b in zip(full, one):
            assert _same(a[r : r + 1], b), (name, r)
    # the log-prob of a drawn token is the sampler's, bit for bit
    if built["pattern"] not in SC.HAS_POS_INF:
        top_k, top_p, min_p = built["cuts"][0] if "cuts" in built else (None, None, None)
        tok, slp, _ = layer_ops.sample_tokens_filtered(x, 1.0, key=(3, 40), top_k=top_k, top_p=top_p, min_p=min_p)
        for N in (0, 20):
            assert _same(layer_ops.token_logprobs(x, tok[:, 0], N)[0], slp), (name, N)
    print(f"{name}: N in {ns}, {KINDS} target sets: largest |log-prob - float64| = {worst:.3g} ({share:.3f} of the bound)")
