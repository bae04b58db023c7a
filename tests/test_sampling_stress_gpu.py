"""-m gpu: the four sampling launches -- hyd_sample_tokens (csrc/layer_ops.hip), hyd_sample_tokens_filtered (csrc/sample_filter.hip),
hyd_sample_tokens_penalized / hyd_sample_tokens_constrained (csrc/sample_select.h), all on the row primitives of csrc/vocab_row.h --
against an independent host mirror of their noise (tests/sampler_mirror.py) and, on the adversarial rows of tests/sampling_stress_cases.py, against the float64 definition of
the cuts (hydragen_amd/sampling.py).  tests/test_sampling_stress.py checks without a device what these tests rest on.

  1. mirror draws at vocabulary size: the drawn token is the mirror's on every row whose margin exceeds EPS (derived in
     tests/sampler_mirror.py from the probe's record), through all four entry points, with keys that use all four 32-bit halves;
  2. a logit more than 20.3 T above every other one is drawn from every position of the thread / wave / loop-trip layout;
  3. on flat rows the drawn column is uniform over the chunk positions, Philox words, waves and loop trips that own the columns,
     and neighbouring rows / consecutive keys do not repeat each other;
  4. the select on the adversarial rows: kept counts equal the definition's exactly, tokens lie in its kept set, log-probs."""
import functools
import math

import numpy as np
import pytest
import torch

from hydragen_amd import layer_ops, sampling
from hydragen_amd.constraint import TokenDFA
from tests import sampler_mirror as M
from tests import sampling_stress_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("plain", "filtered", "penalized", "constrained")


@functools.lru_cache(maxsize=2)
def _allow_all(V):
    return TokenDFA(torch.zeros((1, V), dtype=torch.int32)).to(DEV)  # one state, every token allowed and leading back to it


def _draw(entry, x, T, key, **cuts):
    """-> (tokens [B] int64, log-probs [B] or None, kept [B] or None) of one entry point"""
    if entry == "plain":
        assert not cuts
        return layer_ops.sample_tokens(x, T, key=key)[:, 0], None, None
    if entry == "filtered":
        tok, lp, kept = layer_ops.sample_tokens_filtered(x, T, key=key, **cuts)
    elif entry == "penalized":
        tok, lp, kept = layer_ops.sample_tokens_penalized(x, T, key=key, penalties=layer_ops.Penalties(), **cuts)
    else:
        state = torch.zeros(x.shape[0], dtype=torch.int32, device=DEV)
        tok, lp, kept = layer_ops.sample_tokens_constrained(x, T, key=key, constraint=(_allow_all(x.shape[1]), state, False), **cuts)
    return tok[:, 0], lp, kept


def _agrees(tok, mirror, e):
    """Token == the mirror's lowest tied winner on every row with margin > e; -> the number of rows not compared (0 < margin <= e)."""
    win, margin, lowest = mirror
    sure = margin > e
    got = tok.cpu().numpy()
    assert np.array_equal(got[sure], lowest[sure]), (np.flatnonzero(sure & (got != lowest)), got[sure & (got != lowest)],
                                                     lowest[sure & (got != lowest)], margin[sure & (got != lowest)])
    return int((~sure).sum())


# ---- 1. mirror draws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V, pad", C.MIRROR_SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_every_entry_point_draws_the_mirrors_token(V, pad, dtype):
    xc = C.mirror_rows(V, pad, dtype)
    x = C.on_device(xc, dtype, DEV)
    assert x.stride(0) == V + pad
    x64 = xc.double().numpy()
    skipped = {}
    for T in C.MIRROR_TEMPERATURES:
        mirror = M.mirror_draw(x64, T, *C.MIRROR_KEY)
        e = M.eps(M.max_abs(x64), T)
        for entry in ENTRIES:
            skipped[T, entry] = _agrees(_draw(entry, x, T, C.MIRROR_KEY)[0], mirror, e)
    print(f"rows not compared (0 < margin <= EPS) of {C.MIRROR_ROWS}: {sorted(set(skipped.values()))}")
    assert max(skipped.values()) <= 0.01 * C.MIRROR_ROWS


@pytest.mark.parametrize("entry", ["plain", "filtered"])
def test_each_half_of_the_key_reaches_the_noise(entry):
    V, pad = C.MIRROR_SHAPES[0]
    xc = C.mirror_rows(V, pad, "bf16")
    x, x64 = C.on_device(xc, "bf16", DEV), xc.double().numpy()
    e = M.eps(M.max_abs(x64), 0.7)
    base = _draw(entry, x, 0.7, C.MIRROR_KEY)[0]
    skipped = 0
    for key in C.KEY_VARIANTS:  # each differs from MIRROR_KEY in one bit of one 32-bit half
        tok = _draw(entry, x, 0.7, key)[0]
        skipped += _agrees(tok, M.mirror_draw(x64, 0.7, *key), e)
        assert (tok != base).float().mean() > 0.25
    print(f"rows not compared: {skipped} of {4 * C.MIRROR_ROWS}")
    assert skipped <= 0.01 * 4 * C.MIRROR_ROWS


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_filtered_draw_is_the_mirrors_winner_over_the_kept_set(dtype):
    V, pad = C.MIRROR_SHAPES[0]
    xc = C.mirror_rows(V, pad, dtype)
    x, xd = C.on_device(xc, dtype, DEV), xc.double()
    x64 = xd.numpy()
    e = M.eps(M.max_abs(x64), 0.7)
    # top_k alone is exact (keys); with top_p the kernel's kept set may differ from float64's by a boundary token on a row in a
    # hundred (tests/test_sampling_filters_gpu.py): such rows are told by their kept count and left out, within the same 1 %
    for cuts, exact in ((dict(top_k=40), True), (dict(top_k=50, top_p=0.9), False), (dict(min_p=0.02), False)):
        keep = sampling.kept_mask(xd, cuts.get("top_k"), cuts.get("top_p"), cuts.get("min_p"))
        for entry in ("filtered", "penalized", "constrained"):
            tok, _, kept = _draw(entry, x, 0.7, C.MIRROR_KEY, **cuts)
            same = (kept.cpu().long() == keep.sum(-1)).numpy()
            assert same.all() if exact else (~same).sum() <= 0.01 * len(same)
            win, margin, lowest = M.mirror_draw(x64, 0.7, *C.MIRROR_KEY, keep=keep.numpy())
            skipped = _agrees(tok, (win, np.where(same, margin, 0.0), lowest), e)
            print(f"{cuts} {entry}: rows not compared {skipped}")
            assert skipped <= 0.02 * len(same)


# ---- 2. a decisive logit wins from every position ------------------------------------------------------------------------------------
# n = 8221 = 1027 full chunks + 5 columns.  Plain kernel: 256 threads, thread t owns chunks t + 256 i; the others: 1024 threads.
DECISIVE_N = 8221
DECISIVE_COLS = sorted({0, 7, 8, 15, 504, 511, 2040, 2047, 8184, 8191,  # first / last column of a chunk; last thread of a wave
                        *[512 * w for w in range(16)], *[512 * w + 511 for w in range(16)],  # first / last thread of every wave
                        2048, 2055, 4096,  # the plain kernel's second and third trip
                        8192, 8199, 8200, 8215,  # the other kernels' second trip (threads 0, 1 and 2)
                        8216, 8219, 8220})  # the scalar tail; the last column of an odd n


@pytest.mark.parametrize("pad", [3, 0])  # a row stride of 8224 (a strided view, 16-byte loads) and of 8221 (odd: scalar loads)
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_a_decisive_logit_is_drawn_from_every_position(dtype, pad):
    rows, n = len(DECISIVE_COLS), DECISIVE_N
    g = torch.Generator().manual_seed(31 + pad)
    cols = torch.tensor(DECISIVE_COLS)
    for T in (0.7, 1.0):
        xc = (torch.randn(rows, n, generator=g) * 3.0).to(C.DT[dtype])
        others = float(xc.double().max())
        xc[torch.arange(rows), cols] = others + 20.3 * T + 1.0
        lead = xc.double()[torch.arange(rows), cols] - others
        assert (lead > 20.3 * T).all()  # the noise spans less than 20.3 (tests/test_sampling_stress.py): nothing else can win
        x = C.on_device(C._strided(xc, pad, dtype), dtype, DEV)
        assert x.stride(0) == n + pad
        for key in ((7, 0), C.MIRROR_KEY):
            for entry in ENTRIES:
                for cuts in ((dict(),) if entry == "plain" else (dict(), dict(top_k=3, top_p=0.9, min_p=0.1))):
                    tok = _draw(entry, x, T, key, **cuts)[0].cpu()
                    assert torch.equal(tok, cols), (entry, cuts, T, cols[tok != cols], tok[tok != cols])
    print(f"{rows} positions x 4 entry points: all drawn")


# ---- 3. structural uniformity on flat rows ---------------------------------------------------------------------------------------------
THREADS = {"plain": 256, "filtered": 1024}


@functools.lru_cache(maxsize=4)
def _flat_tokens(entry, offset):
    x = torch.zeros((C.UNIFORM_ROWS, C.UNIFORM_V + 3), dtype=torch.bfloat16, device=DEV)[:, : C.UNIFORM_V]  # stride 8224: 16-byte loads
    return _draw(entry, x, 1.0, (C.MIRROR_KEY[0], offset))[0].cpu().numpy()


@pytest.mark.parametrize("entry", ["plain", "filtered"])
def test_flat_rows_draw_the_lowest_index_of_the_largest_k(entry):
    tok = _flat_tokens(entry, C.MIRROR_KEY[1])[: C.FLAT_ROWS]
    lowest, highest = M.flat_row_tokens(C.FLAT_ROWS, C.UNIFORM_V, *C.MIRROR_KEY)
    print(f"rows with an exact tie of the largest k: {int((lowest != highest).sum())} of {C.FLAT_ROWS}")
    assert np.array_equal(tok, lowest)


@pytest.mark.parametrize("entry", ["plain", "filtered"])
def test_drawn_columns_are_uniform_over_what_owns_them(entry):
    rows, V, threads = C.UNIFORM_ROWS, C.UNIFORM_V, THREADS[entry]
    tok = _flat_tokens(entry, C.MIRROR_KEY[1])
    assert tok.min() >= 0 and tok.max() < V
    col = np.arange(V)
    chunk = col // 8
    owners = {"position in the 8-chunk": col % 8, "Philox word": col % 4, "wave": (chunk % threads) // 64, "loop trip": chunk // threads}
    stats = {}
    for what, owner in owners.items():
        expected = np.bincount(owner) * (rows / V)
        assert expected.min() >= 5
        stats[what] = (C.chi_square(np.bincount(owner[tok], minlength=len(expected)), expected), C.CHI2_Q[len(expected) - 1])
    # coincidences: neighbouring rows, and the same rows under consecutive keys (_next_sample_key advances the offset by 4)
    limit = C.POISSON_Q[rows / V]
    again = _flat_tokens(entry, C.MIRROR_KEY[1] + 4)
    pairs = {"neighbouring rows": int((tok[1:] == tok[:-1]).sum()), "offsets o and o + 4": int((tok == again).sum())}
    print(f"{entry}: chi-square (statistic, 1 - 1e-6 quantile) {stats}; coincidences {pairs} (limit {limit})")
    for what, (stat, q) in stats.items():
        assert stat <= q, (what, stat, q)
    for what, count in pairs.items():
        assert count <= limit, (what, count)


# ---- 4. the select against the definition ------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", list(C.CASES))
def test_select_equals_the_definition_on_adversarial_rows(name):
    case = C.build(name)
    xc, n = case["x"], case["n"]
    x = C.on_device(xc, case["dtype"], DEV)
    assert (x.stride(0) if x.shape[0] > 1 else n) == n + case["pad"]
    xd = xc.double()
    xs = xd.masked_fill(torch.isnan(xd), -math.inf)
    greedy = torch.where(xs == xs.amax(-1, keepdim=True), torch.arange(n), torch.full((1,), n)).amin(-1)
    logp = None if case["pattern"] in C.HAS_POS_INF else torch.log_softmax(xs, -1)
    worst = 0.0
    for top_k, top_p, min_p in case["cuts"]:
        cuts = dict(top_k=top_k, top_p=top_p, min_p=min_p)
        keep = sampling.kept_mask(xd, top_k, top_p, min_p)
        for T in (0.0, 1.0, 50.0):
            a = _draw("filtered", x, T, (3, 40), **cuts)
            b = _draw("penalized", x, T, (3, 40), **cuts)
            assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b)), (cuts, T)
            tok, lp, kept = (t.cpu() for t in a)
            assert torch.equal(kept.long(), keep.sum(-1)), (cuts, T, kept, keep.sum(-1))
            assert ((tok >= 0) & (tok < n)).all() and keep.gather(1, tok[:, None]).all(), (cuts, T, tok)
            if T == 0.0:
                assert torch.equal(tok, greedy), (cuts, tok, greedy)
            if logp is not None:
                diff = (lp.double() - logp.gather(1, tok[:, None])[:, 0]).abs().max().item()
                worst = max(worst, diff)
                assert diff < 1e-4, (cuts, T, diff)
        again = _draw("filtered", x, 1.0, (3, 40), **cuts)  # a repeated key: the same bits
        first = _draw("filtered", x, 1.0, (3, 40), **cuts)
        assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(again, first))
    print(f"{name}: {len(case['cuts'])} cuts x 3 temperatures, kept counts exact; largest |log-prob - float64| = {worst:.3g}")


@pytest.mark.parametrize("name", [k for k, v in C.CASES.items() if v["pattern"] == "pos_inf"])
def test_tied_infinities_draw_the_lowest_index_at_every_temperature(name):
    """+inf + noise = +inf: the +inf columns tie exactly whatever the noise, and the lowest index wins -- across lanes and waves"""
    case = C.build(name)
    x = C.on_device(case["x"], case["dtype"], DEV)
    first = (case["x"].double() == math.inf).int().argmax(-1)
    for entry in ENTRIES:
        for T in (0.0, 1.0, 50.0):
            assert torch.equal(_draw(entry, x, T, C.MIRROR_KEY)[0].cpu(), first), (entry, T)
    print(f"{name}: the first of 1 / 3 tied +inf columns drawn on {x.shape[0]} rows x 4 entry points x 3 temperatures")
