"""-m gpu: hyd_sample_tokens_filtered returns the very bits it returned before its row primitives moved into csrc/vocab_row.h.  The
cuts use integer masses and the draw is a total order on (value, index), so a kernel that is recompiled, rescheduled or rebuilt on
shared text (sample_filter_kernel's body as an instantiation of csrc/sample_select.h's sample_row, say) gives identical tokens, kept
counts and log-prob bits, not close ones: the comparison has no tolerance.

tests/golden/sample_filter_parent.npz holds what the kernel returned before the move, recorded by this module's own `outputs()`:

    python -m tests.test_sampler_golden_gpu --record [PATH]

The inputs are not stored: every row comes from tests/sampling_stress_cases.py's builders and this module's seeds.  The rows are the
smallest on which the body can go wrong: n = 13 (shorter than one chunk per wave, ragged tail), 1000 (idle threads), 16397 (more
than one chunk per thread, ragged tail); a row stride that keeps 16-byte loads and one that breaks them; per dtype and shape the
k-th logit in the last distance bin over masses that underflow to 0 (far_tail), ties across every threshold (plateau), a +0 / -0
plateau, and rows of few or no valid logits (NaN, -inf); each crossed with T = 0 / 0.7 and no cut, top-k, top-p, min-p, all three."""
import functools
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from hydragen_amd import layer_ops
from tests import sampling_stress_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden" / "sample_filter_parent.npz"
NS = (13, 1000, 16397)
STRIDES = ("aligned", "odd")  # the row stride: n rounded up to a multiple of 8 (vec_ok = 1) / the next odd number (vec_ok = 0)
TEMPERATURES = (0.0, 0.7)
ROWS = 6


def _plateau(n, **kw):
    shape = dict(width=3, above=2) if n < 32 else dict(width=100, above=9)
    return dict(pattern="plateau", **shape, **kw)


def _no_valid(spec, rng):
    """few_valid's rows (1, 4, 5, 6 valid columns) and two rows without a valid logit: NaN and -inf mixed, -inf alone"""
    x, cuts, _ = C.few_valid(dict(spec, rows=ROWS - 2), rng)
    tail = torch.full((2, spec["n"]), -torch.inf, dtype=x.dtype)
    tail[0, ::3] = torch.nan
    return torch.cat([x, tail]), cuts, None


def _rows(pattern, dtype, n, stride):
    """-> (x [ROWS, n] CPU tensor with the asked row stride, the five cuts (top_k, top_p, min_p))"""
    name = f"{pattern}_{dtype}_{n}"  # (the two strides hold the same values)
    spec = dict(dict(far_tail=dict(pattern="far_tail"), plateau=_plateau(n), signed_zero=_plateau(n, value=0.0, signed_zero=True),
                     no_valid=dict(pattern="no_valid"))[pattern], n=n, dtype=dtype, rows=ROWS)
    build = _no_valid if pattern == "no_valid" else C.PATTERNS[spec["pattern"]]
    x, cuts, _ = build(spec, np.random.default_rng(zlib.crc32(name.encode())))
    assert x.shape == (ROWS, n) and x.dtype == C.DT[dtype]
    (k, _, _), (_, p, _), (_, _, mp), (_, pk, _) = cuts[:4]  # the builders' cuts: top-k, top-p, min-p, top-p after that top-k
    pad = (-n) % 8 if stride == "aligned" else 2 - (n + 1) % 2
    return C._strided(x, pad, dtype), n + pad, [(None, None, None), (k, None, None), (None, p, None), (None, None, mp), (k, pk or p, mp)]


PATTERNS = ("far_tail", "plateau", "signed_zero", "no_valid")
CASES = [(pt, dt, n, st) for dt in ("f16", "bf16", "f32") for n in NS for st in STRIDES for pt in PATTERNS]


def outputs() -> dict:
    """name -> array [cuts x temperatures, ROWS] of every case: tokens int64, kept counts int32, log-probs as uint32 bits"""
    out = {}
    for pattern, dtype, n, stride in CASES:
        xc, want_stride, cuts = _rows(pattern, dtype, n, stride)
        x = C.on_device(xc, dtype, DEV)
        assert x.stride(0) == want_stride and (x.data_ptr() % 16 == 0)
        got = [layer_ops.sample_tokens_filtered(x, T, C.MIRROR_KEY, top_k=k, top_p=p, min_p=mp) for k, p, mp in cuts for T in TEMPERATURES]
        tok, lp, kept = (torch.stack([g[i].reshape(-1) for g in got]).cpu() for i in range(3))
        name = f"{pattern}/{dtype}/{n}/{stride}"
        out[name + "/tokens"] = tok.numpy().astype(np.int64)
        out[name + "/kept"] = kept.numpy().astype(np.int32)
        out[name + "/logprob_bits"] = lp.view(torch.int32).numpy().view(np.uint32)
    return out


@functools.lru_cache(maxsize=1)
def _got():
    return outputs()


@functools.lru_cache(maxsize=1)
def _want():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case_and_nothing_else():
    want = _want()
    assert sorted(want) == sorted(_got())
    for k, v in want.items():
        assert v.shape == (len(TEMPERATURES) * 5, ROWS), k
        assert v.dtype == dict(tokens=np.int64, kept=np.int32, logprob_bits=np.uint32)[k.rsplit("/", 1)[1]], k


@pytest.mark.parametrize("what", ["tokens", "kept", "logprob_bits"])
def test_filtered_sampler_returns_the_recorded_bits(what):
    got, want = _got(), _want()
    differ = [k for k in want if k.endswith("/" + what) and not np.array_equal(got[k], want[k])]
    assert not differ, (differ, got[differ[0]], want[differ[0]])


def test_the_rows_exercise_what_they_are_there_for():
    """kept counts of the recording itself: the cuts cut, the rows without a valid logit keep nothing, and top-k on a plateau keeps
    its ties -- a fixture of trivial rows would compare equal whatever the kernel did"""
    want = _want()
    NONE, TOP_K, TOP_P, MIN_P, ALL3 = (len(TEMPERATURES) * c for c in range(5))  # the first row of each cut (T = 0)
    for dtype in ("f16", "bf16", "f32"):
        for n in NS:
            kept = want[f"far_tail/{dtype}/{n}/odd/kept"]
            assert (kept[NONE] == n).all() and (kept[TOP_K] >= 8).all() and (kept[TOP_K] < n).all()  # (8 and the 8th's ties)
            assert (kept[TOP_P] <= 5).all() and (kept[MIN_P] <= 5).all() and (kept[ALL3] <= 5).all()  # the head alone
            kept = want[f"no_valid/{dtype}/{n}/aligned/kept"]
            assert (kept[:, ROWS - 2:] == 0).all() and (kept[:, : ROWS - 2] > 0).all()
            width, above = (3, 2) if n < 32 else (100, 9)
            assert (want[f"plateau/{dtype}/{n}/aligned/kept"][TOP_K] == above + width).all()  # top_k = above + 1 keeps the plateau
            assert (want[f"signed_zero/{dtype}/{n}/odd/kept"][TOP_K] == above + width).all()
            assert (want[f"no_valid/{dtype}/{n}/odd/tokens"][:, ROWS - 2:] == 0).all()
            assert (want[f"no_valid/{dtype}/{n}/odd/logprob_bits"][:, ROWS - 2:] == 0x7FC00000).all()


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    path = Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN
    np.savez_compressed(path, **outputs())
    print(f"recorded {len(CASES)} cases in {path} ({path.stat().st_size} bytes)")
