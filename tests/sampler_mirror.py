"""The samplers' noise and draw on the host, in numpy (importable without a GPU).

The four sampling launches (hyd_sample_tokens: sample_kernel in csrc/layer_ops.hip; hyd_sample_tokens_filtered: csrc/sample_filter.hip;
hyd_sample_tokens_penalized / _constrained: sample_row in csrc/sample_select.h) draw  token = argmax_j ( l_j * (1/T) + g_j )  over the
kept, valid columns (lowest index on ties) with Gumbel noise g from Philox4x32-10, all four from one text (philox10 / gumbel_noise in
csrc/vocab_row.h).  The suite holds them bit-equal to each other; this
module is the independent side: Philox from its published definition (checked against the Random123 known-answer vectors), the
counter / key / word layout from the kernels' headers, the noise in float64.

  column j of row r:   word j % 4 of philox4x32_10(counter = (j // 4, r, offset & 0xffffffff, offset >> 32),
                                                     key = (seed & 0xffffffff, seed >> 32))
  k = bits >> 9 (23 bits),  u = (k + 1/2) 2^-23,  e = max(-ln u, 2^-25),  g = -ln e          (float64)

g lies in [G_MIN, G_MAX] = [-2.82, 17.4]: k = 0 gives -ln(24 ln 2) = -2.8117, the clamp bounds it by 25 ln 2 = 17.33
(tests/test_sampler_noise.py asserts the same 17.4).

EPS: the margin below which a row is not compared
-------------------------------------------------
The kernels evaluate v_j = fl(fl(l_j * fl(1 / T)) + g32_j) in fp32 (or the fused form with one rounding fewer); the mirror evaluates
s_j = l_j / T + g_j in float64 with T the fp32 value the kernel is given and l_j the exact value of the (16-bit or fp32) logit.  With
M = max |l_j| over the case's valid finite logits, |g| <= G_MAX and every fp32 rounding a relative 2^-24:
    rounding of 1/T      <= 2^-24 M / T
    rounding of l * (1/T) <= 2^-24 M / T (1 + 2^-24)
    rounding of the sum  <= 2^-24 (M / T + G_MAX) (1 + 2^-23)
    g32 against g        <= GUMBEL_ERR
so |v_j - s_j| <= ERR(M, T) = 2^-24 (3 M / T + G_MAX) (1 + 2^-22) + GUMBEL_ERR, and
    EPS(M, T) = 4 ERR(M, T):
two competing columns are each off by ERR at most (2 ERR on their difference), and the factor 4 leaves the same again for the
rounding of the mirror's own difference and sum (float64: nothing by comparison).  A row whose float64 margin exceeds EPS has the
same winner in fp32; a row whose best two values are EXACTLY equal in float64 has equal logits and equal k, hence equal fp32 values,
and the lowest index wins on both sides; rows with 0 < margin <= EPS are not compared (and are counted: the tests bound their share).

GUMBEL_ERR = 1.62e-6 is measured, not derived: tests/probes/gumbel_noise_probe.hip evaluates the kernels' gumbel expression (two
hardware log2 instructions) for all 2^23 values of k on an MI355X and compares with the float64 expression above; the record is
profiles/sampler_noise_probe.md: max |g32 - g| = 1.610471e-06 at k = 8388598 (9.49e-07 outside the 4096 largest k), g32
non-decreasing in k, range [-2.811541, 16.635532].  For randn * 3 logits at T = 0.7 (M about 15) EPS is 2.7e-5.
"""
from __future__ import annotations

import numpy as np

G_MIN, G_MAX = -2.82, 17.4
GUMBEL_ERR = 1.62e-6  # profiles/sampler_noise_probe.md (measured 1.610471e-06, rounded up)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123): counter = 4 and
    key = 2 arrays (or scalars) of 32-bit values, broadcast against each other -> 4 uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _MASK for c in counter])
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _MASK for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniform(bits):
    """u = ((bits >> 9) + 1/2) 2^-23 in float64 (exact; the kernels' fp32 value is the same number: tests/test_sampler_noise._u)."""
    return ((np.asarray(bits, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(bits):
    e = np.maximum(-np.log(uniform(bits)), 2.0 ** -25)
    return -np.log(e)


def philox_bits(rows, n: int, seed: int, offset: int, word_order=(0, 1, 2, 3)):
    """-> uint64 [R, n]: the 32-bit Philox word of every column, for rows = a row count (rows 0 .. R - 1) or an array of row indices.
    word_order: which output word a column's j % 4 takes -- the kernels' is the identity; anything else is a mutation for
    tests/test_sampling_stress.py."""
    r = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64)
    calls = (n + 3) // 4
    ctr = (np.arange(calls, dtype=np.uint64)[None, :], r[:, None], np.uint64(offset & 0xFFFFFFFF), np.uint64((offset >> 32) & 0xFFFFFFFF))
    words = philox4x32_10(ctr, (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)))
    return np.stack([words[w] for w in word_order], axis=-1).reshape(len(r), 4 * calls)[:, :n]


def noise(rows, n: int, seed: int, offset: int, word_order=(0, 1, 2, 3)):
    """-> (g float64 [R, n], k uint32 [R, n]): the Gumbel noise and the 23 bits it is made from (rows, word_order: philox_bits)"""
    bits = philox_bits(rows, n, seed, offset, word_order)
    return gumbel(bits), (bits >> np.uint64(9)).astype(np.uint32)


def flat_row_tokens(rows: int, n: int, seed: int, offset: int, chunk: int = 1024):
    """What a row of n EQUAL logits must draw at any T > 0, for rows 0 .. rows - 1: g is non-decreasing in k (the probe's record)
    and equal k give equal values, so the token is the lowest index of the largest k.  -> (lowest, highest) index of the largest k;
    they differ on the rows that tie."""
    lo, hi = [], []
    for a in range(0, rows, chunk):
        k = philox_bits(np.arange(a, min(a + chunk, rows)), n, seed, offset) >> np.uint64(9)
        top = k == k.max(-1, keepdims=True)
        lo.append(top.argmax(-1))
        hi.append(n - 1 - top[:, ::-1].argmax(-1))
    return np.concatenate(lo), np.concatenate(hi)


def err(max_abs_logit: float, T: float) -> float:
    """ERR(M, T) of the module docstring"""
    return 2.0 ** -24 * (3.0 * max_abs_logit / T + G_MAX) * (1 + 2.0 ** -22) + GUMBEL_ERR


def eps(max_abs_logit: float, T: float) -> float:
    """EPS(M, T) = 4 ERR(M, T)"""
    return 4.0 * err(max_abs_logit, T)


def max_abs(x64) -> float:
    """M: the largest magnitude among the finite entries of x64 (0 if there is none)"""
    x = np.asarray(x64, dtype=np.float64)
    f = np.isfinite(x)
    return float(np.abs(x[f]).max()) if f.any() else 0.0


def mirror_draw(x64, T: float, seed: int, offset: int, keep=None, rows=None, word_order=(0, 1, 2, 3)):
    """x64 float64 [R, n] (the exact values of the logits; NaN and -inf are never drawn), T > 0, keep bool [R, n] or None (all) ->
    (winner [R], margin [R], lowest [R]): the arg-max of s = x64 / fp32(T) + g over the kept valid columns, the distance from its
    value to the best value that differs from it (inf if there is none), and the lowest index among the columns whose value equals
    the winner's exactly (numpy's argmax returns that one as the winner too: `lowest` is computed on its own).  A row without a kept
    valid column: winner 0, margin inf.  rows: the Philox row index of every row of x64 (default 0 .. R - 1)."""
    x = np.asarray(x64, dtype=np.float64)
    R, n = x.shape
    g, _ = noise(R if rows is None else rows, n, seed, offset, word_order)
    ok = ~np.isnan(x) & (x != -np.inf)
    if keep is not None:
        ok &= np.asarray(keep, dtype=bool)
    with np.errstate(invalid="ignore"):
        s = np.where(ok, np.where(ok, x, 0.0) / float(np.float32(T)) + g, -np.inf)
    winner = s.argmax(-1)
    top = s.max(-1)
    tied = s == top[:, None]
    lowest = np.where(tied, np.arange(n)[None, :], n).min(-1)
    rest = np.where(tied, -np.inf, s).max(-1)
    with np.errstate(invalid="ignore"):
        margin = np.where(np.isfinite(rest), top - rest, np.inf)
    none = ~ok.any(-1)
    winner, lowest = np.where(none, 0, winner), np.where(none, 0, lowest)
    return winner, np.where(none, np.inf, margin), lowest
