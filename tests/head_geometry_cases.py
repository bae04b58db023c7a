"""
Head geometries that are not powers of two: the shared table of tests/test_head_geometry.py (CPU) and
tests/test_head_geometry_gpu.py (-m gpu).

The head count is where the attention kernels branch (DESIGN.md "Head geometries"): the prefix pass decodes its unit and its
rows by dividing by Hkv and g = Hq / Hkv, the grouped-query suffix kernel picks its heads per workgroup from Hkv and cuts
nq * g rows into 16-row chunks, the token-row kernel deals Hkv / (heads per wave instruction) waves per sequence, the
one-unit-per-wave kernel packs 4 heads into a wave.  Every case list below names the launch rule it relies on; the CPU test
recomputes the branch values from (Hq, Hkv, D) so that the table cannot silently stop covering one.

All inputs are seeded normal noise, drawn per kv head (tests.cases._round / make_case): two kv heads never hold the same keys
or values, so a kernel that reads the wrong head, or writes the wrong row, gives a visibly wrong answer -- and `blame_rows`
says whose answer it is.
"""
from __future__ import annotations

import zlib

import numpy as np

from tests.cases import _round, make_case

# name -> (Hq, Hkv)
GEOMETRIES = {
    "mha3": (3, 3), "mha5": (5, 5), "mha6": (6, 6), "mha7": (7, 7), "mha12": (12, 12), "mha20": (20, 20), "mha24": (24, 24),
    "g2x3": (6, 3), "g2x5": (10, 5), "g2x7": (14, 7), "g3x6": (18, 6), "g3x8": (24, 8), "g4x10": (40, 10), "g5x2": (10, 2),
    "g7x1": (7, 1), "g7x2": (14, 2), "g7x3": (21, 3), "g7x4": (28, 4), "g12x1": (12, 1), "g71": (71, 1),
}


def heads(geom) -> tuple[int, int]:
    """(Hq, Hkv) of a named geometry; a literal (Hq, Hkv) passes through."""
    return GEOMETRIES[geom] if isinstance(geom, str) else tuple(geom)


def geom_id(geom) -> str:
    return geom if isinstance(geom, str) else f"{geom[0]}x{geom[1]}"


# ---- A. prefix pass ---------------------------------------------------------------------------------------------------------
# A1 flash_attention: (geometry, D).  The unit decode divides by Hkv, the row decode by g (prefix_unit_w64.h fdiv).
A1_CASES = [(g, 128) for g in ("mha3", "mha5", "g2x3", "g2x5", "g3x8", "g4x10", "g7x1", "g7x3", "g7x4", "g12x1", "g71")] + \
           [(g, D) for D in (64, 256) for g in ("g2x3", "g7x1", "g7x3", "g4x10")]
A1_B, A1_SK = 2, 150


def a1_sq(geom) -> int:
    """50 query tokens from g = 3 on (350 rows at g = 7: three 128-row blocks whose boundaries fall inside a token), 150 below."""
    hq, hkv = heads(geom)
    return 50 if hq // hkv >= 3 else 150


# A2 forced split counts (div_nsplit): sk = 128 ns - 46 rounds to 128-key splits, exactly ns of them
A2_SPLITS = (3, 5, 6, 7)
A2_GEOM, A2_B, A2_SQ = "g7x3", 1, 9


def a2_sk(ns: int) -> int:
    return 128 * ns - 46


# A3 flash_attention_varlen
A3_GEOMS = ("g7x3", "g2x5")
A3_QLENS = [3, 1, 7, 140]
A3_KLENS = {False: [9, 130, 1, 64], True: [9, 130, 7, 200]}  # causal: every query keeps at least one key
# A4 256-row workgroups: 1573 tokens x 7 heads = 11011 rows per kv head; 87 x 3 = 261 128-row units > 256 -> 44 x 3 256-row units
A4_GEOM, A4_SQ, A4_SK, A4_GRID = "g7x3", 1573, 70, 132
# A5 causal with several sequences per group (per = 3)
A5_GEOMS = ("g3x8", "g7x1")
A5_SB, A5_B, A5_NQ, A5_KV = 2, 6, 3, 40

# ---- B. suffix pass ---------------------------------------------------------------------------------------------------------
LENS_HEAD = [1, 31, 32, 33, 64]  # ... then S; the rest is drawn


def suffix_lens(rng, B: int, S: int) -> np.ndarray:
    """int32 [B]: starts with [1, 31, 32, 33, 64, S] clipped to S (a batch too small for all of them still ends with S)."""
    sl = rng.integers(0, S + 1, B).astype(np.int32)
    edge = [min(x, S) for x in LENS_HEAD + [S]]
    sl[: min(B, len(edge))] = edge[:B]
    if B < len(edge):
        sl[-1] = S
    return sl


# B1 matrix-core kernel, one wave per unit: kv_len 70 < 128 (gqa_few_units); heads per workgroup from gqa_launch_plan
B1_B, B1_S = 40, 70
B1_CASES = [("g7x4", 128), ("g3x6", 128), ("g7x3", 128), ("g4x10", 128), ("g71", 128), ("g12x1", 128),
            ("g7x2", 64), ("g71", 64), ("g3x8", 256), ("g7x1", 256)]
# B2 few units: units * chunks < 1024 and kv_len 300 >= 128 -> four waves per unit (D 64 / 128); D = 256 is not eligible then
# (suffix_gqa_eligible) and runs the dot-product kernel, R = 4 (rows <= 4) or 8 rows per chunk (g12x1: 8 + a ragged 4)
B2_B, B2_S = 3, 300
B2_CASES = [(g, D) for D in (64, 128) for g in ("g7x4", "g7x3", "g71")] + [("g3x8", 256), ("g7x1", 256), ("g12x1", 256)]
# B3 nq > 1 with odd g: iq = row / g, gq = row % g
B3_B, B3_S = 40, 40
B3_CASES = [("g7x3", 3), ("g5x2", 2), ("mha5", 3)]  # (geometry, nq), D = 128
# B4 token-row kernel (Hq == Hkv a multiple of the 64 / (D / 8) heads of a wave instruction, kv_len < 64 keeps the shape off
# the four-wave rule): 3, 5 or 6 waves per sequence, so the last workgroup row is ragged
B4_B, B4_S = 9, 40
B4_CASES = [("mha12", 128), ("mha20", 128), ("mha24", 128), ((24, 24), 64), ((40, 40), 64), ("mha6", 256), ((10, 10), 256)]
# B5 one-unit-per-wave kernel (Hkv no multiple of the heads of a wave instruction, or two rows per unit)
B5_LENS = [1, 12, 13, 5, None, 0, 9, 33, 2]  # None = S; <= 12 takes the packed lane-group path where the shape allows it
B5_CASES = [(g, 128) for g in ("mha5", "mha6", "mha7", "mha3", "g2x3", "g2x5", "g2x7")] + \
           [("mha3", 64), ("mha12", 64), ("mha3", 256), ("mha5", 256)]
B5_FORMS = {"one-wave": (9, 40), "four-waves": (3, 200)}  # name -> (B, S): kv_len >= 64 and few units -> four waves per unit


def b5_lens(B: int, S: int) -> np.ndarray:
    lens = [S if x is None else x for x in B5_LENS]
    if B < len(lens):  # the four-wave form's three sequences: a short one, the full cache, an empty one
        lens = [12, S, 0][:B]
    return np.asarray(lens, dtype=np.int32)


# ---- C. the whole operator --------------------------------------------------------------------------------------------------
C_GEOMS = [("g7x4", 128), ("g7x3", 128), ("g4x10", 128), ("mha6", 128), ("mha5", 128), ("mha12", 128), ("g71", 64), ("g7x2", 64)]
C_HIERARCHIES = {
    "ragged": [[37], [9, 1, 40, 17, 3, 12]],
    "varlen+uniform": [[70, 33], [12] * 3, [5, 16, 3, 1, 9, 2]],
    # g = 7: 12 x 7 = 84 rows per (group, kv head) > 64 (level_is_small) -> the prefix kernel, merged in the suffix epilogue
    "prefix-kernel": [[200], [64] * 12],
}
C_SPLIT_HIERARCHY = ("split", [[2048], [20] * 4], "g7x4", 128)  # few units on a long prefix: fp32 split-KV slices into the epilogue
C_PREFILL = ("g7x3", 128, [[37], [5] * 4], 5)  # nq = 5, seq_lens = None: the causal unique-suffix prefill


def operator_cases():
    """(id, sizes, geometry, D) of every nq = 1 operator case."""
    out = [(f"{hn}-{g}-D{D}", sizes, g, D) for hn, sizes in C_HIERARCHIES.items() for g, D in C_GEOMS]
    hn, sizes, g, D = C_SPLIT_HIERARCHY
    return out + [(f"{hn}-{g}-D{D}", sizes, g, D)]


def operator_case(sizes, geom, D, dt, nq=1):
    hq, hkv = heads(geom)
    seed = zlib.crc32(repr((sizes, hq, hkv, D, dt, nq)).encode())
    return make_case(sizes=sizes, qheads=hq, kvheads=hkv, dim=D, dtype=dt, seed=seed, nq=nq, force_seq_lens=nq == 1)


# ---- D. fp8 unique caches: (geometry, B, S), D = 128 ---------------------------------------------------------------------------
D_NATIVE_GQA = [("g7x4", 40, 70), ("g7x3", 40, 70), ("g4x10", 40, 70), ("g3x6", 40, 70)]  # the grouped-query fp8 kernel
D_NATIVE_ROWS = [("mha12", 9, 40), ("mha20", 9, 40)]                                            # the fp8 token-row kernel
D_NATIVE = D_NATIVE_GQA + D_NATIVE_ROWS
D_ORACLE = [("g7x4", 40, 70)] + D_NATIVE_ROWS  # held to the float64 oracle on the dequantized caches
D_FALLBACK = [("mha5", 9, 40), ("mha6", 9, 40)]  # one-row units, Hkv no multiple of 4: no fp8 kernel takes them

# ---- E. model shell: (heads, kv heads) -------------------------------------------------------------------------------------------
E_HEADS = [(6, 2), (3, 3), (7, 1)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def rand(rng, shape, dt):
    return _round(rng.standard_normal(shape, dtype=np.float32), dt)


def seeded(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def poison(k, v, lens):
    """Copies of k / v [B, S, Hkv, D] with NaN keys and +Inf / -Inf / NaN values at and past every sequence's length."""
    kp, vp = k.copy(), v.copy()
    for b, n in enumerate(lens):
        kp[b, n:] = np.nan
        vp[b, n:] = (np.inf, -np.inf, np.nan)[b % 3]
    return kp, vp


# ---- failure text ------------------------------------------------------------------------------------------------------------
def blame_rows(got, want, bound, show=4) -> str:
    """For failure messages only.  got / want: [B, nq, H, D].  Lists the (b, iq, head) rows whose largest error exceeds
    `bound` and, for the first `show` of them, whether `got` equals (within the bound) the oracle's row of ANOTHER head or
    sequence: a head or row mix-up then names itself."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.ndim == 4, (got.shape, want.shape)
    B, nq, H, D = want.shape
    err = np.abs(np.nan_to_num(got, nan=np.inf) - want).max(-1)
    bad = np.argwhere(err > bound)
    if not len(bad):
        return "no row exceeds the bound"
    lines = [f"{len(bad)} of {B * nq * H} rows exceed {bound:.3e}; heads hit: {sorted(set(int(h) for h in bad[:, 2]))[:24]}, "
             f"sequences hit: {sorted(set(int(b) for b in bad[:, 0]))[:24]}"]
    flat = want.reshape(-1, D)
    for b, iq, h in bad[:show]:
        d = np.abs(np.nan_to_num(got[b, iq, h], nan=np.inf)[None] - flat).max(-1)
        hit = np.argwhere(d <= bound).ravel()
        where = [tuple(int(x) for x in np.unravel_index(i, (B, nq, H))) for i in hit[:3]]
        lines.append(f"  row (b={b}, iq={iq}, head={h}): max error {err[b, iq, h]:.3e}; "
                     + (f"it IS the oracle's row (b, iq, head) = {where}" if where else "it matches no other row of the oracle"))
    return "\n".join(lines)
