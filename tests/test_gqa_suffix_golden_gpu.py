"""-m gpu: the matrix-core (grouped-query) suffix kernels -- 16-bit, causal-tail and fp8 -- return the very bits they returned while
csrc/suffix_gqa_kernel.h and csrc/suffix_attn_gqa_fp8.hip each held a hand-kept copy of the partials, the softmax step, the four-wave
merge and the epilogue.  The shared pieces (csrc/suffix_gqa_unit.h) are the same expression trees, so a kernel rebuilt on them gives
identical bytes unless a product was contracted differently, a guard moved or a piece was wired to the wrong state: the comparison has
no tolerance.

tests/golden/gqa_suffix_parent.npz holds what the two copies returned, recorded once on an MI355X with the library of the commit
before the pieces were shared (HYDRAGEN_HIP_LIB selects a library), by this module's own `outputs()`:

    python -m tests.test_gqa_suffix_golden_gpu --record [PATH]

It is never re-recorded from a later tree.  The inputs are not stored: q / k / v and the hand-made partials are normal values from
numpy.random.default_rng seeded by the case's name (fp8 caches: rounded to e4m3 in numpy).  Stored per family: the case names and a
zlib.crc32 per case and batch row of `out` and of `lse` (0 where the case asks for no LSE).

Every sequence's cache rows at and past its length hold NaN (16-bit NaN, the fp8 byte 0x7F).  Lengths: 0, 1, 31, 32, 33, 64, 65 and
the capacity -- the empty sequence, one step, the masked last step, exactly two steps, the third step that refills a tile set where
two are kept (NSET = 2) -- plus 97 and 129 on a 160-row cache, where with four waves per unit some waves get no step at all.

    hpw4        12/4 heads, 96 rows     one wave per unit, 4 kv heads per workgroup, 3-row units
    hpw2        10/2 heads, 96 rows     2 kv heads per workgroup, 5 ragged rows (also D = 256)
    hpw1        21/3 heads, nq 3        1 head per workgroup, 21 rows = two 16-row chunks, nq > 1 non-causal (also D = 256)
    four_waves  8/1 heads, 160 rows     gqa_few_units: the cross-wave merge, idle waves
    causal      CAUSAL_SHAPES           the causal-tail kernel: a row's limit before a wave's first tile, len < T
    small_level two small levels (sb 1, P 40; sb 2, P 24) over hpw4's unique cache, the whole operator: the shared_kv one-wave
                instantiation (default cache policy), then two 16-bit partials in the suffix pass
    one_launch  one level (sb 2) of P = 24 / 160 keys over hpw4's unique cache: the two-segment walk, one wave / four waves per unit.
                (The launcher counts the keys of BOTH segments against gqa_few_units' 128: P = 40 on a 96-row cache would take four
                waves as P = 160 does, so the one-wave walk has P = 24.)
    +partials   hpw4, four_waves and the four-wave causal shape through hyd_suffix_attn_fwd / _causal_fwd with hand-made partials
                (PARTIALS); in every variant one partial has lse = -inf on two batch rows, and the length-0 sequence is merge-only
    fp8         hpw4, hpw2, hpw1, four_waves and their partial variants on fp8 caches, with mixed per-head scales and with null
                scales, flash.dequantize_kv patched to raise

Each case asserts the kernel it reaches by the launcher rules tests/softmax_stress_cases.py restates."""
import ctypes as C
import functools
import sys
import zlib
from pathlib import Path
from unittest import mock

import numpy as np
import pytest
import torch

from hydragen_amd import _lib
from hydragen_amd import flash as F
from hydragen_amd.attention import hydragen_attention_nopad
from hydragen_amd.flash import flash_attention_seqlen
from hydragen_amd.kv_quant import FP8_DTYPE
from tests.glue_ref import fp8_scales
from tests.gpu_util import TORCH_DT, suffix_fwd_with_partials
from tests.softmax_stress_cases import causal_route, round_e4m3, suffix_route

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden" / "gqa_suffix_parent.npz"
BMAX = 10
# name -> (Hq, Hkv, nq, cache rows, head dims, route by suffix_route, kv heads per workgroup)
SHAPES = {
    "hpw4": (12, 4, 1, 96, (64, 128), "gqa/1-wave", 4),
    "hpw2": (10, 2, 1, 96, (64, 128, 256), "gqa/1-wave", 2),
    "hpw1": (21, 3, 3, 96, (64, 128, 256), "gqa/1-wave", 1),
    "four_waves": (8, 1, 1, 160, (64, 128), "gqa/4-waves", 1),
}
# name -> (T, Hq, Hkv, cache rows, head dims, route by causal_route)
CAUSAL_SHAPES = {
    "t2": (2, 8, 1, 70, (64, 128, 256), "gqa/1-wave/hpw1"),
    "t3": (3, 12, 4, 40, (64, 128), "gqa/1-wave/hpw4"),
    "t8": (8, 6, 2, 70, (64, 128), "gqa/1-wave/hpw2"),  # 24 rows
    "t4": (4, 8, 1, 160, (64, 128), "gqa/4-waves"),
}
# variant -> ([(is_f32, slices)], the suffix pass's own LSE asked for)
PARTIALS = {
    "none": ([], False),
    "h": ([(False, 1)], False),
    "f": ([(True, 1)], False),
    "hh": ([(False, 1)] * 2, False),
    "sss+h": ([(True, 3), (False, 1)], False),  # four partials: two requested in front of the stream, a pair behind it
    "five+lse": ([(False, 1), (True, 1), (True, 2), (False, 1)], True),  # nothing in front of the stream; pair, pair, one
}
DTS = ("f16", "bf16")
SCALES = ("mixed", "none")
ONE_LAUNCH_MAX_KEYS = 8192  # api_attn.hip kSingleLaunchMaxKeys


def _cases():
    """(name, family, runner arguments); the family is the npz entry and the test parameter"""
    out = []
    for dt in DTS:
        for s, (_, _, _, _, dims, _, _) in SHAPES.items():
            out += [(f"{s}/{dt}/{D}", "plain", ("plain", s, dt, D, None, None)) for D in dims]
            out += [(f"{s}/fp8-{sc}/{dt}/{D}", "fp8", ("plain", s, dt, D, None, sc)) for D in dims for sc in SCALES]
        for s, (_, _, _, _, dims, _) in CAUSAL_SHAPES.items():
            out += [(f"causal-{s}/{dt}/{D}", "causal", ("causal", s, dt, D, None, None)) for D in dims]
        for D in (64, 128):
            out.append((f"small_level/{dt}/{D}", "operator", ("levels", "hpw4", dt, D, ((1, 40), (2, 24)), None)))
            out += [(f"one_launch-p{P}/{dt}/{D}", "operator", ("levels", "hpw4", dt, D, ((2, P),), None)) for P in (24, 160)]
            for var in PARTIALS:
                out += [(f"{s}+{var}/{dt}/{D}", "partials", ("plain", s, dt, D, var, None)) for s in ("hpw4", "four_waves")]
                out.append((f"causal-t4+{var}/{dt}/{D}", "partials", ("causal", "t4", dt, D, var, None)))
                out += [(f"{s}+{var}/fp8-{sc}/{dt}/{D}", "fp8_partials", ("plain", s, dt, D, var, sc))
                        for s in ("hpw4", "four_waves") for sc in SCALES]
    return out


CASES = _cases()
FAMILIES = tuple(dict.fromkeys(fam for _, fam, _ in CASES))


def lengths(cap):
    """the listed lengths that fit the cache, then lengths just below the capacity up to 8 sequences"""
    sl = [x for x in (0, 1, 31, 32, 33, 64, 65) if x < cap] + [cap] + ([97, 129] if cap == 160 else [])
    return np.array(sl + [cap - 1 - i for i in range(8 - len(sl))], dtype=np.int32)


def _hpw(Hkv, D):
    """suffix_gqa_common.h gqa_launch_plan, one wave per unit on a sequence's own cache"""
    hpw = (4 if Hkv % 4 == 0 else 2 if Hkv % 2 == 0 else 1) if Hkv <= 8 else 1
    return min(hpw, 2) if D == 256 else hpw


def _normal(rng, dt, *shape):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(TORCH_DT[dt]).to(DEV)


def _caches(rng, sl, cap, Hkv, D, dt, fp8):
    """k, v [B, cap, Hkv, D] with NaN at and past each sequence's length"""
    past = torch.arange(cap)[None, :] >= torch.from_numpy(sl.astype(np.int64))[:, None]
    out = []
    for _ in range(2):
        x = rng.standard_normal((len(sl), cap, Hkv, D), dtype=np.float32)
        if fp8:
            x = torch.from_numpy(round_e4m3(x).astype(np.float32)).to(FP8_DTYPE)
            x.view(torch.uint8)[past] = 0x7F
        else:
            x = torch.from_numpy(x).to(TORCH_DT[dt])
            x[past] = float("nan")
        out.append(x.to(DEV))
    return out


def _groups(rng, var, shape, dt):
    """hand-made partials in suffix_fwd_with_partials' layout: float32 numpy (16-bit ones hold 16-bit values); the FIRST partial has
    lse = -inf (and out = 0: it covers no key) on batch rows 1 and 2"""
    groups, first = [], True
    for f32, cnt in PARTIALS[var][0]:
        members = []
        for _ in range(cnt):
            o = rng.standard_normal(shape, dtype=np.float32)
            if not f32:
                o = torch.from_numpy(o).to(TORCH_DT[dt]).float().numpy()
            l = (1.0 + rng.standard_normal(shape[:3])).astype(np.float32)
            if first:
                l[1:3], o[1:3], first = -np.inf, 0.0, False
            members.append((o, l))
        groups.append((f32, members))
    return groups


class _KvqEntry:
    """the loaded library with hyd_suffix_attn_fwd bound to the fp8 entry point: suffix_fwd_with_partials then hands its partials to
    the fp8 kernel (fill_suffix_params marshals fp8 caches as they are: strides count bytes)"""

    def __init__(self, lib, kq):
        self._lib, self._kq = lib, kq

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def hyd_suffix_attn_fwd(self, sp, stream):
        return self._lib.hyd_suffix_attn_fwd_kvq(sp, C.byref(self._kq), stream)


def _no_fallback(*a, **k):
    raise AssertionError("dequantize_kv reached: the fp8 call fell back to the 16-bit path")


def _run(name, kind, shape, dt, D, extra, sc):
    """-> (out, lse or None) of the case, on the device"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    causal = kind == "causal"
    if causal:
        T, Hq, Hkv, cap, _, route = CAUSAL_SHAPES[shape]
        sl = lengths(cap)
        assert causal_route(len(sl), Hq, Hkv, cap, D, T) == route, name
    else:
        Hq, Hkv, T, cap, _, route, hpw = SHAPES[shape]
        sl = lengths(cap)
    B = len(sl)
    q = _normal(rng, dt, B, T, Hq, D)
    k, v = _caches(rng, sl, cap, Hkv, D, dt, sc is not None)
    tsl = torch.from_numpy(sl).to(DEV)
    ks, vs = (None, None) if sc is None else (None if s is None else s.to(DEV) for s in fp8_scales(sc, Hkv))
    if sc is not None:
        assert F.fp8_native(q, k, v), name
    if kind == "levels":
        levels = [(_normal(rng, dt, sb, P, Hkv, D), _normal(rng, dt, sb, P, Hkv, D)) for sb, P in extra]
        if len(levels) == 1:  # the one-launch form (api_attn.hip decode_runs_as_one_launch): both segments count for gqa_few_units
            P = extra[0][1]
            assert B * Hkv * (P + cap) <= ONE_LAUNCH_MAX_KEYS, name
            assert suffix_route(B, Hq, Hkv, cap + P, D, T) == ("gqa/4-waves" if P == 160 else "gqa/1-wave"), name
        else:  # every level is small (<= 64 query rows per group and kv head, <= 1024 keys): the grouped-query kernel, one wave
            assert all(B // sb * (Hq // Hkv) <= 64 and P < 128 for sb, P in extra) and suffix_route(B, Hq, Hkv, cap, D, T) == route, name
        return hydragen_attention_nopad(q, k, v, [x for x, _ in levels], [x for _, x in levels], tsl), None
    if not causal:
        assert suffix_route(B, Hq, Hkv, cap, D, T) == route and (route != "gqa/1-wave" or _hpw(Hkv, D) == hpw), name
    with mock.patch.object(F, "dequantize_kv", _no_fallback):
        if extra is None:
            return flash_attention_seqlen(q, k, v, tsl, k_scale=ks, v_scale=vs, causal_tail=causal)
        groups = _groups(rng, extra, (B, T, Hq, D), dt)
        if sc is None:
            return suffix_fwd_with_partials(q, k, v, tsl, groups, dt, PARTIALS[extra][1], causal=causal)
        with mock.patch.object(_lib, "load", lambda lib=_lib.load(): _KvqEntry(lib, F.kv_quant_params(ks, vs))):
            return suffix_fwd_with_partials(q, k, v, tsl, groups, dt, PARTIALS[extra][1])


def _crcs(t):
    rows = t.contiguous().view(torch.uint8).reshape(t.shape[0], -1).cpu().numpy()
    return [zlib.crc32(r.tobytes()) for r in rows]


def outputs() -> dict:
    """family -> uint32 [cases, 2 (out, lse), BMAX], and family + "/names" -> the case names in the same order"""
    got = {}
    for fam in FAMILIES:
        names = [name for name, f, _ in CASES if f == fam]
        crc = np.zeros((len(names), 2, BMAX), dtype=np.uint32)
        for i, (name, f, args) in enumerate(c for c in CASES if c[1] == fam):
            out, lse = _run(name, *args)
            torch.cuda.synchronize()
            crc[i, 0, : out.shape[0]] = _crcs(out)
            if lse is not None:
                crc[i, 1, : out.shape[0]] = _crcs(lse)
        got[fam], got[fam + "/names"] = crc, np.array(names, dtype=np.bytes_)
    return got


@functools.lru_cache(maxsize=1)
def _got():
    return outputs()


@functools.lru_cache(maxsize=1)
def _want():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case_and_nothing_else():
    want = _want()
    assert sorted(want) == sorted([f for f in FAMILIES] + [f + "/names" for f in FAMILIES])
    for fam in FAMILIES:
        names = [name for name, f, _ in CASES if f == fam]
        assert [n.decode() for n in want[fam + "/names"]] == names, fam
        assert want[fam].shape == (len(names), 2, BMAX) and want[fam].dtype == np.uint32, fam
    assert len(CASES) == len({name for name, _, _ in CASES}) == 2 * (10 + 20 + 9 + 2 * (1 + 2 + 6 * 3 + 6 * 4))
    assert GOLDEN.stat().st_size < 64 * 1024


@pytest.mark.parametrize("family", FAMILIES)
def test_gqa_suffix_kernels_return_the_recorded_bytes(family):
    got, want = _got()[family], _want()[family]
    names = [name for name, f, _ in CASES if f == family]
    differ = [(names[i], ("out", "lse")[t], b) for i, t, b in zip(*np.nonzero(got != want))]
    assert not differ, f"(case, tensor, batch row) whose bytes differ from the recording: {differ}"


def test_the_rows_exercise_what_they_are_there_for():
    """on the recording itself: every row that attends to something has bytes of its own, and the empty sequence without partials
    is zeros with lse = -inf -- a fixture of trivial rows would compare equal whatever the kernels did"""
    want = _want()
    for fam in FAMILIES:
        for (name, _, (kind, shape, dt, D, extra, sc)), crc in zip((c for c in CASES if c[1] == fam), want[fam]):
            if kind == "causal":
                T, Hq, _, cap = CAUSAL_SHAPES[shape][:4]
            else:
                Hq, _, T, cap = SHAPES[shape][:4]
            sl = lengths(cap)
            B = len(sl)
            assert not crc[:, B:].any(), name
            merge_only = kind == "levels" or extra not in (None, "none")  # the empty sequence still has partials to merge
            full = [b for b in range(B) if sl[b] > 0 or merge_only]
            assert len(set(crc[0, full].tolist())) == len(full), name
            want_lse = kind != "levels" and (extra is None or PARTIALS[extra][1])
            assert bool(crc[1, :B].all()) == want_lse and (want_lse or not crc[1].any()), name
            if want_lse:
                assert len(set(crc[1, [b for b in range(B) if sl[b] > 0]].tolist())) == int((sl > 0).sum()), name
                assert crc[1, 0] == zlib.crc32(np.full(T * Hq, -np.inf, np.float32).tobytes()), name
            if not merge_only:
                assert sl[0] == 0 and crc[0, 0] == zlib.crc32(bytes(T * Hq * D * 2)), name


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    path = Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN
    np.savez_compressed(path, **outputs())
    print(f"recorded {len(CASES)} cases in {path} ({path.stat().st_size} bytes)")
