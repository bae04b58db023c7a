"""-m gpu: the RoPE + append preamble writes the very bits it wrote while rope_append.hip held seven hand-kept kernel bodies.  Every
element is a handful of fp32 products with one rounding (and, for fp8 caches, one correctly rounded divide), so a kernel rebuilt on
shared text gives identical bytes unless a product was contracted differently, a guard moved or a store went astray: the comparison
has no tolerance.

tests/golden/rope_append_parent.npz holds what the seven bodies wrote, recorded by this module's own `outputs()`:

    python -m tests.test_rope_append_golden_gpu --record [PATH]

The inputs are not stored: q / k / v (views of one fused projection buffer) and the norm gains are normal values from
numpy.random.default_rng seeded by the case's name, the cos / sin tables are computed here in float64 and rounded to float32.  What
is stored, per case: a zlib.crc32 per output (q_out, the whole k_cache, the whole v_cache, seq_lens) and batch row.  The caches hold
a non-zero byte pattern before each call, so a stray or a missing write changes a checksum.

One case per instantiation and route: {f16, bf16} x D {64, 128, 256} x {plain, fp8 with mixed scales, fp8 with null scales, T = 3,
T = 8, norm, norm + fp8, norm + T = 3}, and the narrow kernel on (d, D) = (80, 128), (96, 128), (192, 256).  B = 6, Hq = 4,
Hkv = 2, a cache of 4 tokens: 48 rows per token = 192 / 384 / 768 threads (x T), so the last block is ragged at every D.  The six
rows sit at cache index -1 (a retired row), 0, 3 (the last slot), 4 (= cache_len: no K/V write), 2 (a multi-token row crosses the
cache's end) and, with a small shared length, at a position beyond the table (clamped table row, no K/V write)."""
import functools
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from hydragen_amd.fused_decode import rope_append_decode, rope_append_multi
from tests.glue_ref import fp8_scales

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden" / "rope_append_parent.npz"
B, HQ, HKV, L, MAX_POS, EPS = 6, 4, 2, 4, 32, 1e-6
SHARED = np.array([5, 7, 3, 9, 6, 2], dtype=np.int64)
INDEX = np.array([-1, 0, 3, 4, 2, MAX_POS + 1 - 2], dtype=np.int64)  # the cache index of the row's (first) token
POS = SHARED + INDEX                                                 # the last one is MAX_POS + 1: beyond the table
TENSORS = ("q_out", "k_cache", "v_cache", "seq_lens")
DT = dict(f16=torch.float16, bf16=torch.bfloat16)
# family -> (tokens per row, norm, fp8 scale mode or None)
FAMILIES = dict(plain=(1, False, None), fp8_mixed=(1, False, "mixed"), fp8_null=(1, False, "none"), multi3=(3, False, None),
                multi8=(8, False, None), norm=(1, True, None), norm_fp8=(1, True, "mixed"), norm_multi3=(3, True, None))
NARROW = ((80, 128), (96, 128), (192, 256))
CASES = [(f"{fam}/{dt}/{D}", fam, dt, D) for fam in FAMILIES for dt in DT for D in (64, 128, 256)]
CASES += [(f"narrow/{dt}/{d}in{D}", "narrow", dt, d) for dt in DT for d, D in NARROW]


def _tables(d):
    """HF rotate-half tables [MAX_POS, d]: float64 arithmetic, rounded to float32"""
    inv = 10000.0 ** (-np.arange(0, d, 2, dtype=np.float64) / d)
    ang = np.arange(MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    ang = np.concatenate([ang, ang], 1)
    return torch.from_numpy(np.cos(ang).astype(np.float32)).to(DEV), torch.from_numpy(np.sin(ang).astype(np.float32)).to(DEV)


def _prefill(which, itemsize, d):
    """the bytes a cache holds before the call: [B, L * HKV * d * itemsize] uint8, never 0, different for K and V"""
    n = B * L * HKV * d * itemsize
    return ((np.arange(n, dtype=np.int64) * (37 + 2 * which) + 11) % 251 + 1).astype(np.uint8).reshape(B, -1)


def _run(name, fam, dt, d):
    """-> the four outputs of the case as CPU uint8 arrays [B, bytes per batch row]"""
    T, norm, fp8 = FAMILIES.get(fam, (1, False, None))
    dtype = DT[dt]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    qkv = torch.from_numpy(rng.standard_normal((B, T, (HQ + 2 * HKV) * d), dtype=np.float32)).to(dtype).to(DEV)
    q = qkv[..., : HQ * d].view(B, T, HQ, d)
    k = qkv[..., HQ * d: (HQ + HKV) * d].view(B, T, HKV, d)
    v = qkv[..., (HQ + HKV) * d:].view(B, T, HKV, d)
    kw = {}
    if norm:
        gains = [torch.from_numpy((1 + 0.3 * rng.standard_normal(d)).astype(np.float32)).to(dtype).to(DEV) for _ in range(2)]
        kw = dict(q_norm=gains[0], k_norm=gains[1], norm_eps=EPS)
    cdtype = torch.float8_e4m3fn if fp8 else dtype
    kc, vc = (torch.from_numpy(_prefill(i, cdtype.itemsize, d)).to(DEV).view(cdtype).view(B, L, HKV, d) for i in range(2))
    if fp8:
        ks, vs = fp8_scales(fp8, HKV)
        if ks is not None:
            kw.update(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    cos, sin = _tables(d)
    pos, shared = torch.from_numpy(POS).to(DEV)[:, None].contiguous(), torch.from_numpy(SHARED).to(DEV)
    if T == 1:
        q_out, seq_lens = rope_append_decode(q, k, v, cos, sin, pos, shared, kc, vc, **kw)
    else:
        q_out, seq_lens = rope_append_multi(q, k, v, cos, sin, pos, shared, kc, vc, **kw)
    torch.cuda.synchronize()
    return [t.contiguous().view(torch.uint8).reshape(B, -1).cpu().numpy() for t in (q_out, kc, vc, seq_lens)]


def _crcs(rows):
    return np.array([zlib.crc32(r.tobytes()) for r in rows], dtype=np.uint32)


def outputs() -> dict:
    """case name -> uint32 [len(TENSORS), B]: the checksum of every output's every batch row"""
    return {name: np.stack([_crcs(t) for t in _run(name, fam, dt, d)]) for name, fam, dt, d in CASES}


@functools.lru_cache(maxsize=1)
def _got():
    return outputs()


@functools.lru_cache(maxsize=1)
def _want():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_case_and_nothing_else():
    want = _want()
    assert sorted(want) == sorted(name for name, *_ in CASES) and len(want) == 2 * 3 * 8 + 2 * 3
    for k, v in want.items():
        assert v.shape == (len(TENSORS), B) and v.dtype == np.uint32, k
    assert GOLDEN.stat().st_size < 64 * 1024


@pytest.mark.parametrize("family", list(FAMILIES) + ["narrow"])
def test_rope_append_writes_the_recorded_bytes(family):
    got, want = _got(), _want()
    differ = [(name, TENSORS[t], b) for name, fam, _, _ in CASES if fam == family
              for t, b in zip(*np.nonzero(got[name] != want[name]))]
    assert not differ, f"(case, tensor, batch row) whose bytes differ from the recording: {differ}"


def test_the_rows_exercise_what_they_are_there_for():
    """on the recording itself: the rows that must not append left the caches' pattern alone, the others changed it, and seq_lens
    follows each form's rule -- a fixture of trivial rows would compare equal whatever the kernel did"""
    want = _want()
    for name, fam, dt, d in CASES:
        T, _, fp8 = FAMILIES.get(fam, (1, False, None))
        q_out, kc, vc, sl = want[name]
        for which, got in ((0, kc), (1, vc)):
            untouched = _crcs(_prefill(which, 1 if fp8 else 2, d)) == got
            assert untouched.tolist() == [True, False, False, True, False, True], (name, which)
        lens = INDEX + 1 if T == 1 else np.where(INDEX >= 0, INDEX + T, 0)
        assert (sl == _crcs(lens.astype(np.int32)[:, None])).all(), name
        assert len(set(q_out.tolist())) == B, name


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], __doc__
    path = Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN
    np.savez_compressed(path, **outputs())
    print(f"recorded {len(CASES)} cases in {path} ({path.stat().st_size} bytes)")
