"""CPU side of the head-geometry tests: the magic-number division the prefix pass decodes its rows with, the float64 oracles on
the head counts the GPU tests lean on them for, and the case table's coverage of the head-count branches."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import hydragen_oracle as O
from tests import head_geometry_cases as HG

CSRC = Path(__file__).resolve().parents[1] / "hydragen_amd" / "csrc"

FASTDIV_PROGRAM = r"""
#include <cstdio>
#include "hyd_kernels.h"
// q = (t + ((n - t) >> sh1)) >> sh2 with t = mulhi(mul, n), as hyd_kernels.h documents it and prefix_unit_w64.h evaluates it
static inline uint32_t fdiv(uint32_t n, const hyd::FastDiv& f) {
    const uint32_t t = (uint32_t)(((uint64_t)f.mul * n) >> 32);
    return (t + ((n - t) >> (f.sh & 0xffu))) >> (f.sh >> 8);
}
static unsigned long long checks = 0, failures = 0;
static inline void check(uint32_t n, uint32_t d, const hyd::FastDiv& f) {
    ++checks;
    if (fdiv(n, f) != n / d && failures++ < 10) printf("FAIL n=%u d=%u got %u want %u\n", n, d, fdiv(n, f), n / d);
}
static void edges(uint32_t d, const hyd::FastDiv& f) {
    // multiples of d and their neighbours along a geometric ladder of k up to 2^32, then the ends of the range
    for (uint64_t k = 1; k <= (uint64_t(1) << 32); k += k / 2 + 1)
        for (int64_t e = -2; e <= 2; ++e) {
            const int64_t n = (int64_t)(k * d) + e;
            if (n >= 0 && n <= 0xffffffffLL) check((uint32_t)n, d, f);
        }
    const uint32_t ends[4] = {0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t n : ends) check(n, d, f);
}
int main() {
    for (uint32_t d = 1; d <= 5000; ++d) {
        const hyd::FastDiv f = hyd::make_fastdiv(d);
        for (uint32_t n = 0; n < 70000; ++n) check(n, d, f);
        edges(d, f);
    }
    const uint32_t big[7] = {65535u, 65536u, 65537u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
    for (uint32_t d : big) {
        const hyd::FastDiv f = hyd::make_fastdiv(d);
        for (uint32_t n = 0; n < 70000; ++n) check(n, d, f);
        edges(d, f);
    }
    printf("checks %llu failures %llu\n", checks, failures);
    return failures ? 1 : 0;
}
"""


def test_fastdiv_is_exact(tmp_path):
    """hyd_kernels.h: FastDiv is "exact for every 32-bit n and d >= 1".  The header's own make_fastdiv, evaluated on the host:
    every d in 1..5000 over n in 0..69999 (the row, unit and split counts the prefix pass divides), k d + {-2..2} along a
    geometric ladder of k up to 2^32, the ends of the 32-bit range, and divisors around 2^16, 2^31 and 2^32."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    src, exe = tmp_path / "fastdiv_check.cpp", tmp_path / "fastdiv_check"
    src.write_text(FASTDIV_PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checks" and int(last[1]) >= 350_000_000 and int(last[3]) == 0, run.stdout[-500:]


def _both_oracles(case):
    a = O.hydragen_attention(case["q"], case["k"], case["v"], case["shared_ks"], case["shared_vs"], case["shared_cu_seq_lens"],
                             case["shared_max_seq_lens"], case["use_varlens"], case["seq_lens"])
    b = O.nosharing_attention(case["q"], case["k"], case["v"], case["shared_ks"], case["shared_vs"], case["shared_cu_seq_lens"],
                              case["use_varlens"], case["seq_lens"])
    return a, b


@pytest.mark.parametrize("cid,sizes,geom,D", HG.operator_cases(), ids=[c[0] for c in HG.operator_cases()])
def test_decomposed_oracle_equals_the_undecomposed_one(cid, sizes, geom, D):
    """The reference the GPU tests compare against is itself right on these head counts: the decomposed float64 operator and
    plain attention over each sequence's concatenated keys agree to 1e-12 on every hierarchy and geometry of section C."""
    a, b = _both_oracles(HG.operator_case(sizes, geom, D, "f16"))
    assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-12


# ---- the table covers every head-count branch ------------------------------------------------------------------------------------
def _g(geom):
    hq, hkv = HG.heads(geom)
    return hq // hkv


def _hpw(geom, D):  # suffix_gqa_common.h gqa_launch_plan, one-wave units
    hkv = HG.heads(geom)[1]
    hpw = 1 if hkv > 8 else 4 if hkv % 4 == 0 else 2 if hkv % 2 == 0 else 1
    return min(hpw, 2) if D == 256 else hpw


def test_every_geometry_is_grouped_evenly():
    assert len(HG.GEOMETRIES) == 20
    for name, (hq, hkv) in HG.GEOMETRIES.items():
        assert hq % hkv == 0, name
    lists = [HG.A1_CASES, HG.B1_CASES, HG.B2_CASES, HG.B4_CASES, HG.B5_CASES, HG.C_GEOMS]
    for geom, D in (c for l in lists for c in l):
        hq, hkv = HG.heads(geom)
        assert hq % hkv == 0 and D in (64, 128, 256), (geom, D)


def test_table_reaches_every_head_count_branch():
    # prefix pass: odd divisors for the row decode, rows of one token on both sides of a 128-row block, every odd split count
    assert {3, 7, 12, 71} <= {_g(g) for g, _ in HG.A1_CASES}
    assert {3, 5, 10} <= {HG.heads(g)[1] for g, _ in HG.A1_CASES}
    assert any(128 % _g(g) != 0 and HG.a1_sq(g) * _g(g) > 128 for g, _ in HG.A1_CASES)
    assert set(HG.A2_SPLITS) == {3, 5, 6, 7} and all(-(-HG.a2_sk(ns) // 128) == ns for ns in HG.A2_SPLITS)
    assert -(-HG.A4_SQ * _g(HG.A4_GEOM) // 128) * HG.heads(HG.A4_GEOM)[1] > 256  # more 128-row units than the chip has CUs
    assert -(-HG.A4_SQ * _g(HG.A4_GEOM) // 256) * HG.heads(HG.A4_GEOM)[1] == HG.A4_GRID
    assert HG.A5_B // HG.A5_SB > 1 and any(_g(g) % 2 for g in HG.A5_GEOMS)
    # grouped-query kernel: 1, 2 and 4 heads per workgroup, Hkv > 8, a ragged last 16-row chunk, nq > 1 with odd g
    assert all(_g(g) >= 3 for g, _ in HG.B1_CASES + HG.B2_CASES)
    assert {_hpw(g, D) for g, D in HG.B1_CASES} == {1, 2, 4}
    assert any(HG.heads(g)[1] > 8 for g, _ in HG.B1_CASES)
    assert any(HG.heads(g)[1] == 8 and D == 256 for g, D in HG.B1_CASES)  # capped at 2 heads per workgroup
    assert any(_g(g) > 16 and _g(g) % 16 for g, _ in HG.B1_CASES)
    assert any(nq > 1 and _g(g) % 2 and nq * _g(g) > 16 and (nq * _g(g)) % 16 for g, nq in HG.B3_CASES)
    assert any(12 % 8 and _g(g) == 12 and D == 256 for g, D in HG.B2_CASES)  # dot-product kernel, 8-row chunks, a ragged second one
    # token-row kernel: 3, 5 and 6 waves per sequence, each head count a whole number of wave instructions
    assert all(_g(g) == 1 and HG.heads(g)[1] % (64 // (D // 8)) == 0 for g, D in HG.B4_CASES)
    assert {3, 5, 6} <= {HG.heads(g)[1] // (64 // (D // 8)) for g, D in HG.B4_CASES}
    assert HG.B4_S < 64 and HG.B1_S < 128 <= HG.B2_S
    # one-unit-per-wave kernel: never a whole number of wave instructions when g = 1; idle lane groups on the packed path
    # (D = 128, Hkv >= 4, Hkv % 4 != 0); a shape below the packed threshold; a ragged last workgroup of 4 units
    assert all(_g(g) <= 2 and (_g(g) == 2 or HG.heads(g)[1] % (64 // (D // 8))) for g, D in HG.B5_CASES)
    assert {5, 6, 7} <= {HG.heads(g)[1] for g, D in HG.B5_CASES if D == 128 and _g(g) == 1 and HG.heads(g)[1] >= 4}
    assert any(HG.heads(g)[1] < 4 and D == 128 and _g(g) == 1 for g, D in HG.B5_CASES)
    assert any(HG.heads(g)[1] > 4 and HG.heads(g)[1] % 4 for g, _ in HG.B5_CASES)
    lens = HG.b5_lens(*HG.B5_FORMS["one-wave"])
    assert (lens <= 12).any() and (lens > 12).any() and (lens == 0).any()
    # fp8: native shapes are grouped-query or token-row shapes, the fallback ones neither
    assert all(_g(g) >= 3 or HG.heads(g)[1] % 4 == 0 for g, _, _ in HG.D_NATIVE)
    assert all(_g(g) == 1 and HG.heads(g)[1] % 4 for g, _, _ in HG.D_FALLBACK)
    # operator: a level above the small-level limit of 64 rows per (group, kv head)
    assert any(len(HG.C_HIERARCHIES["prefix-kernel"][-1]) * _g(g) > 64 for g, _ in HG.C_GEOMS)


def test_blame_rows_names_a_head_mixup():
    rng = np.random.default_rng(0)
    want = rng.standard_normal((2, 1, 6, 8))
    got = want.copy()
    got[1, 0, 4] = want[1, 0, 2]
    text = HG.blame_rows(got, want, 1e-6)
    assert "1 of 12 rows" in text and "(b=1, iq=0, head=4)" in text and "[(1, 0, 2)]" in text
    assert HG.blame_rows(want, want, 1e-6) == "no row exceeds the bound"
