"""-m gpu: the suffix kernels and the LSE merges on adversarial score and LSE patterns (tests/softmax_stress_cases.py), `out` AND
`lse` against the float64 oracle.  Random normal data never makes the running maximum rise late, never leaves a worker (wave, lane
group, token-split slice) with a negligible or an empty state, never lets a weight underflow and never puts a finite giant behind
a sequence's length; these inputs do, on every route the launchers pick -- token-row kernel (4 waves per sequence, token split 2
and 4, unsplit, NPRE = 2), one-unit-per-wave kernel (four waves per unit, R = 2, R = 4, the packed lane-group body), grouped-query
kernel (one and four waves per unit), D = 64 and 256, both fp8 kernels -- and on `combine.hip`.  The bounds are the suite's existing
ones; tests/test_softmax_stress.py shows that the reference's own rounding model meets them on these inputs with twofold room.
Every test prints its largest error / bound ratios (`-s` shows them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hydragen_oracle as O
from tests import softmax_stress_cases as S
from tests.gpu_util import ATOL, REL_L2, assert_close_l2, atol, dev, suffix_fwd_with_partials

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ratios(got, want, dt):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = ATOL["f16"] * max(1.0, float(np.abs(want).max())) if dt == "f16" else atol(dt, want)
    l2 = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    return max(np.abs(got - want).max() / bound, l2 / REL_L2[dt])


def _check_out(got, want, dt, what):
    r = _ratios(got, want, dt) if got.size else 0.0
    print(f"stress-ratio out {what}: {r:.3f}")
    assert_close_l2(got, want, dt, what)


def _check_lse(gl, wl, what):
    """|lse - want| <= 2e-3 + 1e-5 |want|: the bound of the prefix pass's adversarial tests (tests/test_edge_gpu.py)"""
    bound = 2e-3 + 1e-5 * np.abs(wl)
    r = float((np.abs(gl - wl) / bound).max()) if gl.size else 0.0
    print(f"stress-ratio lse {what}: {r:.3f}")
    assert np.isfinite(gl).all() and (np.abs(gl - wl) <= bound).all(), f"{what}: lse off by {np.abs(gl - wl).max():.3e}"


def _tile(x, B, dt=None):
    """a built block on the device, repeated to the route's batch (softmax_stress_cases.block_index)"""
    t = dev(x, dt)
    return t if t.shape[0] == B else t[torch.from_numpy(S.block_index(B)).to(DEV)].contiguous()


def _full(x, B):
    return x if x.shape[0] == B else x[S.block_index(B)]


# ---- a. the suffix pass on its own --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pattern", S.SCORE_PATTERNS)
@pytest.mark.parametrize("route", list(S.SUFFIX_ROUTES))
def test_suffix_kernels_on_adversarial_scores(route, pattern, dt):
    from hydragen_amd.flash import flash_attention_seqlen

    B, Hq, nq = S.SUFFIX_ROUTES[route][0], S.SUFFIX_ROUTES[route][1], S.SUFFIX_ROUTES[route][5]
    c = S.score_case(route, pattern, dt)
    tq, tk, tv, tsl = _tile(c["q"], B, dt), _tile(c["k"], B, dt), _tile(c["v"], B, dt), _tile(c["lens"], B)
    out, lse = flash_attention_seqlen(tq, tk, tv, seq_len=tsl)
    torch.cuda.synchronize()
    want, wlse = O.flash_attention_seqlen(c["q"], c["k"], c["v"], c["lens"])
    got, gl = out.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(got).all()
    nz = _full(c["lens"], B) > 0  # attention over zero keys is undefined; the kernel returns 0 / -inf there (tests/test_fuzz_gpu.py)
    want, wlse = _full(want, B), _full(wlse, B)
    what = f"{route} {pattern} {dt}"
    _check_out(got[nz], want[nz], dt, what)
    _check_lse(gl[nz], wlse[nz], what)
    assert not got[~nz].any() and np.all(np.isneginf(gl[~nz]))
    if pattern == "spike_behind_length":  # the giants behind the length against zeros there: not one bit may move
        out0, lse0 = flash_attention_seqlen(tq, _tile(S.zero_behind_length(c["k"], c["lens"]), B, dt), tv, seq_len=tsl)
        assert torch.equal(out0.view(torch.int16), out.view(torch.int16)) and torch.equal(lse0.view(torch.int32), lse.view(torch.int32))
    if pattern == "ties":
        cf, cl = S.ties_closed_form(c["v"], c["lens"], Hq, nq)
        _check_out(got[nz], _full(cf, B)[nz], dt, what + " closed form")
        _check_lse(gl[nz], _full(cl, B)[nz], what + " closed form")


# ---- b. the same through the fp8 kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pattern", S.FP8_SCORE_PATTERNS)
@pytest.mark.parametrize("route", list(S.FP8_ROUTES))
def test_fp8_suffix_kernels_on_adversarial_scores(monkeypatch, route, pattern, dt):
    """Bounds as tests/test_fp8_kv_gpu.py::test_suffix_fp8_matches_oracle_on_dequantized_caches and
    tests/test_fp8_gqa_gpu.py::test_fp8_gqa_matches_oracle_on_dequantized_caches have them: `out` by gpu_util.assert_close_l2 (the
    16-bit gates: the widening is exact), `lse` by np.allclose(atol=2e-3, rtol=1e-4); the reference is the oracle on
    kv_quant.dequantize_kv of the same bytes.  flash.dequantize_kv is patched to raise, as in test_fp8_gqa_gpu.py: no fallback."""
    from hydragen_amd import flash as F
    from hydragen_amd.kv_quant import FP8_DTYPE, dequantize_kv

    B = S.FP8_ROUTES[route][0]
    c = S.fp8_score_case(route, pattern, dt)
    k8, v8 = _tile(c["k8"], B).to(FP8_DTYPE), _tile(c["v8"], B).to(FP8_DTYPE)
    assert torch.equal(k8[:len(c["lens"])].float().cpu(), torch.from_numpy(c["k8"]))  # the cache holds the stated values exactly
    ks, vs = dev(c["k_scale"]), dev(c["v_scale"])
    tq, tsl = _tile(c["q"], B, dt), _tile(c["lens"], B)
    nb = len(c["lens"])
    kd, vd = dequantize_kv(k8[:nb], ks, torch.float32).cpu().numpy(), dequantize_kv(v8[:nb], vs, torch.float32).cpu().numpy()

    def raiser(*a, **k):
        raise AssertionError("dequantize_kv reached: the fp8 call fell back to the 16-bit path")

    def call(k):
        with monkeypatch.context() as m:
            m.setattr(F, "dequantize_kv", raiser)
            o, l = F.flash_attention_seqlen(tq, k, v8, tsl, k_scale=ks, v_scale=vs)
        torch.cuda.synchronize()
        return o, l

    out, lse = call(k8)
    want, wlse = O.flash_attention_seqlen(c["q"], kd, vd, c["lens"])
    got, gl = out.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(got).all()
    nz = _full(c["lens"], B) > 0
    want, wlse = _full(want, B), _full(wlse, B)
    what = f"{route} {pattern} {dt}"
    _check_out(got[nz], want[nz], dt, what)
    r = float((np.abs(gl[nz] - wlse[nz]) / (2e-3 + 1e-4 * np.abs(wlse[nz]))).max())
    print(f"stress-ratio lse {what}: {r:.3f}")
    assert np.all(np.isneginf(gl[~nz])) and np.allclose(gl[nz], wlse[nz], atol=2e-3, rtol=1e-4), what
    if pattern == "spike_behind_length":
        z8 = _tile(S.zero_behind_length(c["k8"], c["lens"]), B).to(FP8_DTYPE)
        out0, lse0 = call(z8)
        assert torch.equal(out0.view(torch.int16), out.view(torch.int16)) and torch.equal(lse0.view(torch.int32), lse.view(torch.int32))


# ---- c. hand-made partials into hyd_suffix_attn_fwd ----------------------------------------------------------------------------
def _run_merge(c, route, dt, what, causal=False):
    B = c["B"]
    groups, at = [], 0
    for kind, cnt in c["parts"]:
        groups.append((kind != "h", [(_full(c["outs"][i], B), _full(c["lses"][i], B)) for i in range(at, at + cnt)]))
        at += cnt
    tq, tk, tv, tsl = _tile(c["q"], B, dt), _tile(c["k"], B, dt), _tile(c["v"], B, dt), _tile(c["lens"], B)
    ok, want, slse = _full(c["ok"], B), _full(c["want"], B), _full(c["suffix_lse"], B)
    fin = np.isfinite(slse)
    for want_lse in (False, True):
        out, lse = suffix_fwd_with_partials(tq, tk, tv, tsl, groups, dt, want_lse, causal)
        got = out.float().cpu().numpy()
        assert np.isfinite(got).all(), what
        if ok.any():
            _check_out(got[ok], want[ok], dt, f"{what} want_lse={want_lse}")
        assert not got[~ok].any(), f"{what}: a row with nothing to attend to must be exactly 0"
        if want_lse:  # the suffix pass's OWN log-sum-exp, whatever was merged into `out`
            gl = lse.cpu().numpy()
            if fin.any():
                _check_lse(gl[fin], slse[fin], what)
            assert np.all(np.isneginf(gl[~fin])), what
    return got


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pattern", S.LSE_PATTERNS)
@pytest.mark.parametrize("route", list(S.PARTIAL_ROUTES))
def test_suffix_kernels_merge_partials_on_adversarial_lses(route, pattern, dt):
    """Partials of every kind (16-bit, fp32, stacked fp32 slices: the marshalling of tests/test_suffix_partials_gpu.py) whose LSEs
    follow an LSE pattern, with and without the suffix pass's own LSE requested, against O.combine_lse of the stated partials and
    the oracle's suffix attention.  `ties` runs 1, 2, 3, 5, 6 and 7 partials: the last batch of finish_row (NBATCH 2 on the
    token-row kernel, 4 on the one-unit-per-wave kernel) is then partial, and a clamped duplicate given weight moves the mean."""
    lead = S.PARTIAL_ROUTES[route][4]
    for n in (S.TIES_COUNTS if pattern == "ties" else (None,)):
        if n is not None and n < lead:
            continue  # (fewer partials than the route prefetches: another route)
        c = S.merge_case(route, pattern, dt, n)
        got = _run_merge(c, route, dt, f"{route} {pattern} n={n} {dt}")
        if pattern == "ties":
            mean = (np.sum([o.astype(np.float64) for o in c["outs"]], 0) + c["suffix_out"]) / (len(c["outs"]) + 1)
            _check_out(got, _full(mean, c["B"]), dt, f"{route} ties n={n} {dt}: arithmetic mean")
        if pattern == "all_empty":
            assert not got.any()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("route", list(S.PARTIAL_ROUTES))
def test_far_apart_partials_over_a_negligible_suffix(route, dt):
    """far_apart LSEs on far_below scores: the suffix pass's own state (LSE about -41) is the negligible one of the merge"""
    c = S.merge_case(route, "far_apart", dt, scores="far_below")
    _run_merge(c, route, dt, f"{route} far_apart on far_below {dt}")


# ---- c2. the causal tail: a per-row key limit in the score mask -----------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pattern", S.CAUSAL_PATTERNS)
@pytest.mark.parametrize("route", list(S.CAUSAL_ROUTES))
def test_causal_tail_kernels_on_adversarial_scores(route, pattern, dt):
    """hyd_suffix_attn_causal_fwd on every route of CAUSAL_ROUTES: the score patterns laid out by the sequence's length (so that
    last_key_spike is a giant behind the limit of every token but the last), tail_staircase and giants_behind_row_limit, at lengths
    whose limits land on, before and after the tile and wave boundaries, with 0 < len < T, len > kv_len and len < 0."""
    from hydragen_amd.flash import flash_attention_seqlen

    B, Hq, Hkv, cap, D, T = S.causal_shape(route)
    c = S.causal_case(route, pattern, dt)
    tq, tk, tv, tsl = _tile(c["q"], B, dt), _tile(c["k"], B, dt), _tile(c["v"], B, dt), _tile(c["lens"], B)
    assert tuple(tq.shape) == (B, T, Hq, D) and tuple(tk.shape) == (B, cap, Hkv, D)
    out, lse = flash_attention_seqlen(tq, tk, tv, seq_len=tsl, causal_tail=True)
    torch.cuda.synchronize()
    want, wlse = S.causal_reference(c["q"], c["k"], c["v"], c["lens"])
    got, gl = out.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(got).all() and not np.isnan(gl).any()
    has = _full(c["lim"], B) > 0  # [B, T]: the (sequence, token) pairs with a visible key
    want, wlse = _full(want, B), _full(wlse, B)
    what = f"causal {route} {pattern} {dt}"
    _check_out(got[has], want[has], dt, what)
    _check_lse(gl[has], wlse[has], what)
    # no visible key (length <= 0, and the first tokens of a sequence shorter than the step): exact zeros, lse = -inf
    assert (~has).any() and not got[~has].any() and np.all(np.isneginf(gl[~has])), what
    for dst, src in c["twins"]:  # length cap + 3 is length cap, length -2 is length 0: the same data, the same bits
        assert torch.equal(_bits(out[dst]), _bits(out[src])) and torch.equal(_bits(lse[dst]), _bits(lse[src])), (what, dst, src)
    n_of = np.clip(c["lens"], 0, cap)
    if pattern in ("spike_behind_length", "tail_staircase"):  # the giants behind the length against zeros there: not one bit may move
        out0, lse0 = flash_attention_seqlen(tq, _tile(S.zero_behind_length(c["k"], n_of), B, dt), tv, seq_len=tsl, causal_tail=True)
        assert torch.equal(_bits(out0), _bits(out)) and torch.equal(_bits(lse0), _bits(lse)), what
    if pattern == "giants_behind_row_limit":  # ... and behind token 0's limit: this step's draft keys are nothing to token 0
        out0, lse0 = flash_attention_seqlen(tq, _tile(S.zero_from(c["k"], c["lim"][:, 0]), B, dt), tv, seq_len=tsl, causal_tail=True)
        assert torch.equal(_bits(out0[:, 0]), _bits(out[:, 0])) and torch.equal(_bits(lse0[:, 0]), _bits(lse[:, 0])), what
    if pattern == "ties":  # every token's key count, exactly
        cf, cl = S.causal_ties_closed_form(c["v"], c["lim"], Hq)
        _check_out(got[has], _full(cf, B)[has], dt, what + " closed form")
        _check_lse(gl[has], _full(cl, B)[has], what + " closed form")
    if pattern == "tail_staircase":  # token i returns v[len - T + i]: a limit off by one key returns another row
        _check_out(got[has], _full(S.staircase_closed_form(c["v"], c["lim"], Hq), B)[has], dt, what + " closed form")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pattern", S.CAUSAL_LSE_PATTERNS)
@pytest.mark.parametrize("route", S.CAUSAL_MERGE_ROUTES)
def test_causal_tail_kernels_merge_partials_on_adversarial_lses(route, pattern, dt):
    """Hand-made partials through hyd_suffix_attn_causal_fwd, bounds as test_suffix_kernels_merge_partials_on_adversarial_lses.  A
    token without a unique key (length 0, or 0 < len < T) that has a finite partial returns the merge of the partials alone."""
    c = S.causal_merge_case(route, pattern, dt)
    got = _run_merge(c, route, dt, f"causal {route} {pattern} {dt}", causal=True)
    if pattern == "all_empty":
        assert not got.any()


# ---- d. combine_lse (combine.hip) and _combine_many ------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", S.LSE_PATTERNS)
@pytest.mark.parametrize("n", [2, 5, 64, 65, 70])
def test_combine_many_on_adversarial_lses(pattern, n):
    """fp32 partials, the tolerance of tests/test_edge_gpu.py::test_merge_of_more_partials_than_one_launch_takes (rtol 2e-5,
    atol 2e-6); 64, 65 and 70 partials cross the 64-per-launch grouping; D = 63 and 129 as in the parity test's grid."""
    from hydragen_amd.attention import _combine_many

    worst = 0.0
    for D in (63, 64, 129):
        c = S.combine_case(pattern, n, D)
        got = _combine_many([dev(o) for o in c["outs"]], [dev(l) for l in c["lses"]]).cpu().numpy()
        torch.cuda.synchronize()
        assert np.isfinite(got).all()
        ok = c["ok"]
        worst = max(worst, float((np.abs(got[ok] - c["want"][ok]) / (2e-6 + 2e-5 * np.abs(c["want"][ok]))).max()) if ok.any() else 0.0)
        np.testing.assert_allclose(got[ok], c["want"][ok], rtol=2e-5, atol=2e-6)
        assert not got[~ok].any()
    print(f"stress-ratio out combine_many {pattern} n={n}: {worst:.3f}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("pattern", S.LSE_PATTERNS)
def test_combine_lse_16bit_on_adversarial_lses(pattern, dt):
    """combine.hip on 16-bit partials (one launch: 2, 5 and 64 of them), bounds of gpu_util.assert_close_l2"""
    from hydragen_amd.attention import combine_lse

    for n in (2, 5, 64):
        for D in (63, 129):
            c = S.combine_case(pattern, n, D)
            outs = [O.round_fp16(o) if dt == "f16" else O.round_bf16(o) for o in c["outs"]]
            want = np.where(c["ok"][..., None], O.combine_lse(outs, c["lses"]), 0.0)
            got = combine_lse([dev(o.astype(np.float32), dt) for o in outs], [dev(l) for l in c["lses"]]).float().cpu().numpy()
            ok = c["ok"]
            assert np.isfinite(got).all() and not got[~ok].any()
            if ok.any():
                _check_out(got[ok], want[ok], dt, f"combine_lse {pattern} n={n} D={D} {dt}")


# ---- e. the whole operator, real LSEs -------------------------------------------------------------------------------------------
def _plan(B, Hq, Hkv, D, P, dt):
    from hydragen_amd import _lib

    pp = _lib.PrefixParams()
    pp.dtype = _lib.HYD_BF16 if dt == "bf16" else _lib.HYD_F16
    pp.B, pp.nq, pp.Hq, pp.Hkv, pp.D, pp.sb, pp.kv_len = B, 1, Hq, Hkv, D, 1, P
    pp.k_tok_stride = pp.v_tok_stride = Hkv * D
    pp.k_head_stride = pp.v_head_stride = D
    ns, sl = C.c_int32(), C.c_int32()
    _lib.check(_lib.load().hyd_prefix_plan(C.byref(pp), C.byref(ns), None, C.byref(sl)))
    return ns.value, sl.value


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("mass", S.OPERATOR_MASS)
@pytest.mark.parametrize("shape", list(S.OPERATOR_SHAPES))
def test_operator_with_all_the_mass_on_one_side(shape, mass, dt):
    """hydragen_attention_nopad with one and with two shared levels; the prefix holds all the mass, the suffix does, or the two
    LSEs agree to 1e-3.  A prefix of 300 keys (one slice) and one of 4097 that the planner splits: there every key that matters
    lies in ONE slice -- the first, a middle one, the last -- and the other slices' LSEs end 60 or more below it."""
    from hydragen_amd.attention import hydragen_attention_nopad

    B, Hq, Hkv, cap = S.OPERATOR_SHAPES[shape]
    ns, split_len = _plan(B, Hq, Hkv, 128, 4097, dt)
    assert ns > 1, "the planner does not split the 4097-key level"
    spots = [(300, 150, 1), (300, 150, 2), (4097, 3, 1), (4097, split_len * (ns // 2) + 3, 1), (4097, 4097 - 7, 1), (4097, 4097 - 7, 2)]
    for P, hot_at, levels in spots:
        c = S.operator_case(shape, mass, P, hot_at, dt, levels)
        got = hydragen_attention_nopad(dev(c["q"], dt), dev(c["k"], dt), dev(c["v"], dt), [dev(x, dt) for x in c["shared_ks"]],
                                       [dev(x, dt) for x in c["shared_vs"]], dev(c["lens"]))
        torch.cuda.synchronize()
        want = O.hydragen_attention_nopad(c["q"], c["k"], c["v"], c["shared_ks"], c["shared_vs"], c["lens"])
        _check_out(got.float().cpu().numpy(), want, dt, f"operator {shape} {mass} P={P} hot at {hot_at}, {levels} level(s) {dt}")
