"""-m gpu: every body of the prefix pass (tests/prefix_stress_cases.py PREFIX_ROUTES: the 8-wave unit with two key halves and in
its 256-row form, the 4-wave unit at D = 64 in both heights, the D = 256 unit, the persistent unit walk of the decode entry; causal,
forced and planner-chosen splits through combine.hip, cu_seqlens_k groups with empty splits, packed queries) on adversarial score
patterns, `out` AND `lse` against the float64 oracle on the identical rounded inputs.  The bounds are the suite's existing ones
(gpu_util.assert_close_l2; |lse - want| <= 2e-3 + 1e-5 |want|); rows without a visible key must be exactly 0 / -inf; finite giants,
NaN and Inf behind a length may not move one bit; repeated launches must agree bit for bit.  tests/test_prefix_stress.py shows that the
reference's own rounding model meets half of these bounds on every case.  Every test prints its largest error / bound ratios
(`-s` shows them).

Largest error / bound ratios measured on an MI355X, per route over all patterns and both dtypes (measured values, not limits; the
case that gave them in brackets; the decode entry returns no lse; the bf16 rounding of the result alone is 0.40 to 0.45 of the `out` bound):

    w8_kg2                    w8/kg2          out 0.456 (step_just_over_tau bf16 without the anchor rows), lse 0.010 (ramp_per_key bf16)
    w8_kg1                    w8/kg1          out 0.539 (ramp_per_key bf16), lse 0.010 (repeated_late_spikes bf16)
    w4_kg2                    w4/kg2          out 0.543 (repeated_late_spikes bf16), lse 0.006 (repeated_late_spikes bf16)
    w4_kg1                    w4/kg1          out 0.613 (repeated_late_spikes bf16), lse 0.005 (repeated_late_spikes bf16)
    w4_d256                   w4/d256         out 0.544 (ramp_per_key bf16 without the anchor rows), lse 0.016 (repeated_late_spikes bf16)
    w8_kg2_split3             w8/kg2          out 0.459 (key_half_negligible bf16 without the anchor rows), lse 0.009 (repeated_late_spikes bf16)
    w8_kg2_splitP             w8/kg2          out 0.465 (plateau_just_under_the_bound bf16 without the anchor rows), lse 0.011 (repeated_late_spikes bf16)
    w4_kg2_split3             w4/kg2          out 0.630 (ramp_per_block bf16 without the anchor rows), lse 0.007 (repeated_late_spikes bf16)
    w4_kg2_splitP             w4/kg2          out 0.493 (ramp_per_block bf16 without the anchor rows), lse 0.007 (ramp_per_key bf16)
    w4_d256_split3            w4/d256         out 0.632 (ramp_per_key bf16 without the anchor rows), lse 0.014 (repeated_late_spikes bf16)
    w4_d256_splitP            w4/d256         out 0.522 (ramp_per_key bf16 without the anchor rows), lse 0.020 (ramp_per_block f16)
    ragged_k_d128             w8/kg2          out 0.346 (giants_behind_length bf16 without the anchor rows), lse 0.012 (repeated_late_spikes f16)
    ragged_k_d256             w4/d256         out 0.471 (giants_behind_length bf16 without the anchor rows), lse 0.018 (repeated_late_spikes f16)
    ragged_qk                 w8/kg2          out 0.478 (ramp_per_key bf16 without the anchor rows), lse 0.010 (repeated_late_spikes bf16)
    w4_persist                w4/persist      out 0.717 (ramp_per_block bf16 without the anchor rows), lse 0.000 (-)
    w4_persist_d64            w4/kg2+persist  out 0.637 (ramp_per_block bf16 without the anchor rows), lse 0.000 (-)
    w8_kg2_split3_deep        w8/kg2          out 0.466 (ties bf16), lse 0.012 (repeated_late_spikes bf16)
    w4_kg2_split3_deep        w4/kg2          out 0.626 (ramp_per_block bf16 without the anchor rows), lse 0.007 (repeated_late_spikes bf16)
    w8_kg2_causal             w8/kg2          out 0.525 (other_key_half_negligible bf16 without the anchor rows), lse 0.010 (ramp_per_key bf16)
    w8_kg1_causal             w8/kg1          out 0.513 (ramp_per_key bf16 without the anchor rows), lse 0.009 (repeated_late_spikes f16)
    w4_kg2_causal             w4/kg2          out 0.542 (ramp_per_block bf16 without the anchor rows), lse 0.005 (repeated_late_spikes bf16)
    w4_kg1_causal             w4/kg1          out 0.577 (repeated_late_spikes bf16), lse 0.004 (ramp_per_block bf16)
    w4_d256_causal            w4/d256         out 0.551 (step_just_under_tau bf16 without the anchor rows), lse 0.016 (repeated_late_spikes f16)
    w8_kg2_split3_causal      w8/kg2          out 0.577 (ramp_per_key bf16 without the anchor rows), lse 0.008 (ramp_per_key bf16)
    w8_kg2_splitP_causal      w8/kg2          out 0.606 (ramp_per_block bf16 without the anchor rows), lse 0.011 (repeated_late_spikes bf16)
    w4_kg2_split3_causal      w4/kg2          out 0.554 (ramp_per_block bf16 without the anchor rows), lse 0.006 (repeated_late_spikes bf16)
    w4_kg2_splitP_causal      w4/kg2          out 0.539 (ramp_per_block bf16 without the anchor rows), lse 0.007 (ramp_per_key bf16)
    w4_d256_split3_causal     w4/d256         out 0.575 (ramp_per_block bf16 without the anchor rows), lse 0.014 (repeated_late_spikes bf16)
    w4_d256_splitP_causal     w4/d256         out 0.569 (ramp_per_block bf16 without the anchor rows), lse 0.020 (ramp_per_block f16)
    ragged_qk_causal          w8/kg2          out 0.474 (ramp_per_key bf16 without the anchor rows), lse 0.007 (repeated_late_spikes f16)
    w8_kg2_split3_deep_causal w8/kg2          out 0.508 (ramp_per_key bf16 without the anchor rows), lse 0.007 (ramp_per_key bf16)
    w4_kg2_split3_deep_causal w4/kg2          out 0.604 (ramp_per_block bf16 without the anchor rows), lse 0.006 (ramp_per_key bf16)
    lengths D=64                              out 0.403 (ties bf16 fixed causal=True), lse 0.002 (last_key_spike bf16 ragged, 1 split(s))
    lengths D=128                             out 0.401 (ties bf16 fixed causal=True), lse 0.005 (last_key_spike f16 ragged, 1 split(s))
    lengths D=256                             out 0.401 (ties bf16 fixed causal=True), lse 0.005 (last_key_spike bf16 ragged, 1 split(s))
    sq > sk sk=37                             out 0.425 (sq=300 > sk=37 D=64 bf16), lse 0.000 (-)
    causal ties                               out 0.412 (ties sq=40 sk=70 D=64 bf16), lse 0.000 (-)
    staircase D=64                            out 0.000 (-), lse 0.004 (bf16)
    staircase D=128                           out 0.000 (-), lse 0.009 (bf16)
    staircase D=256                           out 0.000 (-), lse 0.011 (f16)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import prefix_stress_cases as P
from tests.gpu_util import dev
from tests.test_softmax_stress_gpu import _bits, _check_lse, _check_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = list(P.PREFIX_ROUTES)
DTYPES = ["bf16", "f16"]


# ---- a case in group form -> one launch of the route's entry point ----------------------------------------------------------------
def _tile(x, sb, dt=None):
    """a built block on the device, repeated to the route's group count"""
    t = dev(x, dt)
    return t if t.shape[0] == sb else t[torch.arange(sb, device=DEV) % t.shape[0]].contiguous()


def _full(x, sb):
    return x if x.shape[0] == sb else x[np.arange(sb) % x.shape[0]]


def _decode_launch(q, sk, sv, wgs):
    """the decode entry with an empty unique cache and one shared level, held to `wgs` persistent workgroups (0: one per unit)"""
    from hydragen_amd import _lib
    from hydragen_amd import attention as A

    B, Hkv, D = q.shape[0], sk.shape[2], q.shape[3]
    ku = torch.empty((B, 0, Hkv, D), dtype=q.dtype, device=q.device)
    seen = []

    def spy(lib, p, two_stream, stream, kq=None):
        p.phase, p.shared_max_workgroups, p.single_launch_small = _lib.HYD_PHASE_ALL, wgs, 0
        _lib.check(lib.hyd_decode_attn_fused(C.byref(p), stream))
        seen.append(wgs)

    orig = A._launch_decode
    try:
        A._PARAM_CACHE.clear()
        A._launch_decode = spy
        out = A.hydragen_attention(q, ku, ku, [sk], [sv], [None], [None], [False])
    finally:
        A._launch_decode = orig
        A._PARAM_CACHE.clear()
    assert seen == [wgs]
    return out


def _launcher(route_row, c, dt, wgs=None, splits=None):
    """() -> (out [sb, T, Hq, D], lse [sb, Hq, T] or None) on the device, every call one launch of the same tensors"""
    from hydragen_amd._lib import HYD_LSE_BQH
    from hydragen_amd.flash import flash_attention, flash_attention_varlen, prefix_attention

    r = route_row
    entry, sb, T, Hq, D = r["entry"], r["sb"], c["q"].shape[1], c["Hq"], c["D"]
    splits = r["splits"] if splits is None else splits
    q = _tile(c["q"], sb, dt)
    if entry in ("flash", "split", "decode"):
        L = int(c["klens"][0])
        assert (c["klens"] == L).all()
        k, v = _tile(c["k"], sb, dt)[:, :L], _tile(c["v"], sb, dt)[:, :L]  # views: whatever the buffers hold behind L stays where it is
        if entry == "flash":
            return lambda: flash_attention(q, k, v, causal=c["causal"])
        if entry == "split":
            def run():
                out, lse = prefix_attention(q, k, v, sb=sb, kv_len=L, group_stride=(k.stride(0), v.stride(0)), tok_stride=(k.stride(1), v.stride(1)),
                                            head_stride=(k.stride(2), v.stride(2)), B=sb, nq=T, causal=c["causal"], lse_layout=HYD_LSE_BQH,
                                            lse_shape=(sb, T, Hq), num_splits=splits)
                return out, lse.permute(0, 2, 1)
            return run
        qd = q.reshape(sb * T, 1, Hq, D)
        return lambda: (_decode_launch(qd, k, v, r["wgs"] if wgs is None else wgs).view(sb, T, Hq, D), None)
    assert sb == len(c["klens"])
    kp, vp, cu = P.pack_keys(c)
    kp, vp, cu = dev(kp, dt), dev(vp, dt), dev(cu)
    if entry == "ragged_k":
        qd = q.reshape(sb * T, 1, Hq, D)

        def run():
            out, lse = prefix_attention(qd, kp, vp, sb=sb, kv_len=int(c["klens"].max()), group_stride=(0, 0), tok_stride=(kp.stride(0), vp.stride(0)),
                                        head_stride=(kp.stride(1), vp.stride(1)), B=sb * T, nq=1, causal=False, lse_layout=HYD_LSE_BQH,
                                        lse_shape=(sb * T, 1, Hq), cu_seqlens_k=cu, num_splits=splits)
            return out.view(sb, T, Hq, D), lse.view(sb, T, Hq).permute(0, 2, 1)
        return run
    assert entry == "varlen"
    ql = [int(n) for n in c["qlens"]]
    cu_q = dev(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32))
    qp = torch.cat([q[i, :n] for i, n in enumerate(ql)], 0).contiguous()

    def run():
        outp, lse = flash_attention_varlen(qp, kp, vp, cu_q, cu, max(ql), int(c["klens"].max()), causal=c["causal"])
        out = torch.zeros_like(q)
        at = 0
        for i, n in enumerate(ql):
            out[i, :n] = outp[at:at + n]
            at += n
        return out, lse
    return run


def _check(c, sb, out, lse, dt, what, want=None):
    """out / lse of one launch against the oracle (or a closed form given as `want` = (out, lse or None)); returns the two ratios"""
    ref_out, ref_lse, valid, has = P.reference(c)
    if want is not None:
        ref_out, ref_lse = want[0], (ref_lse if want[1] is None else want[1])
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    assert got.shape[0] == sb
    ref_out, wl, valid, has = _full(ref_out, sb), _full(ref_lse.transpose(0, 2, 1), sb), _full(valid, sb), _full(has, sb)
    none = valid & ~has  # a query token without a visible key: exactly 0, lse = -inf
    assert np.isfinite(got[valid]).all() and not got[none].any(), f"{what}: rows without a visible key must be exactly 0"
    _check_out(got[has], ref_out[has], dt, what)
    if want is None and c["anchor"].any():
        # the anchor rows set the tensor's largest element and with it the max-abs bound (prefix_stress_cases.ANCHOR_LOG2): where the
        # reference's rounding model says the other rows meet half the bounds on their own, hold them to the bounds on their own as well
        plain, ok = P.plain_rows_checkable(c)
        if ok:
            plain = _full(plain, sb)
            _check_out(got[plain], ref_out[plain], dt, what + " without the anchor rows")
    if lse is not None:
        gl = lse.float().cpu().numpy().transpose(0, 2, 1)
        _check_lse(gl[has], wl[has], what)
        assert np.isneginf(gl[none]).all(), f"{what}: lse of a row without a visible key must be -inf"


PAIRS = [(r, p) for r in ROUTES for p in P.SCORE_PATTERNS + (P.SPLIT_PATTERNS if r in P.SPLIT_ROUTES else ())]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("route,pattern", PAIRS)
def test_prefix_routes_on_adversarial_scores(route, pattern, dt):
    """route x score pattern x dtype, out and lse (the decode entry returns no lse).  split_negligible_*: the planner's and the
    forced slices + combine.hip with the mass in one split; the ragged rows' short groups leave a split empty.  At D = 64 the
    persistent launch and the one-unit launch run the same 4-wave arithmetic on the same units: equal bits."""
    r = P.PREFIX_ROUTES[route]
    c = P.route_case(route, pattern, dt)
    out, lse = _launcher(r, c, dt)()
    what = f"{route} {pattern} {dt}"
    _check(c, r["sb"], out, lse, dt, what)
    if pattern == "ties":  # the mean of the visible v rows, lse = ln(count): a limit off by one key moves lse by 1 / n
        _check(c, r["sb"], out, lse, dt, what + " closed form", want=P.ties_closed_form(c))
    if pattern == "last_key_spike" and not r["causal"]:  # v[L - 1]: a lost or zero-filled last key returns another row
        _check(c, r["sb"], out, lse, dt, what + " closed form", want=(P.last_visible_closed_form(c), None))
    if r["entry"] == "decode" and r["D"] == 64:
        one, _ = _launcher(r, c, dt, wgs=0)()
        assert torch.equal(_bits(one), _bits(out)), f"{what}: the persistent walk differs from the one-unit launch"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_last_key_spike_and_ties_over_the_length_list(D, dt):
    """Lengths around the 32-key block, the 64-key half, the 128-key tile and the split boundary: as ONE cu_seqlens_k launch (unsplit, and
    with 3 forced splits that the short groups leave empty) and group by group as fixed-length launches; ties also causal, where 40
    query tokens on 1 or 31 keys leave rows without any key."""
    from hydragen_amd.flash import flash_attention

    split_len = P.lengths_split_len(D)
    for pattern in ("last_key_spike", "ties"):
        c = P.lengths_case(pattern, D, dt, split_len)
        nb = len(c["klens"])
        closed = P.ties_closed_form(c) if pattern == "ties" else (P.last_visible_closed_form(c), None)
        row = dict(entry="ragged_k", sb=nb, splits=1)
        for splits in (1, P.LENGTHS_SPLITS):
            out, lse = _launcher(row, c, dt, splits=splits)()
            what = f"lengths {pattern} D={D} {dt} ragged, {splits} split(s)"
            _check(c, nb, out, lse, dt, what)
            _check(c, nb, out, lse, dt, what + " closed form", want=closed)
        for causal in ((False, True) if pattern == "ties" else (False,)):
            cc = dict(c, causal=causal)
            outs, lses = [], []
            for i, n in enumerate(int(x) for x in c["klens"]):
                o, l = flash_attention(dev(c["q"][i:i + 1], dt), dev(c["k"][i:i + 1, :n], dt), dev(c["v"][i:i + 1, :n], dt), causal=causal)
                outs.append(o)
                lses.append(l)
            out, lse = torch.cat(outs), torch.cat(lses)
            what = f"lengths {pattern} D={D} {dt} fixed causal={causal}"
            _check(cc, nb, out, lse, dt, what)
            _check(cc, nb, out, lse, dt, what + " closed form", want=P.ties_closed_form(cc) if pattern == "ties" else closed)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("route", ROUTES)
def test_giants_behind_the_length_do_not_move_a_bit(route, dt):
    """Fixed groups: K / V are [:, :L] views of longer buffers that hold finite giants (90 log2-units) in K and NaN / Inf in V behind L.
    Ragged groups: the next group's first keys (and pad rows behind the last group) are the giants.  Against the twin with zeros
    there, not one bit of out or lse may differ; and both meet the oracle."""
    r = P.PREFIX_ROUTES[route]
    c = P.giants_case(route, dt)
    out, lse = _launcher(r, c, dt)()
    out0, lse0 = _launcher(r, P.zero_behind(c), dt)()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(out0)), f"{route} {dt}: what lies behind the length reached out"
    if lse is not None:
        assert torch.equal(_bits(lse.contiguous()), _bits(lse0.contiguous())), f"{route} {dt}: what lies behind the length reached lse"
    _check(c, r["sb"], out, lse, dt, f"{route} giants_behind_length {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_causal_rows_without_a_visible_key(D, dt):
    """causal with sq > sk: the leading sq - sk rows see nothing and must be exactly 0 with lse = -inf, the rest the oracle's.  100 on 37:
    rows with and without keys share a workgroup (and a wave); 300 on 37: whole workgroups without a key."""
    for sq, sk in ((100, 37), (300, 37)):
        c = P.more_queries_than_keys_case(D, dt, sq, sk)
        row = dict(entry="flash", sb=2, splits=1)
        out, lse = _launcher(row, c, dt)()
        assert (~P.reference(c)[3]).sum() == 2 * (sq - sk)
        _check(c, 2, out, lse, dt, f"sq={sq} > sk={sk} D={D} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_causal_ties_count_every_rows_own_keys(D, dt):
    """q = 0 under the causal mask with sq < sk (40 on 70), sq = sk (70 on 70: token i sees exactly i + 1 keys) and sq > sk (100 on 37): out = the
    mean of the row's visible v rows, lse = ln(count).  Every count is below 500, so a limit off by one key moves lse above its bound."""
    for sq, sk in ((40, 70), (70, 70), (100, 37)):
        c = P.more_queries_than_keys_case(D, dt, sq, sk)
        c["q"] = np.zeros_like(c["q"])
        out, lse = _launcher(dict(entry="flash", sb=2, splits=1), c, dt)()
        what = f"causal ties sq={sq} sk={sk} D={D} {dt}"
        _check(c, 2, out, lse, dt, what)
        _check(c, 2, out, lse, dt, what + " closed form", want=P.ties_closed_form(c))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_causal_last_rows_staircase(D, dt):
    """7 rows over 200 keys, the last 7 keys a ramp: causal row i returns v[L - 7 + i]; a limit off by one returns a neighbour"""
    c = P.staircase_case(D, dt)
    out, lse = _launcher(dict(entry="flash", sb=2, splits=1), c, dt)()
    _check(c, 2, out, lse, dt, f"staircase D={D} {dt}")
    _check(c, 2, out, lse, dt, f"staircase D={D} {dt} closed form", want=(P.last_visible_closed_form(c), None))


@pytest.mark.parametrize("route", P.REPEAT_ROUTES)
def test_repeated_prefix_launches_are_bit_identical(route):
    """20 back-to-back launches per route: no atomics on the path, so a difference is a race (a ring slot reused too early, a DMA not
    waited for, the persistent walk's barrier between units).  D = 64, D = 256, the 256-row workgroups, the split slices and the
    persistent rows; tests/test_edge_gpu.py::test_repeated_launches_are_bit_identical covers D = 128 one-unit launches."""
    r = P.PREFIX_ROUTES[route]
    run = _launcher(r, P.route_case(route, "late_spike_after_plateau", "bf16"), "bf16")
    res = [run() for _ in range(20)]
    torch.cuda.synchronize()
    for out, lse in res[1:]:
        assert torch.equal(_bits(out), _bits(res[0][0])), route
        assert lse is None or torch.equal(_bits(lse.contiguous()), _bits(res[0][1].contiguous())), route
