"""-m gpu: every attention kernel on head geometries that are not powers of two (tests/head_geometry_cases.py), `out` and LSE
against the float64 oracle on the rounded inputs with the project's usual bounds.  Which kernel a shape reaches is read from the
dispatch rules in the source; each section names the rule it relies on.  A new launch rule keyed on Hkv or g = Hq / Hkv gets
its case here (DESIGN.md "Head geometries")."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hydragen_oracle as O
from tests import head_geometry_cases as HG
from tests.gpu_util import ATOL, assert_close, assert_close_l2, atol, case_to_device, dev

pytestmark = pytest.mark.gpu
DTYPES = ["f16", "bf16"]


def _np(t):
    return t.float().cpu().numpy()


def _check_out(got, want, dt, what, l2=False, keep=None):
    """gpu_util.assert_close (or assert_close_l2 where the tensor is small: see its docstring) with the rows at fault named.
    keep: boolean [B], the sequences that are compared (all of them when None)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    g, w = (got, want) if keep is None else (got[keep], want[keep])
    try:
        (assert_close_l2 if l2 else assert_close)(g, w, dt, what)
    except AssertionError as e:
        # the absolute bound the failed assertion used (gpu_util: assert_close_l2 scales the fp16 one by max |want| above 1)
        bound = ATOL["f16"] * max(1.0, float(np.abs(w).max())) if l2 and dt == "f16" else atol(dt, w)
        g4, w4 = (got.copy(), want) if got.ndim == 4 else (got[None].copy(), want[None])
        if keep is not None:
            g4[~keep] = w4[~keep]
        raise AssertionError(f"{e}\n{HG.blame_rows(g4, w4, bound)}") from None


def _check_lse(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.all(np.isneginf(got[~fin])), f"{what}: the LSE of a row without keys must be -inf"
    w = np.where(fin, want, 0.0)
    with np.errstate(invalid="ignore"):
        bad = fin & ~(np.abs(got - w) <= 2e-3 + 1e-5 * np.abs(w))  # (a NaN is off as well)
    assert not bad.any(), f"{what}: {int(bad.sum())} LSE entries off, the first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"{got[bad][:4]} for {want[bad][:4]}"


def _plan(dt, B, nq, hq, hkv, D, sb, kv_len, num_splits=0, causal=False):
    """(num_splits, grid) hyd_prefix_plan gives a contiguous [sb, kv_len, Hkv, D] level."""
    from hydragen_amd import _lib

    pp = _lib.PrefixParams()
    pp.dtype = _lib.HYD_F16 if dt == "f16" else _lib.HYD_BF16
    pp.B, pp.nq, pp.Hq, pp.Hkv, pp.D, pp.sb, pp.kv_len = B, nq, hq, hkv, D, sb, kv_len
    pp.k_tok_stride = pp.v_tok_stride = hkv * D
    pp.num_splits, pp.causal = num_splits, 1 if causal else 0
    ns, grid = C.c_int32(), C.c_int32()
    _lib.check(_lib.load().hyd_prefix_plan(C.byref(pp), C.byref(ns), C.byref(grid), None))
    return ns.value, grid.value


# ---- A. prefix pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("causal", [False, True], ids=["dense", "causal"])
@pytest.mark.parametrize("geom,D", HG.A1_CASES, ids=[f"{g}-D{D}" for g, D in HG.A1_CASES])
def test_a1_flash_attention(geom, D, causal, dt):
    """prefix_unit_w64.h: unit -> (group, kv head, split, row block) divides by Hkv, row -> (token, head) by g; with sq < sk the
    causal mask is bottom-right aligned and its bounds come from the same decode."""
    from hydragen_amd.flash import flash_attention

    hq, hkv = HG.heads(geom)
    b, sq, sk = HG.A1_B, HG.a1_sq(geom), HG.A1_SK
    rng = HG.seeded("a1", geom, D, dt)  # (the same inputs for the dense and the causal run)
    q, k, v = HG.rand(rng, (b, sq, hq, D), dt), HG.rand(rng, (b, sk, hkv, D), dt), HG.rand(rng, (b, sk, hkv, D), dt)
    out, lse = flash_attention(dev(q, dt), dev(k, dt), dev(v, dt), causal=causal)
    torch.cuda.synchronize()
    want, wlse = O.flash_attention(q, k, v, causal=causal)
    assert lse.shape == (b, hq, sq) and lse.dtype == torch.float32
    _check_out(_np(out), want, dt, f"flash_attention {geom} D{D}")
    _check_lse(lse.cpu().numpy(), wlse, f"flash_attention {geom} D{D}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("ns", HG.A2_SPLITS)
def test_a2_split_counts(ns, D, dt):
    """div_nsplit with 3, 5, 6 and 7 splits: the slices and the in-library merge give the unsplit answer."""
    from hydragen_amd._lib import HYD_LSE_BHQ
    from hydragen_amd.flash import prefix_attention

    hq, hkv = HG.heads(HG.A2_GEOM)
    b, sq, sk = HG.A2_B, HG.A2_SQ, HG.a2_sk(ns)
    assert _plan(dt, b, sq, hq, hkv, D, b, sk, num_splits=ns)[0] == ns
    rng = HG.seeded("a2", ns, D, dt)
    q, k, v = HG.rand(rng, (b, sq, hq, D), dt), HG.rand(rng, (b, sk, hkv, D), dt), HG.rand(rng, (b, sk, hkv, D), dt)
    tq, tk, tv = dev(q, dt), dev(k, dt), dev(v, dt)
    out, lse = prefix_attention(
        tq, tk, tv, sb=b, kv_len=sk, group_stride=(tk.stride(0), tv.stride(0)), tok_stride=(tk.stride(1), tv.stride(1)),
        head_stride=(tk.stride(2), tv.stride(2)), B=b, nq=sq, causal=False, lse_layout=HYD_LSE_BHQ, lse_shape=(b, hq, sq),
        num_splits=ns)
    torch.cuda.synchronize()
    want, wlse = O.flash_attention(q, k, v)
    _check_out(_np(out), want, dt, f"{ns} splits D{D}")
    _check_lse(lse.cpu().numpy(), wlse, f"{ns} splits D{D}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("causal", [False, True], ids=["dense", "causal"])
@pytest.mark.parametrize("geom", HG.A3_GEOMS)
def test_a3_flash_attention_varlen(geom, causal, dt):
    from hydragen_amd.flash import flash_attention_varlen

    hq, hkv = HG.heads(geom)
    D, qlens, klens = 128, HG.A3_QLENS, HG.A3_KLENS[causal]
    cu_q = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    cu_k = np.concatenate([[0], np.cumsum(klens)]).astype(np.int32)
    rng = HG.seeded("a3", geom, causal, dt)
    q, k, v = HG.rand(rng, (cu_q[-1], hq, D), dt), HG.rand(rng, (cu_k[-1], hkv, D), dt), HG.rand(rng, (cu_k[-1], hkv, D), dt)
    out, lse = flash_attention_varlen(dev(q, dt), dev(k, dt), dev(v, dt), dev(cu_q), dev(cu_k), max(qlens), max(klens),
                                      causal=causal)
    torch.cuda.synchronize()
    want, wlse = O.flash_attention_varlen(q, k, v, cu_q, cu_k, max(qlens), max(klens), causal=causal)
    _check_out(_np(out), want, dt, f"varlen {geom}")
    got_lse = lse.cpu().numpy()
    assert got_lse.shape == wlse.shape
    for i, n in enumerate(qlens):  # valid entries only: [nseq, Hq, max_seqlen_q] is padded past each sequence's queries
        _check_lse(got_lse[i, :, :n], wlse[i, :, :n], f"varlen {geom} sequence {i}")


@pytest.mark.parametrize("dt", DTYPES)
def test_a4_256_row_workgroups_with_odd_divisors(dt):
    """plan_prefix: more 128-row units than the chip has CUs (87 x 3) -> 256-row workgroups, 44 x 3 units, 3 rows in the last
    block; 7 heads per token straddle every block and wave boundary."""
    from hydragen_amd.flash import flash_attention

    hq, hkv = HG.heads(HG.A4_GEOM)
    D, sq, sk = 128, HG.A4_SQ, HG.A4_SK
    assert _plan(dt, 1, sq, hq, hkv, D, 1, sk) == (1, HG.A4_GRID)
    rng = HG.seeded("a4", dt)
    q, k, v = HG.rand(rng, (1, sq, hq, D), dt), HG.rand(rng, (1, sk, hkv, D), dt), HG.rand(rng, (1, sk, hkv, D), dt)
    out, lse = flash_attention(dev(q, dt), dev(k, dt), dev(v, dt))
    torch.cuda.synchronize()
    want, wlse = O.flash_attention(q, k, v)
    _check_out(_np(out), want, dt, "256-row workgroups")
    _check_lse(lse.cpu().numpy(), wlse, "256-row workgroups")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom", HG.A5_GEOMS)
def test_a5_causal_with_several_sequences_per_group(geom, dt):
    """hyd_prefix_attn_fwd takes causal with per = B / sb > 1 (tests/abi_table.py plans it): every sequence's nq queries are
    masked bottom-right against its GROUP's keys (row_lim = tok % nq + L - nq)."""
    from hydragen_amd._lib import HYD_LSE_BQH
    from hydragen_amd.flash import prefix_attention

    hq, hkv = HG.heads(geom)
    D, sb, B, nq, L = 128, HG.A5_SB, HG.A5_B, HG.A5_NQ, HG.A5_KV
    rng = HG.seeded("a5", geom, dt)
    q, k, v = HG.rand(rng, (B, nq, hq, D), dt), HG.rand(rng, (sb, L, hkv, D), dt), HG.rand(rng, (sb, L, hkv, D), dt)
    tq, tk, tv = dev(q, dt), dev(k, dt), dev(v, dt)
    out, lse = prefix_attention(
        tq, tk, tv, sb=sb, kv_len=L, group_stride=(tk.stride(0), tv.stride(0)), tok_stride=(tk.stride(1), tv.stride(1)),
        head_stride=(tk.stride(2), tv.stride(2)), B=B, nq=nq, causal=True, lse_layout=HYD_LSE_BQH, lse_shape=(B, nq, hq))
    torch.cuda.synchronize()
    want, wlse = np.zeros(q.shape), np.zeros((B, nq, hq))
    for i in range(B):  # each sequence on its own against its group's keys
        gi = i // (B // sb)
        o, l = O.flash_attention(q[i:i + 1], k[gi:gi + 1], v[gi:gi + 1], causal=True)
        want[i], wlse[i] = o[0], l[0].T
    _check_out(_np(out), want, dt, f"causal, 3 sequences per group, {geom}")
    _check_lse(lse.cpu().numpy(), wlse, f"causal, 3 sequences per group, {geom}")


# ---- B. suffix pass -------------------------------------------------------------------------------------------------------------
def _suffix_case(geom, D, B, S, nq, dt, lens=None, l2=False):
    """flash_attention_seqlen with int32 lengths; K past every length is NaN, V +-Inf / NaN."""
    from hydragen_amd.flash import flash_attention_seqlen

    hq, hkv = HG.heads(geom)
    rng = HG.seeded("suffix", HG.geom_id(geom), D, B, S, nq, dt)
    q, k, v = HG.rand(rng, (B, nq, hq, D), dt), HG.rand(rng, (B, S, hkv, D), dt), HG.rand(rng, (B, S, hkv, D), dt)
    sl = HG.suffix_lens(rng, B, S) if lens is None else lens
    kp, vp = HG.poison(k, v, sl)
    out, lse = flash_attention_seqlen(dev(q, dt), dev(kp, dt), dev(vp, dt), seq_len=dev(sl))
    torch.cuda.synchronize()
    want, wlse = O.flash_attention_seqlen(q, k, v, sl)
    what = f"seqlen {HG.geom_id(geom)} D{D} B{B} S{S} nq{nq}"
    got = _np(out)
    assert lse.shape == (B, nq, hq) and lse.dtype == torch.float32
    assert np.isfinite(got).all(), f"{what}: padding leaked into the output"
    _check_out(got, want, dt, what, l2=l2, keep=sl > 0)  # (rows of an empty sequence are undefined: only their LSE, -inf, is checked)
    _check_lse(lse.cpu().numpy(), wlse, what)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,D", HG.B1_CASES, ids=[f"{g}-D{D}" for g, D in HG.B1_CASES])
def test_b1_matrix_core_kernel_one_wave_per_unit(geom, D, dt):
    """gqa_launch_plan: 4 (g7x4), 2 (g3x6, g7x2; g3x8 at D = 256, capped) or 1 kv head per workgroup (odd Hkv, Hkv > 8); g71 is five
    16-row chunks, the last of 7 rows."""
    _suffix_case(geom, D, HG.B1_B, HG.B1_S, 1, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,D", HG.B2_CASES, ids=[f"{g}-D{D}" for g, D in HG.B2_CASES])
def test_b2_few_units(geom, D, dt):
    """gqa_few_units: four waves per unit at D 64 / 128; at D = 256 suffix_gqa_eligible refuses the shape and launch_suffix_t runs
    the dot-product kernel with 4 or 8 rows per chunk."""
    _suffix_case(geom, D, HG.B2_B, HG.B2_S, 1, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,nq", HG.B3_CASES, ids=[f"{g}-nq{n}" for g, n in HG.B3_CASES])
def test_b3_several_queries_with_odd_g(geom, nq, dt):
    """iq = row / g, gq = row % g: 21 rows (16 + 5, a token's heads on both sides of the chunk boundary), 10 rows, and 3 rows at g = 1."""
    _suffix_case(geom, 128, HG.B3_B, HG.B3_S, nq, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,D", HG.B4_CASES, ids=[f"{HG.geom_id(g)}-D{D}" for g, D in HG.B4_CASES])
def test_b4_token_row_kernel_ragged_waves_per_sequence(geom, D, dt):
    """launch_suffix_rows: wps = Hkv / HPI = 3, 5 or 6 waves per sequence in workgroups of 4: the waves of the last workgroup row
    whose first head is past Hkv leave before the barriers."""
    _suffix_case(geom, D, HG.B4_B, HG.B4_S, 1, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("form", list(HG.B5_FORMS))
@pytest.mark.parametrize("geom,D", HG.B5_CASES, ids=[f"{g}-D{D}" for g, D in HG.B5_CASES])
def test_b5_one_unit_per_wave_kernel(geom, D, form, dt):
    """launch_suffix_r: grid (B, ceil(Hkv / 4)) with a ragged last workgroup; at D = 128 with Hkv >= 4 lengths <= 12 take the packed
    lane-group path, whose idle lane groups (Hkv = 5, 6, 7) shadow the last head and never store."""
    B, S = HG.B5_FORMS[form]
    _suffix_case(geom, D, B, S, 1, dt, lens=HG.b5_lens(B, S), l2=True)


# ---- C. the whole operator ------------------------------------------------------------------------------------------------------
def _oracle(case):
    return O.hydragen_attention(case["q"], case["k"], case["v"], case["shared_ks"], case["shared_vs"], case["shared_cu_seq_lens"],
                                case["shared_max_seq_lens"], case["use_varlens"], case["seq_lens"])


def _single_launch_forms(d):
    """hydragen_attention(**d) issued with single_launch_small 1 and 0 (the spy of test_single_launch_form_of_tiny_problems)."""
    from hydragen_amd import attention as A, _lib

    seen, outs, orig = [], {}, A._launch_decode

    def spy(lib, p, two_stream, stream, single=1):
        p.phase, p.shared_max_workgroups, p.single_launch_small = _lib.HYD_PHASE_ALL, 0, single
        _lib.check(lib.hyd_decode_attn_fused(C.byref(p), stream))
        seen.append(single)

    try:
        for single in (1, 0):
            A._PARAM_CACHE.clear()
            A._launch_decode = lambda lib, p, ts, st, single=single: spy(lib, p, ts, st, single)
            outs[single] = _np(A.hydragen_attention(**d))
    finally:
        A._launch_decode = orig
        A._PARAM_CACHE.clear()
    assert seen == [1, 0]
    return outs


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cid,sizes,geom,D", HG.operator_cases(), ids=[c[0] for c in HG.operator_cases()])
def test_c_hydragen_attention(cid, sizes, geom, D, dt):
    """The decode operator in every form it is issued in: one call, the two-stream form (default and 3 persistent prefix
    workgroups), fp32 partials and, on the first hierarchy, the one-launch form of tiny problems and its two-pass twin."""
    from hydragen_amd import attention as A

    hq, hkv = HG.heads(geom)
    case = HG.operator_case(sizes, geom, D, dt)
    d = case_to_device(case)
    want = _oracle(case)
    flat = O.nosharing_attention(case["q"], case["k"], case["v"], case["shared_ks"], case["shared_vs"],
                                 case["shared_cu_seq_lens"], case["use_varlens"], case["seq_lens"])
    if cid.startswith("split"):  # the level is cut: fp32 split-KV slices go into the suffix epilogue
        B, P = len(sizes[-1]), sizes[0][0]
        assert _plan(dt, B, 1, hq, hkv, D, 1, P)[0] > 1

    forms, orig = [], A._launch_decode  # what each call was issued as: the two-stream labels below are only worth what this shows
    A._launch_decode = lambda lib, p, two, st, *kq: (forms.append(bool(two)), orig(lib, p, two, st, *kq))[1]
    prev_mode, prev_cus = A.set_two_stream("off"), A.TWO_STREAM_PREFIX_CUS
    try:
        outs = {"one call": _np(A.hydragen_attention(**d))}
        A.set_two_stream("on")
        outs["two streams"] = _np(A.hydragen_attention(**d))
        A.TWO_STREAM_PREFIX_CUS = 3  # persistent workgroups (the 4-wave unit at D = 128) walk the prefix units
        A._PARAM_CACHE.clear()
        outs["two streams, 3 prefix workgroups"] = _np(A.hydragen_attention(**d))
        A.set_two_stream("off")
        prev = A.set_f32_partials(True)
        try:
            outs["fp32 partials"] = _np(A.hydragen_attention(**d))
        finally:
            A.set_f32_partials(prev)
    finally:
        A._launch_decode = orig
        A.TWO_STREAM_PREFIX_CUS = prev_cus
        A.set_two_stream(prev_mode)
        A._PARAM_CACHE.clear()
    assert forms == [False, True, True, False], forms
    if cid.startswith("ragged"):
        for single, o in _single_launch_forms(d).items():
            outs[f"single_launch_small = {single}"] = o
    torch.cuda.synchronize()
    for form, got in outs.items():
        _check_out(got, want, dt, f"{cid} {dt}, {form}, vs the decomposed oracle", l2=True)
        _check_out(got, flat, dt, f"{cid} {dt}, {form}, vs plain attention over the concatenated keys", l2=True)


@pytest.mark.parametrize("dt", DTYPES)
def test_c_prefill_shaped_call(dt):
    """nq = 5 with seq_lens = None: prefix passes over 5 x 7 = 35 rows per sequence and kv head, a causal MFMA pass over the unique
    keys, the N-way merge."""
    from hydragen_amd import attention as A

    geom, D, sizes, nq = HG.C_PREFILL
    case = HG.operator_case(sizes, geom, D, dt, nq=nq)
    assert case["seq_lens"] is None and case["k"].shape[1] == nq
    out = A.hydragen_attention(**case_to_device(case))
    torch.cuda.synchronize()
    _check_out(_np(out), _oracle(case), dt, f"prefill-shaped {geom}", l2=True)


# ---- D. fp8 unique caches -------------------------------------------------------------------------------------------------------
def _fp8_problem(geom, B, S, dt, seed, scales="arbitrary"):
    from tests.test_fp8_gqa_gpu import _problem

    hq, hkv = HG.heads(geom)
    q, k8, v8, ks, vs, sl = _problem(np.random.default_rng(seed), (B, hq, hkv, 1, 128, S), dt, scales)
    return q, k8, v8, ks, vs, sl, torch.from_numpy(sl).to(q.device)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,B,S", HG.D_NATIVE_GQA, ids=[g for g, _, _ in HG.D_NATIVE_GQA])
def test_d_fp8_grouped_query_shapes_are_bit_identical_to_the_16bit_kernel(monkeypatch, geom, B, S, dt):
    """suffix_attn_gqa_fp8.hip takes gqa_launch_plan's choices (heads per workgroup, waves per unit) and widens each element to the
    16-bit value dequantize_kv gives: the same bits as the 16-bit kernel, whatever the scales (per-head scales whose products
    do not fit the 16-bit formats included)."""
    from hydragen_amd import flash as F
    from tests.test_fp8_gqa_gpu import _assert_bit_identical

    for i, scales in enumerate(("arbitrary", "caches", None)):
        q, k8, v8, ks, vs, _, sl_t = _fp8_problem(geom, B, S, dt, 11 + B + S + i, scales)
        assert F.fp8_native(q, k8, v8) is True
        _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl_t, f"fp8 {geom} {dt} scales={scales}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,B,S", HG.D_NATIVE_ROWS, ids=[g for g, _, _ in HG.D_NATIVE_ROWS])
def test_d_fp8_token_row_shapes_are_bit_identical_to_the_16bit_kernel(monkeypatch, geom, B, S, dt):
    """12 and 20 MHA heads are native on the fp8 TOKEN-ROW kernel (launch_suffix_rows: 3 and 5 waves per sequence, the launcher and
    the body of the 16-bit kernel).  That kernel folds k_scale into its fp32 score multiplier and multiplies the accumulator by
    v_scale once (suffix_rows.h) where dequantize_kv rounds every fp8 x scale product to 16 bits, so the caches it is
    bit-identical to the 16-bit kernel on are those whose widening is exact and whose scale multiplications change nothing: unit
    scales (k_scale = v_scale = None), which is what the model shell's fp8 arenas start with.  Everything the head count decides --
    which wave takes which heads, which rows it reads and stores, which waves leave -- is the same for every scale.  Per-head scales
    on these shapes are held to the float64 oracle by test_d_fp8_matches_oracle_on_dequantized_caches (a scale read for the wrong
    head fails there) and, here, to the 16-bit kernel on the dequantized caches within the operator's usual gates."""
    from hydragen_amd import flash as F
    from hydragen_amd.kv_quant import dequantize_kv
    from tests.test_fp8_gqa_gpu import _assert_bit_identical, _no_fallback

    q, k8, v8, ks, vs, _, sl_t = _fp8_problem(geom, B, S, dt, 11 + B + S, None)
    assert ks is None and vs is None and F.fp8_native(q, k8, v8) is True
    _assert_bit_identical(monkeypatch, q, k8, v8, ks, vs, sl_t, f"fp8 {geom} {dt}")
    # per-head scales: beside the 16-bit kernel on the dequantized caches to the operator's usual gates (as tests/test_fp8_kv_gpu.py)
    q, k8, v8, ks, vs, sl, sl_t = _fp8_problem(geom, B, S, dt, 11 + B + S, "arbitrary")
    with monkeypatch.context() as m:
        _no_fallback(m)
        o8, l8 = F.flash_attention_seqlen(q, k8, v8, sl_t, k_scale=ks, v_scale=vs)
    o16, l16 = F.flash_attention_seqlen(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), sl_t)
    torch.cuda.synchronize()
    _check_out(_np(o8), _np(o16), dt, f"fp8 {geom} {dt}, per-head scales, vs the 16-bit kernel", l2=True, keep=sl > 0)
    # (no LSE comparison between the two: the 16-bit kernel reads keys ROUNDED to the q dtype, other inputs than the fp8 kernel's, and
    # the 2e-3 LSE bound is one for identical inputs -- the oracle test below holds this kernel's LSE to it on the kernel's own inputs)
    assert torch.equal(torch.isneginf(l8), torch.isneginf(l16))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,B,S", HG.D_FALLBACK, ids=[g for g, _, _ in HG.D_FALLBACK])
def test_d_fp8_shapes_without_a_kernel_say_so(geom, B, S, dt):
    from hydragen_amd import flash as F
    from hydragen_amd.kv_quant import dequantize_kv

    q, k8, v8, ks, vs, _, sl_t = _fp8_problem(geom, B, S, dt, 23)
    assert F.fp8_native(q, k8, v8) is False
    o8, l8 = F.flash_attention_seqlen(q, k8, v8, sl_t, k_scale=ks, v_scale=vs)
    o16, l16 = F.flash_attention_seqlen(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), sl_t)
    torch.cuda.synchronize()
    assert not torch.isnan(o8).any()
    assert torch.equal(o8, o16) and torch.equal(l8, l16)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geom,B,S", HG.D_ORACLE, ids=[g for g, _, _ in HG.D_ORACLE])
def test_d_fp8_matches_oracle_on_dequantized_caches(monkeypatch, geom, B, S, dt):
    """g7x4 on the grouped-query fp8 kernel; 12 and 20 MHA heads on the fp8 token-row kernel with 3 and 5 waves per sequence."""
    from hydragen_amd import flash as F
    from hydragen_amd.kv_quant import dequantize_kv
    from tests.test_fp8_gqa_gpu import _no_fallback

    q, k8, v8, ks, vs, sl, sl_t = _fp8_problem(geom, B, S, dt, 5)
    with monkeypatch.context() as m:
        _no_fallback(m)
        out, lse = F.flash_attention_seqlen(q, k8, v8, sl_t, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    # the oracle reads what the kernel reads (poisoned rows are past the lengths).  Grouped-query kernel: the caches as dequantize_kv
    # widens them to the q dtype for its MFMAs; token-row kernel: fp8 x scale in fp32, never rounded to 16 bits (as tests/test_fp8_kv_gpu.py)
    wide = q.dtype if (geom, B, S) in HG.D_NATIVE_GQA else torch.float32
    kn = dequantize_kv(k8, ks, wide).float().nan_to_num(0.0).cpu().numpy()
    vn = dequantize_kv(v8, vs, wide).float().nan_to_num(0.0).cpu().numpy()
    want, wlse = O.flash_attention_seqlen(_np(q), kn, vn, sl)
    has = sl > 0
    assert np.isfinite(_np(out)).all()
    _check_out(_np(out), want, dt, f"fp8 {geom} {dt}", l2=True, keep=has)
    _check_lse(lse.cpu().numpy(), wlse, f"fp8 {geom} {dt}")
