"""-m gpu: the decode step's glue kernels held to float64 references (tests/glue_ref.py) -- the fused RoPE + K/V append kernel
with 16-bit and fp8 caches (csrc/rope_append.hip), add + RMSNorm and SwiGLU (csrc/layer_ops.hip).

Addressing is tested without a tolerance: tables of {0, +-1, +-1/2} and inputs on a 2^-3 grid make the rotation exact, every
buffer is pre-filled with a sentinel and compared WHOLE, guards included, so a wrong stride, row or bound is a failed
assertion inside the allocation.  Rounding is tested against float64 on the kernel's own fp32 tables with the bound one
round-to-nearest allows.  The entry points are called through the C ABI where the Python faces cannot express a layout."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from hydragen_amd import _lib, layer_ops
from hydragen_amd.flash import _stream
from hydragen_amd.fused_decode import rope_append_decode
from hydragen_amd.kv_quant import FP8_DTYPE, quantize_kv
from hydragen_amd.llama import RotaryTable
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
HEAD_DIMS = [64, 128, 256]
HEADS = [(1, 1), (4, 4), (8, 1), (6, 3)]
BATCHES = [1, 3, 37]
CODE = {torch.float16: _lib.HYD_F16, torch.bfloat16: _lib.HYD_BF16}


# ------------------------------------------------------------------------------------------------------------------------
# hyd_rope_append_decode[_kvq] through the C ABI, every buffer guarded
# ------------------------------------------------------------------------------------------------------------------------
def _rope_abi(q, k, v, q_out, kc, vc, cos, sin, pos, shared, seq_lens, scales=None):
    """q [B, Hq, D], k / v [B, Hkv, D] (heads contiguous, any batch stride), caches [maxB, cache_len, Hkv, D] views with any
    strides (uint8 = fp8 bytes), cos / sin [max_pos, D] row-strided views, pos [B] with any element stride."""
    lib = _lib.load()
    B, Hq, D = q.shape
    assert all(t.shape[1] == 1 or t.stride(1) == D for t in (q, k, v)) and sin.stride() == cos.stride() and cos.stride(1) == 1
    p = _lib.RopeParams()
    p.q, p.k, p.v, p.q_out = q.data_ptr(), k.data_ptr(), v.data_ptr(), q_out.data_ptr()
    p.k_cache, p.v_cache, p.cos, p.sin = kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr()
    p.position_ids, p.seq_lens = pos.data_ptr(), seq_lens.data_ptr()
    if shared is not None:
        p.shared_len = shared.data_ptr()
    p.q_batch_stride, p.k_batch_stride, p.v_batch_stride = q.stride(0), k.stride(0), v.stride(0)
    p.kc_batch_stride, p.kc_tok_stride, p.kc_head_stride = kc.stride(0), kc.stride(1), kc.stride(2)
    p.vc_batch_stride, p.vc_tok_stride, p.vc_head_stride = vc.stride(0), vc.stride(1), vc.stride(2)
    p.pos_stride, p.cs_stride = pos.stride(0), cos.stride(0)
    p.dtype, p.B, p.Hq, p.Hkv, p.D, p.cache_len, p.max_pos = CODE[q.dtype], B, Hq, k.shape[1], D, kc.shape[1], cos.shape[0]
    if kc.dtype == torch.uint8:
        kq = _lib.KvQuant()
        kq.kv_dtype = _lib.HYD_FP8_E4M3
        if scales[0] is not None:
            kq.k_scale, kq.v_scale = scales[0].data_ptr(), scales[1].data_ptr()
        _lib.check(lib.hyd_rope_append_decode_kvq(C.byref(p), C.byref(kq), _stream()))
    else:
        _lib.check(lib.hyd_rope_append_decode(C.byref(p), _stream()))


def _run_exact(c, layout, *, fused_qkv, wide_pos, wide_cs, maxB, fp8=None, table_guard=0, nan_second_half=False):
    """Run the exact case `c` (glue_ref.make_exact_rope_case) in the given layout and compare EVERY output buffer, guards
    included, bit for bit with the float64-derived expectation.  fp8: None (16-bit caches) or a glue_ref.FP8_SCALE_MODES name."""
    dtype, D, Hq, Hkv, B, L, max_pos = c["dtype"], c["D"], c["Hq"], c["Hkv"], c["B"], c["cache_len"], c["max_pos"]
    # inputs: views of one fused projection output, or three tensors
    if fused_qkv:
        qkv = torch.cat([c["q"].reshape(B, -1), c["k"].reshape(B, -1), c["v"].reshape(B, -1)], 1).to(DEV)
        q = qkv[:, : Hq * D].view(B, Hq, D)
        k = qkv[:, Hq * D: (Hq + Hkv) * D].view(B, Hkv, D)
        v = qkv[:, (Hq + Hkv) * D:].view(B, Hkv, D)
    else:
        q, k, v = c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV)
    # tables: NaN everywhere outside the [max_pos, D] window the kernel may read
    off = 4 if wide_cs else 0
    tabs = []
    for t in (c["cos"], c["sin"]):
        wide = torch.full((max_pos + 2 * table_guard, D + 2 * off), float("nan"))
        wide[table_guard: table_guard + max_pos, off: off + D] = t
        if nan_second_half:
            wide[:, off + D // 2:] = float("nan")
        tabs.append(wide.to(DEV)[table_guard: table_guard + max_pos, off: off + D])
    # positions: one column of a wider matrix whose other columns hold other VALID positions
    pos = c["pos"]
    if wide_pos:
        mat = torch.stack([(pos + 7 * j + 1) % max_pos for j in range(5)], 1)
        mat[:, 3] = pos
        pos_dev = mat.to(DEV)[:, 3]
    else:
        pos_dev = pos.to(DEV)
    shared = None if c["shared"] is None else c["shared"].to(DEV)
    # caches and outputs: sentinel-filled, the expectation is built on a host copy of the same buffers
    make = (lambda s, i: R.sentinel8(s, i)) if fp8 else (lambda s, i: R.sentinel16(s, dtype, i))
    host = [make(s, i) for i, s in enumerate(R.cache_buffer_shapes(layout, maxB, L, Hkv, D))]
    dev = [b.to(DEV) for b in host]
    kc, vc = R.cache_views(layout, dev, maxB, L)
    ek, ev = R.cache_views(layout, host, maxB, L)
    scales = (None, None)
    if fp8:
        ks, vs = R.fp8_scales(fp8, Hkv)
        want_k, want_v = quantize_kv(c["want_k"], ks).view(torch.uint8), quantize_kv(c["v"], vs).view(torch.uint8)
        scales = (None, None) if ks is None else (ks.to(DEV), vs.to(DEV))
    else:
        want_k, want_v = c["want_k"], c["v"]
    rows = torch.nonzero(c["written"]).flatten()
    ek[rows, c["idx"][rows]] = want_k[rows]
    ev[rows, c["idx"][rows]] = want_v[rows]
    eq, es = R.sentinel16((B + 2, Hq, D), dtype, 7), torch.full((B + 2,), -77, dtype=torch.int32)
    q_out, seq_lens = eq.to(DEV), es.to(DEV)
    eq[1: B + 1], es[1: B + 1] = c["want_q"], c["seq_lens"]

    _rope_abi(q, k, v, q_out[1: B + 1], kc, vc, tabs[0], tabs[1], pos_dev, shared, seq_lens[1: B + 1], scales)
    torch.cuda.synchronize()

    what = f"{dtype} D={D} heads={Hq}/{Hkv} B={B} {layout} fused_qkv={fused_qkv} wide_pos={wide_pos} wide_cs={wide_cs} fp8={fp8}"
    assert not torch.isnan(q_out[1: B + 1]).any(), what
    assert torch.equal(R.bits(q_out.cpu()), R.bits(eq)), "q_out: " + what
    assert torch.equal(seq_lens.cpu(), es), "seq_lens: " + what
    for name, got, want in zip(("k", "v") if len(dev) == 2 else ("kv",), dev, host):
        got = got.cpu()
        if fp8:  # NaN exactly where the expectation has one (either NaN encoding), every other byte bit for bit
            gn, wn = (got & 0x7F) == 0x7F, (want & 0x7F) == 0x7F
            assert torch.equal(gn, wn), f"{name} cache NaN positions: " + what
            assert torch.equal(got[~wn], want[~wn]), f"{name} cache: " + what
        else:
            assert torch.equal(R.bits(got), R.bits(want)), f"{name} cache: " + what
    return q_out[1: B + 1], dev


def _grid_positions(B, L, with_shared, max_pos=R.EXACT_MAX_POS):
    """Cache indices that cover 0 and L - 1, at positions spread over the whole table when a shared length is given."""
    idx = (np.arange(B) * 3 + (L - 1)) % L
    if B > 1:
        idx[-1] = 0
    if not with_shared:
        return idx, None
    shared = (np.arange(B) * 5 + 2) % (max_pos - L + 1)
    return idx + shared, shared


def _flag_cycle(i):
    return dict(fused_qkv=bool(i & 1), wide_pos=bool(i & 2), wide_cs=bool(i & 4)), bool(i & 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rope_append_16bit_exact_addressing(dtype, D):
    """Part 1: every head / batch shape in every cache layout; the stride variants (fused projection views, pos_stride 5,
    cs_stride D + 8, shared_len given or NULL) cycle so that each meets each layout.  maxB = B + 1: rows above B stay untouched."""
    L, seen = 11, set()
    for i, ((Hq, Hkv), B, layout) in enumerate(itertools.product(HEADS, BATCHES, R.CACHE_LAYOUTS)):
        flags, with_shared = _flag_cycle(i)
        pos, shared = _grid_positions(B, L, with_shared)
        c = R.make_exact_rope_case(dtype, D, Hq, Hkv, B, pos, shared, L)
        _run_exact(c, layout, maxB=B + 1, **flags)
        seen |= {(layout, n, val) for n, val in list(flags.items()) + [("shared", with_shared)]}
    assert len(seen) == 3 * 4 * 2


@pytest.mark.parametrize("fp8", [None, "mixed"], ids=["16bit", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_rope_append_ragged_last_block_in_every_stride_combination(dtype, fp8):
    """B = 37 with 8 query heads on one kv head at D = 64 -- several 256-thread blocks and a ragged last one -- crossed with all
    16 combinations of the stride variants in every cache layout (the grid above only cycles them)."""
    L, (Hq, Hkv), B = 11, (8, 1), 37
    for layout, i in itertools.product(R.CACHE_LAYOUTS, range(16)):
        flags, with_shared = _flag_cycle(i)
        pos, shared = _grid_positions(B, L, with_shared)
        c = R.make_exact_rope_case(dtype, 64, Hq, Hkv, B, pos, shared, L, nan=bool(fp8))
        _run_exact(c, layout, maxB=B + 1, fp8=fp8, **flags)


@pytest.mark.parametrize("fp8", [None, "none"], ids=["16bit", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_rope_append_reads_only_the_first_half_of_the_tables(dtype, fp8):
    """include/hydragen_hip.h: "first D/2 columns are read" -- NaN in the second half of cos / sin changes no bit, in the
    16-bit kernel and in the fp8 kernel (which has its own table loads)."""
    pos, shared = _grid_positions(5, 11, True)
    c = R.make_exact_rope_case(dtype, 128, 6, 3, 5, pos, shared, 11)
    _run_exact(c, "contig", maxB=6, fused_qkv=True, wide_pos=False, wide_cs=True, nan_second_half=True, fp8=fp8)


@pytest.mark.parametrize("fp8", [None, "mixed", "none"], ids=["16bit", "fp8", "fp8-null-scales"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rope_append_clamps_positions_to_the_table(dtype, D, fp8):
    """Part 3: positions in [max_pos, max_pos + g) rotate by row max_pos - 1, positions in [-g, 0) by row 0 -- the tables are the
    inner rows of a larger one whose g = 4 guard rows are NaN, so an unclamped read is a NaN in q_out, not a fault.  Without
    shared_len the cache index is the position: only the in-range rows append (cache_len = max_pos)."""
    g, max_pos = R.GUARD, 16
    pos = np.array([max_pos, max_pos + 1, max_pos + 2, max_pos + g - 1, -1, -2, -3, -g, 0, max_pos - 1, 5])
    c = R.make_exact_rope_case(dtype, D, 6, 3, len(pos), pos, None, max_pos, max_pos=max_pos, nan=bool(fp8))
    assert c["written"].tolist() == [False] * 8 + [True] * 3
    for layout in R.CACHE_LAYOUTS:
        _run_exact(c, layout, maxB=len(pos), fused_qkv=False, wide_pos=True, wide_cs=True, table_guard=g, fp8=fp8)


@pytest.mark.parametrize("fp8", [None, "mixed", "none"], ids=["16bit", "fp8", "fp8-null-scales"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rope_append_writes_nothing_at_or_past_cache_len(dtype, D, fp8):
    """Part 3: a cache index in [cache_len, cache_len + g) writes no K and no V (the caches are [:, :cache_len] of buffers with
    g guard tokens, all compared), q_out is still rotated and seq_lens = index + 1; the neighbouring rows append normally,
    index 0 and cache_len - 1 included."""
    L, g = 6, R.GUARD
    idx = np.array([0, L, L - 1, L + 1, 2, L + g - 1, L - 1, L + 2, 0, L])
    shared = (np.arange(len(idx)) * 3 + 1) % (R.EXACT_MAX_POS - L - g + 1)
    for layout, with_shared in itertools.product(R.CACHE_LAYOUTS, (True, False)):
        c = R.make_exact_rope_case(dtype, D, 4, 2, len(idx), idx + shared * with_shared, shared if with_shared else None, L,
                                   nan=bool(fp8))
        assert c["written"].tolist() == [i < L for i in idx] and torch.equal(c["seq_lens"], torch.from_numpy(idx + 1).int())
        _run_exact(c, layout, maxB=len(idx) + 1, fused_qkv=True, wide_pos=True, wide_cs=False, fp8=fp8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rope_append_fp8_exact_addressing_and_quantization(dtype, D):
    """Part 4: the cache bytes are quantize_kv of the float64-derived rotated K (and of V) -- no 16-bit kernel involved --, in
    every layout (byte strides), with unit, arbitrary (saturating) and absent scales, a NaN in k and in v."""
    L, pairs, i = 11, set(), 0
    for ci, ((Hq, Hkv), B) in enumerate(itertools.product(HEADS, BATCHES)):
        for si, mode in enumerate(R.FP8_SCALE_MODES):
            layout = R.CACHE_LAYOUTS[(ci + si) % 3]
            flags, with_shared = _flag_cycle(i)
            i += 1
            pos, shared = _grid_positions(B, L, with_shared)
            c = R.make_exact_rope_case(dtype, D, Hq, Hkv, B, pos, shared, L, nan=True)
            if mode == "mixed":  # the clamp at +-448 is exercised
                ks, _ = R.fp8_scales(mode, Hkv)
                assert (c["want_k"].float().nan_to_num().abs() / ks[:, None] > 448).any()
            _run_exact(c, layout, maxB=B + 1, fp8=mode, **flags)
            pairs.add((layout, mode))
    assert len(pairs) == 9


def test_exact_case_agrees_with_the_python_face():
    """The contiguous layout once through fused_decode.rope_append_decode (what the model shell calls), 16-bit and fp8."""
    B, L, D = 5, 11, 64
    pos, shared = _grid_positions(B, L, True)
    c = R.make_exact_rope_case(torch.bfloat16, D, 4, 2, B, pos, shared, L)
    args = [c[n].to(DEV)[:, None] for n in ("q", "k", "v")] + [c["cos"].to(DEV), c["sin"].to(DEV), c["pos"].to(DEV)[:, None], c["shared"].to(DEV)]
    for fp8 in (False, True):
        kc = torch.zeros(B, L, 2, D, device=DEV, dtype=torch.uint8 if fp8 else torch.bfloat16)
        vc = torch.zeros_like(kc)
        qo, sl = rope_append_decode(*args, kc.view(FP8_DTYPE) if fp8 else kc, vc.view(FP8_DTYPE) if fp8 else vc)
        assert torch.equal(qo[:, 0].cpu(), c["want_q"]) and torch.equal(sl.cpu(), c["seq_lens"])
        want = quantize_kv(c["want_k"], None).view(torch.uint8) if fp8 else c["want_k"]
        assert torch.equal(R.bits(kc.cpu()[torch.arange(B), c["idx"]]), R.bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("base,max_pos", [(1e4, 4096), (5e5, 8192)])
def test_rope_append_rounds_once(dtype, D, base, max_pos):
    """Part 2: real tables, positions over the whole table (0 and max_pos - 1 included), three input magnitudes.  The reference
    is float64 arithmetic on the fp32 table values the kernel was given (copied off the device), the bound is
    glue_ref.rope_bound: 1/2 ulp16(want) + 2^-22 (|x| + |y|) for every element of q_out and of the appended K; V is a copy."""
    rot = RotaryTable(D, max_pos, base, device=DEV)
    cos, sin = rot.cos_cached.cpu().numpy(), rot.sin_cached.cpu().numpy()
    B, Hq, Hkv, L = 192, 4, 2, 8
    for i, scale in enumerate((1.0, 2.0 ** -10, 100.0)):
        g = torch.Generator().manual_seed(1000 * D + 10 * int(max_pos) + i)
        q, k, v = ((torch.randn(B, 1, H, D, generator=g) * scale).to(dtype) for H in (Hq, Hkv, Hkv))
        pos = torch.randint(0, max_pos, (B,), generator=g)
        pos[:2] = torch.tensor([0, max_pos - 1])
        idx = torch.minimum(torch.arange(B) % L, pos)
        kc = R.sentinel16((B, L, Hkv, D), dtype).to(DEV)
        vc = R.sentinel16((B, L, Hkv, D), dtype, 1).to(DEV)
        qo, sl = rope_append_decode(q.to(DEV), k.to(DEV), v.to(DEV), rot.cos_cached, rot.sin_cached, pos[:, None].to(DEV),
                                    (pos - idx).to(DEV), kc, vc)
        assert torch.equal(sl.cpu(), (idx + 1).int())
        bi = torch.arange(B)
        assert torch.equal(R.bits(vc.cpu()[bi, idx]), R.bits(v[:, 0]))  # V bit for bit
        for name, got, x in (("q", qo[:, 0].cpu(), q[:, 0]), ("k", kc.cpu()[bi, idx], k[:, 0])):
            x64 = x.double().numpy()
            want = R.rope_ref64(x64, cos[pos.numpy()], sin[pos.numpy()])
            ratio = np.abs(got.double().numpy() - want) / R.rope_bound(want, x64, dtype)
            assert ratio.max() <= 1.0, (name, scale, float(ratio.max()))


# ------------------------------------------------------------------------------------------------------------------------
# hyd_add_rmsnorm
# ------------------------------------------------------------------------------------------------------------------------
def _slice_of(rows, n, pad, dtype, salt):
    """(host sentinel matrix [rows + 1, n + 2 * pad], device copy): the operand is columns [pad, pad + n) of the first rows."""
    h = R.sentinel16((rows + 1, n + 2 * pad), dtype, salt)
    return h, h.to(DEV)


def _norm_abi(x, r, w, s, o, rows, n, eps=1e-5):
    """x / r / s / o: [rows, n] column-slice views (r, s may be None); returns the entry point's code."""
    p = _lib.AddRmsnormParams()
    p.x, p.weight, p.norm_out, p.x_row_stride, p.norm_row_stride = x.data_ptr(), w.data_ptr(), o.data_ptr(), x.stride(0), o.stride(0)
    if r is not None:
        p.residual, p.residual_row_stride = r.data_ptr(), r.stride(0)
    if s is not None:
        p.sum_out, p.sum_row_stride = s.data_ptr(), s.stride(0)
    p.rows, p.n, p.dtype, p.eps = rows, n, CODE[x.dtype], eps
    rc = _lib.load().hyd_add_rmsnorm(C.byref(p), _stream())
    torch.cuda.synchronize()
    return rc


def _norm_case(x, r, w, eps=1e-5, alias=None):
    """Run host tensors x / r [rows, n], w [n] through the ABI with four DIFFERENT row strides, every operand a column slice of
    a sentinel matrix; check guards, the stored sum bit for bit and the norm within the elementwise bound.  alias: None, or
    'residual' / 'x' = sum_out is that operand."""
    rows, n = x.shape
    dtype = x.dtype
    pads = dict(x=8, r=16, s=24, o=32)
    hx, dx = _slice_of(rows, n, pads["x"], dtype, 1)
    hr, dr = _slice_of(rows, n, pads["r"], dtype, 2)
    hs, ds = _slice_of(rows, n, pads["s"], dtype, 3)
    ho, do = _slice_of(rows, n, pads["o"], dtype, 4)
    view = lambda m, name: m[:rows, pads[name]: pads[name] + n]  # noqa: E731
    view(hx, "x")[:] = x
    dx.copy_(hx)
    if r is not None:
        view(hr, "r")[:] = r
        dr.copy_(hr)
    want_sum, want = R.add_rmsnorm_ref64(x, r, w, eps)
    s_view = None if r is None else {None: view(ds, "s"), "residual": view(dr, "r"), "x": view(dx, "x")}[alias]
    rc = _norm_abi(view(dx, "x"), None if r is None else view(dr, "r"), w.to(DEV), s_view, view(do, "o"), rows, n, eps)
    assert rc == 0, _lib.load().hyd_last_error_string()
    if r is not None:
        view({None: hs, "residual": hr, "x": hx}[alias], {None: "s", "residual": "r", "x": "x"}[alias])[:] = want_sum
    got = view(do.cpu(), "o")
    for name, h, d in (("x", hx, dx), ("residual", hr, dr), ("sum_out", hs, ds)):
        assert torch.equal(R.bits(d.cpu()), R.bits(h)), f"{name} buffer (operand, stored sum or guards) n={n} alias={alias}"
    ho_want = ho.clone()
    view(ho_want, "o")[:] = got
    assert torch.equal(R.bits(do.cpu()), R.bits(ho_want)), f"norm_out guards n={n}"
    return got, want, want_sum


def _assert_norm_close(got, want, dtype, what=""):
    err = (got.double() - want).abs()
    bound = R.REL_HALF_ULP[dtype] * want.abs() + 1e-6
    assert (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("n", [2040, 2048, 2056, 4088, 4096, 4104, 6144, 8184, 8192, 8200, 12288, 16376, 16384])
def test_add_rmsnorm_at_the_instantiation_boundaries(dtype, n, with_residual):
    """Part 5: on, just below and just above every switch between the NV = 1, 2, 4, 8 register tiles and at the upper limit,
    through the C ABI with four different row strides and guard columns."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(3, n, generator=g).to(dtype)
    r = (3 * torch.randn(3, n, generator=g)).to(dtype) if with_residual else None
    w = (1 + 0.1 * torch.randn(n, generator=g)).to(dtype)
    got, want, _ = _norm_case(x, r, w)
    _assert_norm_close(got, want, dtype, n)


def test_add_rmsnorm_refuses_rows_wider_than_16384():
    dtype, n = torch.bfloat16, 16392
    hx, dx = _slice_of(3, n, 8, dtype, 1)
    hs, ds = _slice_of(3, n, 8, dtype, 2)
    ho, do = _slice_of(3, n, 8, dtype, 3)
    w = torch.ones(n, dtype=dtype, device=DEV)
    rc = _norm_abi(dx[:3, 8: 8 + n], dx[:3, 8: 8 + n], w, ds[:3, 8: 8 + n], do[:3, 8: 8 + n], 3, n)
    assert rc == -2  # HYD_ERR_UNSUPPORTED
    for h, d in ((hx, dx), (hs, ds), (ho, do)):
        assert torch.equal(R.bits(d.cpu()), R.bits(h))  # nothing was written
    with pytest.raises(NotImplementedError):
        layer_ops.add_rms_norm(dx[:3, 8: 8 + n], None, w, 1e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n", [520, 4104, 16384])
def test_add_rmsnorm_sum_out_may_alias_residual_or_x(dtype, n):
    """include/hydragen_hip.h: "sum_out may alias residual or x" -- bit-equal to the call with a separate sum_out."""
    g = torch.Generator().manual_seed(n + 1)
    x, r = torch.randn(3, n, generator=g).to(dtype), (3 * torch.randn(3, n, generator=g)).to(dtype)
    w = (1 + 0.1 * torch.randn(n, generator=g)).to(dtype)
    base, want, _ = _norm_case(x, r, w)
    _assert_norm_close(base, want, dtype, n)
    for alias in ("residual", "x"):
        got, _, _ = _norm_case(x, r, w, alias=alias)  # (checks that the aliased operand now holds the rounded sum)
        assert torch.equal(R.bits(got), R.bits(base)), alias


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_add_rmsnorm_value_edges(dtype):
    """An all-zero row gives zeros; rows scaled by 2^-12 and 2^6 are held to the float64 formula WITH eps (eps = 1e-5 against a
    mean square of about 2^-24: not scale invariance); an f16 sum that overflows is inf in sum_out exactly where the
    float64-then-rounded sum is."""
    n = 4104
    g = torch.Generator().manual_seed(3)
    row = torch.randn(n, generator=g)
    x = torch.stack([torch.zeros(n), row, row * 2.0 ** -12, row * 2.0 ** 6]).to(dtype)
    w = (1 + 0.1 * torch.randn(n, generator=g)).to(dtype)
    for r in (None, torch.zeros_like(x)):
        got, want, _ = _norm_case(x, r, w)
        assert (got[0] == 0).all() and not torch.isnan(got).any()
        _assert_norm_close(got, want, dtype)
    assert (want[2] / want[1]).median() < 0.1  # eps dominates the small row: the expectation is not the unscaled row's
    if dtype == torch.float16:
        big = row.clamp(-3, 3) * 20000  # finite in f16; where |big| > 32760 the sum is not
        x = torch.stack([big, row]).to(dtype)
        r = torch.stack([big, row * 0.5]).to(dtype)
        got, want, want_sum = _norm_case(x, r, w)  # (the stored sum is compared bit for bit inside)
        assert torch.isinf(want_sum[0]).any() and torch.isfinite(want_sum[0]).any()
        # row 0 holds inf: its mean square is inf and its norm NaN / 0 in the kernel and in float64 alike.  Only its sum_out is
        # held to the reference (inside _norm_case); of its norm_out only that it is not passed off as finite.
        assert not torch.isfinite(got[0]).all()
        _assert_norm_close(got[1], want[1], dtype)


# ------------------------------------------------------------------------------------------------------------------------
# hyd_swiglu
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("up", [1.0, -3.5, 2.0 ** -10, 240.0])
def test_swiglu_over_every_16bit_gate(dtype, up):
    """Part 6: all 65536 gate bit patterns in one launch against float64 gate / (1 + exp(-gate)) * up."""
    gate = R.all_bit_patterns(dtype)
    upt = torch.full_like(gate, up)
    got = layer_ops.swiglu(gate.to(DEV), upt.to(DEV)).cpu()
    want = R.swiglu_ref64(gate, upt)
    rounded = want.to(dtype)  # one rounding: where the reference leaves the dtype's range
    nan = torch.isnan(want)
    assert torch.equal(nan, torch.isnan(gate) | (gate == -float("inf")))
    assert torch.equal(torch.isnan(got), nan)  # NaN exactly where the formula's is (NaN and -inf gates)
    over = torch.isinf(rounded) & ~nan
    assert over[gate == float("inf")].all() and (gate[over & torch.isinf(gate)] > 0).all()
    assert (over & torch.isfinite(gate)).any() == (abs(up) > 1)  # finite gates overflow the dtype only through a large `up`
    assert torch.equal(got[over], rounded[over])  # the same signed infinity (+inf gates included)
    fin = ~nan & ~over
    assert torch.isfinite(gate[fin]).all() and torch.isfinite(got[fin]).all()
    err = (got.double() - want).abs()[fin]
    assert (err <= R.REL_HALF_ULP[dtype] * want.abs()[fin] + 1e-6).all(), float(err.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_swiglu_independent_row_strides(dtype):
    rows, n = 3, 264
    g = torch.Generator().manual_seed(9)
    gate, up = (2 * torch.randn(rows, n, generator=g)).to(dtype), (2 * torch.randn(rows, n, generator=g)).to(dtype)
    hg, dg = _slice_of(rows, n, 8, dtype, 1)
    hu, du = _slice_of(rows, n, 16, dtype, 2)
    ho, do = _slice_of(rows, n, 24, dtype, 3)
    hg[:rows, 8: 8 + n], hu[:rows, 16: 16 + n] = gate, up
    dg.copy_(hg)
    du.copy_(hu)
    p = _lib.SwigluParams()
    p.gate, p.up, p.out = dg[:rows, 8:].data_ptr(), du[:rows, 16:].data_ptr(), do[:rows, 24:].data_ptr()
    p.gate_row_stride, p.up_row_stride, p.out_row_stride = dg.stride(0), du.stride(0), do.stride(0)
    p.rows, p.n, p.dtype = rows, n, CODE[dtype]
    _lib.check(_lib.load().hyd_swiglu(C.byref(p), _stream()))
    torch.cuda.synchronize()
    got = do.cpu()[:rows, 24: 24 + n]
    want = R.swiglu_ref64(gate, up)
    assert ((got.double() - want).abs() <= R.REL_HALF_ULP[dtype] * want.abs() + 1e-6).all()
    ho[:rows, 24: 24 + n] = got
    assert torch.equal(R.bits(do.cpu()), R.bits(ho))  # guard columns and the guard row of out
    assert torch.equal(R.bits(dg.cpu()), R.bits(hg)) and torch.equal(R.bits(du.cpu()), R.bits(hu))
