"""CPU: the references, exact test data and bounds of tests/glue_ref.py held to their own claims, so that the GPU tests of
tests/test_decode_glue_gpu.py compare the kernels with something that is itself checked -- and an fp32 emulation of the RoPE
kernel's arithmetic that keeps the derived rounding bound honest without a GPU."""
import numpy as np
import pytest
import torch

from hydragen_amd.kv_quant import quantize_kv
from hydragen_amd.llama import RotaryTable, apply_rotary_pos_emb
from tests import glue_ref as R

DTYPES = [torch.bfloat16, torch.float16]
HEAD_DIMS = [64, 128, 256]
TABLES = [(1e4, 4096), (5e5, 8192)]
MAGNITUDES = [1.0, 2.0 ** -10, 100.0]


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("max_pos", [R.EXACT_MAX_POS, 16])
def test_exact_tables_are_distinguishable(D, max_pos):
    cos, sin = R.exact_tables(D, max_pos)
    assert cos.shape == sin.shape == (max_pos, D) and cos.dtype == sin.dtype == np.float32
    assert set(np.unique(cos)) <= set(R.EXACT_VALUES) and set(np.unique(sin)) <= set(R.EXACT_VALUES)
    assert np.array_equal(cos[:, : D // 2], cos[:, D // 2:]) and np.array_equal(sin[:, : D // 2], sin[:, D // 2:])
    assert not ((cos == 0) & (sin == 0)).any()
    assert R.tables_distinguishable(cos, sin)
    c2 = cos.copy()
    c2[3], s2 = c2[7], sin.copy()
    s2[3] = s2[7]
    assert not R.tables_distinguishable(c2, s2)  # the check itself notices two equal rows


def test_exact_inputs_encode_their_index():
    q, k, v = R.exact_inputs(37, 8, 3, 256)
    for x in (q, k, v):
        assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() <= 63 / 8
        assert (x[1:] != x[:-1]).all() and (x[:, 1:] != x[:, :-1]).all() and (x[..., 1:] != x[..., :-1]).all()
        assert (x[..., 8:] != x[..., :-8]).all() and (x[..., 127:] != x[..., :-127]).all()
        for half in (32, 64, 128):
            assert (x[..., half:] != x[..., :-half]).all()
    assert (k != v).all() and (q[:, :3] != k).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_exact_rope_case_is_exact_in_both_dtypes(dtype, D):
    """make_exact_rope_case refuses (asserts) any value the dtype cannot hold; the float64 expectation is also what the
    prefill path's torch formula gives in float64, at clamped, negative and shared-offset positions."""
    B = 9
    pos = np.array([0, 23, 24, 27, -1, -4, 5, 11, 17])
    c = R.make_exact_rope_case(dtype, D, 6, 3, B, pos, None, cache_len=12)
    assert torch.equal(c["seq_lens"], torch.from_numpy(pos + 1).int())
    assert c["written"].tolist() == [True, False, False, False, False, False, True, True, False]
    rows = torch.from_numpy(np.clip(pos, 0, 23))[:, None]
    qr, kr = apply_rotary_pos_emb(c["q"].double()[:, None], c["k"].double()[:, None], c["cos"].double(), c["sin"].double(), rows)
    assert torch.equal(qr[:, 0], c["want_q"].double()) and torch.equal(kr[:, 0], c["want_k"].double())
    assert c["want_q"].abs().max() <= 15.75
    shared = np.arange(B) % 5
    c2 = R.make_exact_rope_case(dtype, D, 6, 3, B, pos, shared, cache_len=12)
    assert torch.equal(c2["idx"], torch.from_numpy(pos - shared)) and torch.equal(c2["want_k"], c["want_k"])


def test_exact_fp8_expectation_saturates_and_keeps_nan():
    """What part 4 of the GPU module expects is quantize_kv of the float64-derived 16-bit values: with the mixed scales it must
    reach +-448 (the clamp is exercised) and hold NaN exactly at the injected element and its rotation partner."""
    c = R.make_exact_rope_case(torch.bfloat16, 64, 4, 4, 5, np.arange(5), None, cache_len=8, nan=True)
    ks, vs = R.fp8_scales("mixed", 4)
    assert (ks >= 4).any() and (ks <= 2.0 ** -6).any() and (vs >= 4).any() and (vs <= 2.0 ** -6).any()
    for Hkv in (1, 3, 4):
        a, b = R.fp8_scales("mixed", Hkv)
        both = torch.cat([a, b])
        assert (both >= 4).any() and (both <= 2.0 ** -6).any()
    k8, v8 = quantize_kv(c["want_k"], ks).float(), quantize_kv(c["v"], vs).float()
    assert (k8.abs() == 448).any() and (v8.abs() == 448).any()
    assert torch.isnan(k8).nonzero().tolist() == [[2, 3, 5], [2, 3, 37]] and torch.isnan(v8).nonzero().tolist() == [[4, 0, 7]]
    assert not (R.sentinel8((4096,)) % 128 == 127).any()


def test_ulp16_and_bound():
    w = np.array([1.0, 1.5, 2.0, -3.0, 0.0, 2.0 ** -14, 2.0 ** -20, 2.0 ** -126, 2.0 ** -130, 65504.0])
    assert R.ulp16(w, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -21, 2.0 ** -27,
                                                     2.0 ** -133, 2.0 ** -133, 2.0 ** 8]
    assert R.ulp16(w, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24,
                                                    2.0 ** -24, 2.0 ** -24, 2.0 ** 5]
    for dtype in DTYPES:  # the spacing really is the dtype's: next representable value above |w|
        t = torch.tensor(w[[0, 1, 2, 5]], dtype=dtype)
        up = (R.bits(t) + 1).view(dtype)
        assert np.array_equal((up.double() - t.double()).numpy(), R.ulp16(t.double().numpy(), dtype))
    x = np.array([[[3.0, -1.0, 0.5, 0.0]]])
    b = R.rope_bound(np.array([[[1.0, 1.0, 1.0, 1.0]]]), x, torch.float16)
    assert np.allclose(b - 2.0 ** -11, 2.0 ** -22 * np.array([3.5, 1.0, 3.5, 1.0]), rtol=0, atol=0)


def _rope_rounding_case(dtype, D, base, max_pos, scale, rows, seed):
    rot = RotaryTable(D, max_pos, base, device="cpu")
    cos, sin = rot.cos_cached.numpy(), rot.sin_cached.numpy()
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, 1, D, generator=g) * scale).to(dtype)
    pos = torch.randint(0, max_pos, (rows,), generator=g).numpy()
    pos[:2] = [0, max_pos - 1]
    x64 = x.double().numpy()
    return x64, cos[pos], sin[pos], R.rope_ref64(x64, cos[pos], sin[pos])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("base,max_pos", TABLES)
def test_fp32_emulation_of_the_rope_kernel_meets_the_derived_bound(dtype, D, base, max_pos):
    """fp32 tables, fp32 products, one rounding -- with and without FMA contraction -- stays inside
    1/2 ulp16(want) + 2^-22 (|x| + |y|) of float64 on the same fp32 table values, over 4096 rows per magnitude; the same
    arithmetic with cos / sin rounded to the 16-bit dtype first (the prefill path's torch form) does not."""
    for i, scale in enumerate(MAGNITUDES):
        x64, cr, sr, want = _rope_rounding_case(dtype, D, base, max_pos, scale, 4096, 100 * D + i)
        bound = R.rope_bound(want, x64, dtype)
        for mode in R.ROPE_FP32_MODES:
            got = R.rope_emulate_fp32(x64, cr, sr, dtype, mode).double().numpy()
            ratio = np.abs(got - want) / bound
            assert ratio.max() <= 1.0, (scale, mode, float(ratio.max()))
        c16 = torch.from_numpy(cr).to(dtype).float().numpy()
        s16 = torch.from_numpy(sr).to(dtype).float().numpy()
        bad = R.rope_emulate_fp32(x64, c16, s16, dtype).double().numpy()
        assert (np.abs(bad - want) > bound).any(), (scale, "16-bit tables went unnoticed")


@pytest.mark.parametrize("dtype", DTYPES)
def test_glue_references_agree_with_torch_float64(dtype):
    g = torch.Generator().manual_seed(5)
    x, r = torch.randn(3, 520, generator=g).to(dtype), (3 * torch.randn(3, 520, generator=g)).to(dtype)
    w = (1 + 0.1 * torch.randn(520, generator=g)).to(dtype)
    s, nrm = R.add_rmsnorm_ref64(x, r, w, 1e-5)
    assert torch.equal(s, (x.float() + r.float()).to(dtype))
    want = torch.nn.functional.rms_norm(s.double(), (520,), w.double(), float(np.float32(1e-5)))
    assert torch.allclose(nrm, want, rtol=1e-13, atol=0)
    s0, n0 = R.add_rmsnorm_ref64(x, None, w, 1e-5)
    assert s0 is x and torch.allclose(n0, torch.nn.functional.rms_norm(x.double(), (520,), w.double(), float(np.float32(1e-5))), rtol=1e-13, atol=0)
    gate = R.all_bit_patterns(dtype)
    assert gate.shape == (1, 65536) and len(set(R.bits(gate).flatten().tolist())) == 65536
    ref = R.swiglu_ref64(gate, torch.full_like(gate, -3.5))
    fin = torch.isfinite(gate) & (gate.double().abs() < 700)
    silu = torch.nn.functional.silu(gate.double()) * -3.5
    assert torch.allclose(ref[fin], silu[fin], rtol=1e-13, atol=0)
    assert torch.equal(torch.isnan(ref), torch.isnan(gate) | (gate == -float("inf")))
    assert (ref[gate == float("inf")] == -float("inf")).all()
    assert (ref[torch.isfinite(gate) & (gate.double() < -800)] == 0).all()  # exp overflows to inf: -x / inf = -0, times up


@pytest.mark.parametrize("layout", R.CACHE_LAYOUTS)
def test_cache_layout_views(layout):
    maxB, L, Hkv, D = 3, 5, 2, 64
    bufs = [R.sentinel16(s, torch.float16, i) for i, s in enumerate(R.cache_buffer_shapes(layout, maxB, L, Hkv, D))]
    k, v = R.cache_views(layout, bufs, maxB, L)
    assert k.shape == v.shape == (maxB, L, Hkv, D) and k.stride(3) == 1 and k.data_ptr() != v.data_ptr()
    assert all(st % 8 == 0 for st in k.stride()[:3]) and k.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
    if layout == "head_major":
        assert k.stride(2) > k.stride(1)
    if layout == "fused":
        assert k.stride(1) == 2 * Hkv * D and v.data_ptr() - k.data_ptr() == 2 * Hkv * D
    # the guard tokens behind cache_len of the same sequence and head are inside the buffer
    for c, buf in ((k, bufs[0]), (v, bufs[-1])):
        assert c[maxB - 1, L - 1, Hkv - 1].storage_offset() + R.GUARD * c.stride(1) + D <= buf.numel()
