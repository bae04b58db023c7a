"""float64 references, exact test data and derived error bounds for the decode-step glue kernels (rope_append.hip,
layer_ops.hip: hyd_rope_append_decode[_kvq], hyd_add_rmsnorm, hyd_swiglu).  CPU only (numpy / torch on the host):
tests/test_decode_glue.py holds these helpers to their own claims, tests/test_decode_glue_gpu.py holds the kernels to them.

Nothing here is measured on a kernel: every bound is the precision of a number format or a stated argument."""
import numpy as np
import torch

M_BITS = {torch.bfloat16: 7, torch.float16: 10}       # stored mantissa bits
E_MIN = {torch.bfloat16: -126, torch.float16: -14}    # exponent of the smallest normal number
REL_HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # the elementwise bound of tests/test_layer_ops_gpu.py

# ------------------------------------------------------------------------------------------------------------------------
# RoPE + append with EXACT arithmetic: tables of {0, +-1, +-1/2} and inputs on a 2^-3 grid
# ------------------------------------------------------------------------------------------------------------------------
EXACT_VALUES = np.array([0.0, 1.0, -1.0, 0.5, -0.5], dtype=np.float32)
EXACT_MAX_POS = 24  # rows of the exact tables (small: every row is used, and the guarded variants stay tiny)


def exact_tables(D, max_pos=EXACT_MAX_POS):
    """(cos, sin) fp32 [max_pos, D]: every (row, pair column) cell draws its own (cos, sin) from {0, +-1, +-1/2}^2 without
    (0, 0) (a cell that would erase its inputs); columns d and d + D/2 hold the same value (rotate-half convention).  These
    are not a rotation -- the kernel takes the tables as arguments and only multiplies and adds."""
    rng = np.random.default_rng(1000 + D)
    code = rng.integers(1, 25, (max_pos, D // 2))
    cos, sin = EXACT_VALUES[code // 5], EXACT_VALUES[code % 5]
    return np.concatenate([cos, cos], 1), np.concatenate([sin, sin], 1)


def tables_distinguishable(cos, sin):
    """Every table row differs from every other one inside every 8-column chunk (what one thread reads), and every pair
    column differs from every other one: a kernel that reads a wrong row or column computes something else."""
    half = cos.shape[1] // 2
    cell = (cos[:, :half] * 4).astype(np.int64) * 16 + (sin[:, :half] * 4).astype(np.int64)  # one code per (cos, sin)
    for c0 in range(0, half, 8):
        if len({tuple(r) for r in cell[:, c0:c0 + 8]}) != cell.shape[0]:
            return False
    return len({tuple(c) for c in cell.T}) == half


def exact_inputs(B, Hq, Hkv, D):
    """q [B, Hq, D], k, v [B, Hkv, D] float64: multiples of 2^-3 in [-63/8, 63/8] that encode (tensor, b, head, d) -- changing
    any one of b, head or d by less than 127, or d by D/2, changes the value (127 is prime, no multiplier divides it).  With
    the exact tables x*c - y*s is a multiple of 2^-4 of magnitude <= 15.75: at most 8 significant bits, exact in bf16 and f16."""
    def one(t, H):
        b, h, d = np.meshgrid(np.arange(B), np.arange(H), np.arange(D), indexing="ij")
        return (((b * 41 + h * 17 + d * 5 + (d // 127) * 3 + t * 59) % 127) - 63) / 8.0
    return one(0, Hq), one(1, Hkv), one(2, Hkv)


def rope_ref64(x, cos_rows, sin_rows):
    """x [B, H, D] float64 rotated by one table row per b (cos_rows / sin_rows [B, D], only the first D/2 columns are read):
    out[:D/2] = x1*c - x2*s, out[D/2:] = x2*c + x1*s, the rotate-half form of include/hydragen_hip.h."""
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    c, s = cos_rows[:, None, :half].astype(np.float64), sin_rows[:, None, :half].astype(np.float64)
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def to_dtype_exact(x64, dtype):
    """float64 numpy -> torch `dtype`, refusing any value the dtype cannot hold exactly (NaN stays NaN)."""
    t = torch.from_numpy(np.ascontiguousarray(x64)).to(dtype)
    back = t.double().numpy()
    assert np.array_equal(back, x64, equal_nan=True), "value not representable in " + str(dtype)
    return t


def make_exact_rope_case(dtype, D, Hq, Hkv, B, pos, shared, cache_len, max_pos=EXACT_MAX_POS, nan=False):
    """One exact-arithmetic call: inputs, tables and the float64-derived expectation (all host tensors).  pos int64 [B]
    absolute positions (clamped to the table as the header states), shared int64 [B] or None; the cache index is pos - shared,
    rows whose index is outside [0, cache_len) write nothing, seq_lens = index + 1 regardless."""
    cos, sin = exact_tables(D, max_pos)
    q, k, v = exact_inputs(B, Hq, Hkv, D)
    if nan:  # NaN passes through the fp8 quantizer; RoPE spreads k's to its rotation partner
        k[B // 2, Hkv - 1, 5] = np.nan
        v[B - 1, 0, 7] = np.nan
    pos = np.asarray(pos, dtype=np.int64)
    rows = np.clip(pos, 0, max_pos - 1)
    idx = pos - (0 if shared is None else np.asarray(shared, dtype=np.int64))
    return dict(
        dtype=dtype, D=D, Hq=Hq, Hkv=Hkv, B=B, max_pos=max_pos, cache_len=cache_len,
        q=to_dtype_exact(q, dtype), k=to_dtype_exact(k, dtype), v=to_dtype_exact(v, dtype),
        cos=torch.from_numpy(cos), sin=torch.from_numpy(sin),
        pos=torch.from_numpy(pos), shared=None if shared is None else torch.from_numpy(np.asarray(shared, dtype=np.int64)),
        want_q=to_dtype_exact(rope_ref64(q, cos[rows], sin[rows]), dtype),
        want_k=to_dtype_exact(rope_ref64(k, cos[rows], sin[rows]), dtype),
        idx=torch.from_numpy(idx), written=torch.from_numpy((idx >= 0) & (idx < cache_len)),
        seq_lens=torch.from_numpy((idx + 1).astype(np.int32)))


# ------------------------------------------------------------------------------------------------------------------------
# RoPE rounding: float64 on the kernel's own fp32 table values, and the bound one rounding allows
# ------------------------------------------------------------------------------------------------------------------------
def ulp16(want, dtype):
    """Spacing of `dtype` at |want| (float64 array): 2^(max(floor(log2 |want|), e_min) - m)."""
    _, e = np.frexp(np.abs(want))  # |want| = f * 2^e with f in [1/2, 1): floor(log2 |want|) = e - 1
    ex = np.where(want == 0, E_MIN[dtype], np.maximum(e - 1, E_MIN[dtype]))
    return np.ldexp(1.0, ex - M_BITS[dtype])


def rope_bound(want, x, dtype):
    """|got - want| <= 1/2 ulp16(want) + 2^-22 (|x| + |y|), x and y the two inputs of the element's pair (x [.., D] float64,
    the kernel's input widened).  First term: one round-to-nearest to the 16-bit dtype.  Second: the fp32 evaluation -- two
    products and a sum, each within 2^-24 relative, |cos|, |sin| <= 1, so the fp32 value is within 2^-23 (|x| + |y|) of the
    exact one whether or not the compiler contracts a product into an FMA -- doubled for the case where that error moves the
    value across a rounding boundary into a binade with a twice larger spacing."""
    half = x.shape[-1] // 2
    a = np.abs(x[..., :half]) + np.abs(x[..., half:])
    return 0.5 * ulp16(want, dtype) + 2.0 ** -22 * np.concatenate([a, a], -1)


ROPE_FP32_MODES = ("separate", "fma_first", "fma_second")


def rope_emulate_fp32(x, cos_rows, sin_rows, dtype, mode="separate"):
    """fp32 emulation of the kernel's arithmetic: fp32 tables, fp32 products, fp32 sum, ONE rounding to dtype.  x [B, H, D]
    holds 16-bit values (any float array), cos_rows / sin_rows [B, D] fp32.  mode: how the compiler may have contracted
    a*b -+ c*d: not at all, or into an FMA that keeps the first or the second product exact."""
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half].astype(np.float32), x[..., half:].astype(np.float32)
    c, s = cos_rows[:, None, :half].astype(np.float32), sin_rows[:, None, :half].astype(np.float32)

    def mul_add(a, b, p, q, sign):  # a*b + sign*p*q
        if mode == "separate":
            return a * b + np.float32(sign) * (p * q)
        if mode == "fma_first":   # fma(a, b, +-fl(p*q)): a*b is exact in float64 (16 x 24 bits)
            return (a.astype(np.float64) * b + sign * (p * q).astype(np.float64)).astype(np.float32)
        return ((a * b).astype(np.float64) + sign * (p.astype(np.float64) * q)).astype(np.float32)

    out = np.concatenate([mul_add(x1, c, x2, s, -1.0), mul_add(x2, c, x1, s, 1.0)], -1)
    return torch.from_numpy(out).to(dtype)


# ------------------------------------------------------------------------------------------------------------------------
# Sentinels, guarded buffers and the cache layouts (pure view functions: the same on a host and a device copy)
# ------------------------------------------------------------------------------------------------------------------------
def sentinel16(shape, dtype, salt=0):
    """A 16-bit tensor of `dtype` whose bit patterns change from element to element (compare it as int16)."""
    n = int(np.prod(shape))
    bits = ((np.arange(n, dtype=np.int64) * 40503 + 977 + 7919 * salt) % 65536).astype(np.uint16).view(np.int16)
    return torch.from_numpy(bits).view(dtype).reshape(shape)


def sentinel8(shape, salt=0):
    """uint8 sentinel bytes in [0, 126]: never an e4m3fn NaN (0x7f / 0xff)."""
    n = int(np.prod(shape))
    return torch.from_numpy(((np.arange(n, dtype=np.int64) * 37 + 11 + 53 * salt) % 127).astype(np.uint8)).reshape(shape)


def bits(t):
    """Any 16-bit or 8-bit tensor as integers, for bit-for-bit comparison."""
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8)


CACHE_LAYOUTS = ("contig", "fused", "head_major")
GUARD = 4  # guard tokens behind cache_len (and guard rows around the rotary tables)


def cache_buffer_shapes(layout, maxB, cache_len, Hkv, D, guard=GUARD):
    """Shapes of the buffers that hold the K and V caches [maxB, cache_len, Hkv, D] with `guard` tokens behind every
    sequence and whole guard sequences around them.  What each layout varies: contig and fused differ in the batch and token
    strides (fused: token stride 2 Hkv D, K and V one buffer) but both keep the head stride at D; only head_major has a head
    stride other than D, and only with Hkv > 1 does a head stride matter at all -- a kernel that used D for it is caught by the
    head_major cases with more than one kv head, nowhere else."""
    if layout == "contig":       # token-major, the layout setup_caches allocates
        return [(maxB + 1, cache_len + guard, Hkv, D)] * 2
    if layout == "fused":        # K and V are the two halves of ONE buffer: token stride 2 Hkv D
        return [(maxB + 2, cache_len + guard, 2, Hkv, D)]
    if layout == "head_major":   # [maxB, Hkv, maxS, D] viewed token-major: head stride > token stride
        return [(maxB + 1, Hkv, cache_len + guard, D)] * 2
    raise ValueError(layout)


def cache_views(layout, bufs, maxB, cache_len):
    """(k_cache, v_cache) views [maxB, cache_len, Hkv, D] of the buffers of cache_buffer_shapes."""
    if layout == "contig":
        return bufs[0][:maxB, :cache_len], bufs[1][:maxB, :cache_len]
    if layout == "fused":
        return bufs[0][1:maxB + 1, :cache_len, 0], bufs[0][1:maxB + 1, :cache_len, 1]
    return bufs[0][:maxB, :, :cache_len].permute(0, 2, 1, 3), bufs[1][:maxB, :, :cache_len].permute(0, 2, 1, 3)


FP8_SCALE_MODES = ("ones", "mixed", "none")


def fp8_scales(mode, Hkv):
    """(k_scale, v_scale) fp32 [Hkv] or None.  mixed: arbitrary (not powers of two: the division rounds) values with one >= 4
    and one <= 2^-6 among every head count's K and V scales; 448 * 0.013 = 5.8 < 15.75: K saturates."""
    if mode == "none":
        return None, None
    if mode == "ones":
        return torch.ones(Hkv), torch.ones(Hkv)
    ks = torch.tensor([0.013, 4.5, 0.37, 1.7])[torch.arange(Hkv) % 4]
    vs = torch.tensor([5.25, 0.011, 2.3, 0.6])[torch.arange(Hkv) % 4]
    return ks.contiguous(), vs.contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# add + RMSNorm and SwiGLU in float64
# ------------------------------------------------------------------------------------------------------------------------
def add_rmsnorm_ref64(x, residual, weight, eps):
    """The header's definition: sum = residual + x rounded to the dtype (x itself without a residual), norm = sum *
    rsqrt(mean(sum^2) + eps) * weight in float64 (unrounded).  x / residual [rows, n], weight [n] host tensors of the dtype.
    The float64 sum of two 16-bit values is exact for every pair whose exponents differ by less than 40, and torch's rounding
    of it through fp32 is innocuous: fp32 has more than 2p + 2 bits for p = 8 and p = 11.  eps is the fp32 value the ABI takes."""
    if residual is None:
        s = x
    else:
        s = (x.double() + residual.double()).to(x.dtype)
    h = s.double()
    e = float(np.float32(eps))
    return s, h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + e) * weight.double()


def swiglu_ref64(gate, up):
    """gate / (1 + exp(-gate)) * up in float64 (unrounded): NaN for NaN and -inf gates, +-inf for +inf gates."""
    g = gate.double()
    return g / (1.0 + torch.exp(-g)) * up.double()


def all_bit_patterns(dtype):
    """Every one of the 65536 values of a 16-bit dtype, as one row [1, 65536]."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(dtype).reshape(1, 65536)
