"""float64 definition, test data and the derived error bound of the per-head q/k RMSNorm inside the RoPE + append kernels
(rope_append.hip: hyd_rope_append_decode_qkn, hyd_rope_append_multi_qkn).  CPU only; tests/test_qk_norm.py holds these helpers to
their own claims, tests/test_qk_norm_gpu.py holds the kernels to them.

The rule of tests/glue_ref.py applies: nothing here is measured on a kernel.  Every bound is the precision of a number format,
the accuracy an instruction documents, or a stated argument."""
import numpy as np
import torch

from tests.glue_ref import rope_ref64, ulp16

U = 2.0 ** -24  # unit roundoff of fp32 (round to nearest): every fp32 product, sum and FMA is within U relative of its exact value


def qk_norm_ref64(x, w, eps):
    """n = x * rsqrt(mean_d(x_d^2) + eps) * w in float64 (unrounded).  x [..., D] and w [D] float64 arrays holding the 16-bit
    input values, eps the fp32 value the ABI takes."""
    e = float(np.float32(eps))
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + e) * w


def qk_norm_rope_ref64(x, w, eps, cos_rows, sin_rows):
    """(want, n): the definition of the header -- the norm above, then the rotate-half rotation of glue_ref.rope_ref64 with one
    fp32 table row per b -- in float64, and the normalised row n the bound needs.  x [B, H, D], w [D], cos_rows / sin_rows [B, D]."""
    n = qk_norm_ref64(x, w, eps)
    return rope_ref64(n, cos_rows, sin_rows), n


def norm_rel_err(D):
    """Relative error of the kernel's fp32 n_d against the exact one, from its fp32 steps:
      * sum of D squares, any order: each square within U, each of the at most D - 1 additions of positive terms within U, so the
        sum is within gamma_D = D U / (1 - D U) of the exact one whichever way it is bracketed (lane-local terms first, then a
        butterfly) and whether or not a product is contracted into an FMA (that only removes a rounding);
      * mean + eps: the division by D is a power of two, exact; the addition (or the FMA that does both) adds U;
      * the reciprocal square root halves a relative error of its argument (|d/dm m^-1/2| m / m^-1/2 = 1/2) and adds its own:
        v_rsq_f32 is documented to 1 ulp, and an ulp is at most 2 U relative to the value;
      * x * r and (x r) * w: two products, U each.
    Squares of inputs so small that they are subnormal in fp32 (|x| < 2^-63) may lose everything: against eps >= 1e-6 that is
    an absolute error below 2^-126 D / eps of the argument, far below U.  The factor 1.01 covers the second-order terms."""
    gamma = D * U / (1 - D * U)
    return 1.01 * ((gamma + U) / 2 + 2 * U + 2 * U)


def qk_norm_rope_bound(want, n, dtype):
    """|got - want| <= 1/2 ulp16(want) + c (|n_x| + |n_y|), n_x and n_y the two exact normalised inputs of the element's pair.
    First term: the ONE round-to-nearest to the 16-bit dtype.  c, as in glue_ref.rope_bound: before that rounding the fp32 value
    is off by the error of the two normalised inputs, norm_rel_err(D) (|n_x| + |n_y|) at most since |cos|, |sin| <= 1, plus the
    rotation's own two products and sum, 2 U (|n_x| + |n_y|) (1 + norm_rel_err) -- contracted into an FMA or not --; the sum is
    doubled for the case where that error moves the value across a rounding boundary into a binade with twice the spacing."""
    D = n.shape[-1]
    half = D // 2
    c = qk_norm_c(D)
    a = np.abs(n[..., :half]) + np.abs(n[..., half:])
    return 0.5 * ulp16(want, dtype) + c * np.concatenate([a, a], -1)


def qk_norm_c(D):
    e = norm_rel_err(D)
    return 2 * (e + 2 * U * (1 + e))


# ------------------------------------------------------------------------------------------------------------------------
# Test data: heads of very different size, the rows that break a careless kernel
# ------------------------------------------------------------------------------------------------------------------------
def head_scale(h):
    """Head h is scaled by 2^(h - 3): a sum of squares that crosses a head boundary is off by a factor of 4 or more."""
    return 2.0 ** (h - 3)


def make_inputs(dtype, B, Hq, Hkv, D, seed=0):
    """q [B, Hq, D], k / v [B, Hkv, D] host tensors of `dtype` and the 16-bit gains (q_w, k_w [D]):
      * head h of q and of k is scaled by 2^(h - 3);
      * the last q head of row 0 and the last k head of the last row are all zero (exact zeros out, no NaN);
      * q head 0 of the last row has a single non-zero element;
      * for f16, q head 1 (or 0 with one head) of row B // 2 holds values near 6e4: a square taken in f16 overflows;
      * the gains are 1 + 0.3 normal with zero and negative entries planted; q and k gains differ."""
    rng = np.random.default_rng(1234 + seed + D)
    q = rng.standard_normal((B, Hq, D)) * np.array([head_scale(h) for h in range(Hq)])[None, :, None]
    k = rng.standard_normal((B, Hkv, D)) * np.array([head_scale(h) for h in range(Hkv)])[None, :, None]
    v = rng.standard_normal((B, Hkv, D))
    q[0, Hq - 1] = 0.0
    k[B - 1, Hkv - 1] = 0.0
    q[B - 1, 0] = 0.0
    q[B - 1, 0, D // 2 + 3] = -1.75
    if dtype == torch.float16:
        q[B // 2, min(1, Hq - 1)] = rng.uniform(5.5e4, 6.5e4, D) * rng.choice([-1.0, 1.0], D)
    qw, kw = 1 + 0.3 * rng.standard_normal(D), 1 + 0.3 * rng.standard_normal(D)
    qw[[1, D // 2]] = 0.0
    qw[[2, D - 1]] *= -1
    kw[[0, D // 2 + 1]] = 0.0
    kw[[5, D // 2 - 1]] = -np.abs(kw[[5, D // 2 - 1]])
    t = lambda a: torch.from_numpy(a).to(dtype)
    return t(q), t(k), t(v), t(qw), t(kw)


def rotary_tables(D, max_pos, base=10000.0):
    """fp32 cos / sin [max_pos, D] as hydragen_amd.llama.RotaryTable builds them (host)."""
    inv_freq = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    freqs = torch.outer(torch.arange(max_pos, dtype=torch.float32), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos(), emb.sin()


def f64(t):
    return t.double().numpy()
