// Fused decode-step preamble of the attention block ("next" row 1 of SURVEY 8f): one kernel that
//   * applies rotary position embedding to this step's q and k at ABSOLUTE positions
//     (/root/reference/hydragen/llama.py:485-501, HF rotate-half convention),
//   * appends the rotated k and the v at index (position - shared length) of the unique KV caches
//     (llama.py:236-262, two scatter_ kernels in the reference; index rule llama.py:487-492),
//   * emits seq_lens[b] = index + 1 as int32 for the suffix kernel (llama.py:569, flash.py:220),
// replacing ~10 small torch kernels per layer per token.  HBM-bound and tiny: B*(Hq+2*Hkv)*D elements.
//
// ONE row body, rope_append_row<T, D, MULTI, NORM, FP8>, for rows of D = 64 / 128 / 256 elements; eight of the nine __global__ names
// below are its instantiations (every combination of the three switches).  The ninth, "narrow" (hyd_rope_params.head_dim = d < D, d % 16 == 0; 16-bit caches), keeps its own
// preamble behind them and shares rotated_row: q / k / v arrive from the GEMM as rows of d elements with head stride d, the rotate-half pairs are
// (i, i + d / 2) -- 8-element vectors, hence d % 16 == 0 --, K (rotated) and V go into the caches as rows of d elements at the caches'
// strides, and q_out keeps the attention kernels' pitch of D with exact zeros in its pad columns.  The body's switches:
//   MULTI  (hyd_rope_append_multi): q / k / v are [B, T, H, D], the row's position is that of its FIRST token and token i is
//          rotated at position + i and appended at cache index idx0 + i, idx0 = position - shared length.  K/V rows of drafts that
//          the step rejects stay in the cache behind the row's next length: nothing reads them (every kernel stops at seq_len),
//          and the next step, which starts behind the last accepted token and writes T rows again, overwrites them.
//   NORM   (hyd_qk_norm; Qwen3's self_attn.q_norm / k_norm): for a q row and a k row, in front of the rotation,
//            r = rsqrt(mean_d(x_d^2) + eps),  n_d = x_d * r * w_d,
//          in fp32 on the widened 16-bit GEMM output with ONE rounding to the 16-bit dtype behind the rotation (the RMSNorm
//          convention of layer_ops.hip: multiply in fp32, round once).  v rows are copied as they are.
//   FP8    (hyd_kv_quant): the rotated k -- the 16-bit value a 16-bit cache would hold -- and v are stored as quantize_kv(x, scale)
//          (hydragen_amd/kv_quant.py); the caches' strides are in bytes and a null scale pointer means 1.
#include <type_traits>

#include "hyd_kernels.h"

namespace hyd {

template <typename T>
__device__ __forceinline__ void widen8x(const u32x4& v, float (&f)[8]) {
    using TR = Traits<T>;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = TR::lo(v[i]);
        f[2 * i + 1] = TR::hi(v[i]);
    }
}

// NORM's sum of squares: a thread holds 16 of its row's D elements, so it is 16 terms per lane and a butterfly over the row's
// TPR = D / 16 adjacent lanes -- DPP moves inside one 16-lane row of the wave, no LDS --, after which every lane of the row holds the
// same bits.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true);
    return v + __builtin_bit_cast(float, o);
}
// every stage adds the value of the lane's mirror image inside 2 / 4 / 8 / 16 lanes; the earlier stages made each half uniform, so
// the mirror lane holds what lane ^ 4 (^ 8) holds and both partners form the same sum a + b
template <int TPR>
__device__ __forceinline__ float row_sum(float v) {
    static_assert(TPR == 4 || TPR == 8 || TPR == 16, "a row is 4, 8 or 16 adjacent lanes");
    v = dpp_add<0xB1>(v);                  // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);                  // quad_perm [2, 3, 0, 1]
    if (TPR >= 8) v = dpp_add<0x141>(v);   // row_half_mirror
    if (TPR >= 16) v = dpp_add<0x140>(v);  // row_mirror
    return v;
}

// The thread's 8 + 8 elements of a rotated q or k row: loaded at src + d0 and src + half + d0, widened, normalised with the gains w
// when NORM (rows of DC elements; DC is not read otherwise), rotated by the table rows cr / sr, rounded once.  Every kernel of the file
// rotates here.
template <typename T, int DC, bool NORM>
__device__ __forceinline__ void rotated_row(const uint16_t* src, const uint16_t* w, float eps, const float* cr, const float* sr, int d0, int half,
                                            u32x4& olo, u32x4& ohi) {
    using TR = Traits<T>;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(src + d0);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(src + half + d0);
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr + d0), c1 = *reinterpret_cast<const f32x4*>(cr + d0 + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr + d0), s1 = *reinterpret_cast<const f32x4*>(sr + d0 + 4);
    float x[8], y[8];
    widen8x<T>(lo, x);
    widen8x<T>(hi, y);
    if constexpr (NORM) {
        float gx[8], gy[8];
        widen8x<T>(*reinterpret_cast<const u32x4*>(w + d0), gx);
        widen8x<T>(*reinterpret_cast<const u32x4*>(w + half + d0), gy);
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) ss += x[i] * x[i] + y[i] * y[i];
        ss = row_sum<DC / 16>(ss);
        const float r = __builtin_amdgcn_rsqf(ss * (1.0f / DC) + eps);  // v_rsq_f32: 1 ulp
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            x[i] = x[i] * r * gx[i];
            y[i] = y[i] * r * gy[i];
        }
    }
    // x c - y s and y c + x s: one product is rounded and the FMA takes the other.  Which one is written out here, because the
    // compiler chose for itself while the loop had two spellings and chose differently: behind the norm x s is the rounded one,
    // without it y c.  tests/golden/rope_append_parent.npz holds those bits, so a row keeps them whatever a later compiler prefers.
    const auto first = [](float xv, float yv, float c, float s) { return __builtin_fmaf(xv, c, -(yv * s)); };
    const auto second = [](float xv, float yv, float c, float s) { return NORM ? __builtin_fmaf(yv, c, xv * s) : __builtin_fmaf(xv, s, yv * c); };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float ca = i < 2 ? c0[2 * i] : c1[2 * i - 4], cb = i < 2 ? c0[2 * i + 1] : c1[2 * i - 3];
        const float sa = i < 2 ? s0[2 * i] : s1[2 * i - 4], sb = i < 2 ? s0[2 * i + 1] : s1[2 * i - 3];
        olo[i] = TR::pack2(first(x[2 * i], y[2 * i], ca, sa), first(x[2 * i + 1], y[2 * i + 1], cb, sb));
        ohi[i] = TR::pack2(second(x[2 * i], y[2 * i], ca, sa), second(x[2 * i + 1], y[2 * i + 1], cb, sb));
    }
}

// quantize_kv: a correctly rounded x / scale, clamped to +-448 (NaN passes through the comparisons), then v_cvt_pk_fp8_f32
// (round-half-even; the clamp keeps it away from the overflow encoding), 8 bytes per store.
__device__ __forceinline__ float fp8_prescale(float x, float s) {
    const float y = x / s;
    return y > 448.f ? 448.f : (y < -448.f ? -448.f : y);
}
template <typename T>
__device__ __forceinline__ u32x2 quant_fp8x8(const u32x4& v, float s) {
    float x[8];
    widen8x<T>(v, x);
    u32x2 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(x[4 * i], s), fp8_prescale(x[4 * i + 1], s), 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(x[4 * i + 2], s), fp8_prescale(x[4 * i + 3], s), w, true);
        r[i] = (uint32_t)w;
    }
    return r;
}

// D / 16 threads per row: each owns 8 elements of the row's first half and the matching 8 of the second.
template <typename T, int D, bool MULTI, bool NORM, bool FP8>
__device__ __forceinline__ void rope_append_row(const RopeArgs& a) {
    using Cache = typename std::conditional<FP8, uint8_t, uint16_t>::type;  // the caches' strides count these
    constexpr int tpr = D / 16, half = D / 2;
    const int T_ = MULTI ? a.T : 1;
    const int rows_per_t = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / tpr;
    const int sub = (int)(gid % tpr);
    if (row >= (int64_t)a.B * T_ * rows_per_t) return;
    const int h = (int)(row % rows_per_t);
    const int64_t bt = row / rows_per_t;  // batch row and token
    const int b = MULTI ? (int)(bt / a.T) : (int)bt, i = MULTI ? (int)(bt % a.T) : 0;
    const int64_t pos0 = a.pos[(int64_t)b * a.pos_stride];
    const int64_t idx0 = pos0 - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t idx = idx0 + i, pos_raw = pos0 + i;
    // never read past the rotary tables (the host checks the range before launching; a kernel cannot raise)
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    // one token: index + 1, also where that is <= 0.  Several: a retired row (position shared_len - 1) reports 0
    if (h == 0 && sub == 0 && i == 0) a.seq_lens[b] = MULTI ? (idx0 >= 0 ? (int32_t)(idx0 + a.T) : 0) : (int32_t)(idx0 + 1);
    // never write out of the allocated cache, and never for a retired row: idx0 + i >= 0 for its later tokens must not write
    const bool store_kv = idx0 >= 0 && idx < a.cache_len;
    const int d0 = sub * 8;
    u32x4 olo, ohi;  // what the thread stores: its elements of the rotated q or k row, or of the v row
    Cache* dst;
    float s = 1.0f;
    if (h < a.Hq + a.Hkv) {
        // The lanes of a row enter NORM's butterfly together: the bounds exit and the q / k / v branch are decided per row, and
        // every cache guard sits behind it.  A ragged last wave ends on a row boundary (256 % TPR == 0), so no live lane reads
        // one that has left.
        const bool isq = h < a.Hq;
        const int hk = h - a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_bs + (int64_t)i * a.q_ts + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)i * a.k_ts + (int64_t)hk * D;
        rotated_row<T, D, NORM>(src, static_cast<const uint16_t*>(isq ? a.q_weight : a.k_weight), a.eps, a.cos + pos * a.cs_stride,
                                 a.sin + pos * a.cs_stride, d0, half, olo, ohi);
        if (isq) {  // q is always written
            uint16_t* qo = static_cast<uint16_t*>(a.q_out) + (bt * a.Hq + h) * D;
            *reinterpret_cast<u32x4*>(qo + d0) = olo;
            *reinterpret_cast<u32x4*>(qo + half + d0) = ohi;
            return;
        }
        if (!store_kv) return;
        if (FP8) s = a.k_scale ? a.k_scale[hk] : 1.0f;
        dst = static_cast<Cache*>(a.k_cache) + (int64_t)b * a.kc_bs + idx * a.kc_ts + (int64_t)hk * a.kc_hs;
    } else {
        if (!store_kv) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)i * a.v_ts + (int64_t)hv * D;
        olo = *reinterpret_cast<const u32x4*>(src + d0);
        ohi = *reinterpret_cast<const u32x4*>(src + half + d0);
        if (FP8) s = a.v_scale ? a.v_scale[hv] : 1.0f;
        dst = static_cast<Cache*>(a.v_cache) + (int64_t)b * a.vc_bs + idx * a.vc_ts + (int64_t)hv * a.vc_hs;
    }
    if constexpr (FP8) {
        *reinterpret_cast<u32x2*>(dst + d0) = quant_fp8x8<T>(olo, s);
        *reinterpret_cast<u32x2*>(dst + half + d0) = quant_fp8x8<T>(ohi, s);
    } else {
        *reinterpret_cast<u32x4*>(dst + d0) = olo;
        *reinterpret_cast<u32x4*>(dst + half + d0) = ohi;
    }
}

// the kernels of the row body: rope_append_row<T, D, MULTI, NORM, FP8>
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_kernel(const RopeArgs a) { rope_append_row<T, D, false, false, false>(a); }
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_fp8_kernel(const RopeArgs a) { rope_append_row<T, D, false, false, true>(a); }
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_multi_kernel(const RopeArgs a) { rope_append_row<T, D, true, false, false>(a); }
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_norm_kernel(const RopeArgs a) { rope_append_row<T, D, false, true, false>(a); }
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_norm_fp8_kernel(const RopeArgs a) { rope_append_row<T, D, false, true, true>(a); }
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_norm_multi_kernel(const RopeArgs a) { rope_append_row<T, D, true, true, false>(a); }
// ... and fp8 caches under several tokens (hyd_rope_append_multi_kvq): token i is quantized with its kv head's scale and written at idx0 + i
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_multi_fp8_kernel(const RopeArgs a) { rope_append_row<T, D, true, false, true>(a); }
template <typename T, int D> __global__ __launch_bounds__(256) void rope_append_norm_multi_fp8_kernel(const RopeArgs a) { rope_append_row<T, D, true, true, true>(a); }

// Narrow head dims keep a preamble of their own.  As an instantiation of rope_append_row with a runtime row width the kernel measured
// +0.17 us on 7.4 us per layer against a parent spread of 0.07 us (profiles/rope_append_body.md, "First attempt"), so the thread
// decoding, the clamp, the seq_lens rule and the guards below are the earlier kernel's text on RopeArgs -- the one-token rules of
// rope_append_row, to be changed together with it --, while the loads, the table rows and the rotation are rotated_row's.  D / 16
// threads per row as above: the first d / 16 work on the narrow row, the others write the D - d pad columns of a q row (two vectors
// each) and have nothing to do for k / v.
template <typename T>
__global__ __launch_bounds__(256) void rope_append_narrow_kernel(const RopeArgs a) {
    const int D = a.D, d = a.d;
    const int tpr = D / 16, act = d / 16;
    const int rows_per_b = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / tpr;
    const int sub = (int)(gid % tpr);
    if (row >= (int64_t)a.B * rows_per_b) return;
    const int b = (int)(row / rows_per_b);
    const int h = (int)(row % rows_per_b);
    const int64_t pos_raw = a.pos[(int64_t)b * a.pos_stride];
    const int64_t idx = pos_raw - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0) a.seq_lens[b] = (int32_t)(idx + 1);
    if (sub >= act) {
        if (h < a.Hq) {  // q_out's pad columns: 16 of them per thread
            uint16_t* dst = static_cast<uint16_t*>(a.q_out) + ((int64_t)b * a.Hq + h) * D + d + (sub - act) * 16;
            const u32x4 z = {0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(dst) = z;
            *reinterpret_cast<u32x4*>(dst + 8) = z;
        }
        return;
    }
    const int d0 = sub * 8, half = d / 2;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_bs + (int64_t)h * d
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)(h - a.Hq) * d;
        u32x4 olo, ohi;
        rotated_row<T, 0, false>(src, nullptr, 0.f, a.cos + pos * a.cs_stride, a.sin + pos * a.cs_stride, d0, half, olo, ohi);
        uint16_t* dst;
        if (isq) {
            dst = static_cast<uint16_t*>(a.q_out) + ((int64_t)b * a.Hq + h) * D;
        } else {
            if (idx < 0 || idx >= a.cache_len) return;  // out of the allocated cache: never write out of bounds
            dst = static_cast<uint16_t*>(a.k_cache) + (int64_t)b * a.kc_bs + idx * a.kc_ts + (int64_t)(h - a.Hq) * a.kc_hs;
        }
        *reinterpret_cast<u32x4*>(dst + d0) = olo;
        *reinterpret_cast<u32x4*>(dst + half + d0) = ohi;
    } else {
        if (idx < 0 || idx >= a.cache_len) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hv * d;
        uint16_t* dst = static_cast<uint16_t*>(a.v_cache) + (int64_t)b * a.vc_bs + idx * a.vc_ts + (int64_t)hv * a.vc_hs;
        *reinterpret_cast<u32x4*>(dst + d0) = *reinterpret_cast<const u32x4*>(src + d0);
        *reinterpret_cast<u32x4*>(dst + half + d0) = *reinterpret_cast<const u32x4*>(src + half + d0);
    }
}

using RopeKernel = void (*)(const RopeArgs);

// the kernel of a.D-element rows for the call's features
template <typename T, int D>
static RopeKernel rope_kernel_of(const RopeArgs& a) {
    const bool norm = a.q_weight != nullptr, multi = a.T > 1;
    if (a.fp8 && multi) return norm ? rope_append_norm_multi_fp8_kernel<T, D> : rope_append_multi_fp8_kernel<T, D>;
    if (a.fp8) return norm ? rope_append_norm_fp8_kernel<T, D> : rope_append_fp8_kernel<T, D>;
    if (multi) return norm ? rope_append_norm_multi_kernel<T, D> : rope_append_multi_kernel<T, D>;
    return norm ? rope_append_norm_kernel<T, D> : rope_append_kernel<T, D>;
}

template <typename T>
static RopeKernel rope_kernel_of(const RopeArgs& a) {
    if (a.d != a.D) {  // narrow rows: 16-bit caches, one token, no norm
        const bool ok = a.D % 16 == 0 && a.d % 16 == 0 && a.d >= 16 && a.d < a.D && !a.fp8 && !a.q_weight && a.T == 1;
        return ok ? rope_append_narrow_kernel<T> : nullptr;
    }
    return a.D == 128 ? rope_kernel_of<T, 128>(a) : a.D == 64 ? rope_kernel_of<T, 64>(a) : a.D == 256 ? rope_kernel_of<T, 256>(a) : nullptr;
}

int launch_rope_append(const RopeArgs& a, int dtype, hipStream_t s) {
    const int64_t threads = (int64_t)a.B * a.T * (a.Hq + 2 * a.Hkv) * (a.D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;  // (an empty call succeeds whatever else it asks for, as it always has at D = 64 / 128 / 256)
    const RopeKernel kernel = dtype == HYD_F16 ? rope_kernel_of<F16>(a) : rope_kernel_of<BF16>(a);
    if (!kernel) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
