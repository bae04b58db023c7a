// Fused decode-step preamble of the attention block ("next" row 1 of SURVEY 8f): one kernel that
//   * applies rotary position embedding to this step's q and k at ABSOLUTE positions
//     (/root/reference/hydragen/llama.py:485-501, HF rotate-half convention),
//   * appends the rotated k and the v at index (position - shared length) of the unique KV caches
//     (llama.py:236-262, two scatter_ kernels in the reference; index rule llama.py:487-492),
//   * emits seq_lens[b] = index + 1 as int32 for the suffix kernel (llama.py:569, flash.py:220),
// replacing ~10 small torch kernels per layer per token.  HBM-bound and tiny: B*(Hq+2*Hkv)*D elements.
#include "hyd_kernels.h"

namespace hyd {

template <typename T>
__device__ __forceinline__ void rope8(const u32x4& lo, const u32x4& hi, const float* c, const float* s, u32x4& olo,
                                      u32x4& ohi) {
    using TR = Traits<T>;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x0 = TR::lo(lo[i]), x1 = TR::hi(lo[i]);
        const float y0 = TR::lo(hi[i]), y1 = TR::hi(hi[i]);
        const float c0 = c[2 * i], c1 = c[2 * i + 1], s0 = s[2 * i], s1 = s[2 * i + 1];
        olo[i] = TR::pack2(x0 * c0 - y0 * s0, x1 * c1 - y1 * s1);
        ohi[i] = TR::pack2(y0 * c0 + x0 * s0, y1 * c1 + x1 * s1);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void rope_append_kernel(const RopeArgs a) {
    constexpr int TPR = D / 16;  // threads per row: each owns 8 dims of the first half + the matching 8 of the second
    const int rows_per_b = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / TPR;
    const int sub = (int)(gid % TPR);
    if (row >= (int64_t)a.B * rows_per_b) return;
    const int b = (int)(row / rows_per_b);
    const int h = (int)(row % rows_per_b);
    const int64_t pos_raw = a.pos[(int64_t)b * a.pos_stride];
    const int64_t idx = pos_raw - (a.shared_len ? a.shared_len[b] : 0);
    // never read past the rotary tables (the host checks the range before launching; a kernel cannot raise)
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0) a.seq_lens[b] = (int32_t)(idx + 1);
    const int d0 = sub * 8;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_bs + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)(h - a.Hq) * D;
        const u32x4 lo = *reinterpret_cast<const u32x4*>(src + d0);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
        float c[8], s[8];
        const float* cr = a.cos + pos * a.cs_stride + d0;
        const float* sr = a.sin + pos * a.cs_stride + d0;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr), c1 = *reinterpret_cast<const f32x4*>(cr + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = c0[i];
            c[4 + i] = c1[i];
            s[i] = s0[i];
            s[4 + i] = s1[i];
        }
        u32x4 olo, ohi;
        rope8<T>(lo, hi, c, s, olo, ohi);
        uint16_t* dst;
        if (isq) {
            dst = static_cast<uint16_t*>(a.q_out) + ((int64_t)b * a.Hq + h) * D;
        } else {
            if (idx < 0 || idx >= a.cache_len) return;  // out of the allocated cache: never write out of bounds
            dst = static_cast<uint16_t*>(a.k_cache) + (int64_t)b * a.kc_bs + idx * a.kc_ts + (int64_t)(h - a.Hq) * a.kc_hs;
        }
        *reinterpret_cast<u32x4*>(dst + d0) = olo;
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = ohi;
    } else {
        if (idx < 0 || idx >= a.cache_len) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hv * D;
        uint16_t* dst = static_cast<uint16_t*>(a.v_cache) + (int64_t)b * a.vc_bs + idx * a.vc_ts + (int64_t)hv * a.vc_hs;
        *reinterpret_cast<u32x4*>(dst + d0) = *reinterpret_cast<const u32x4*>(src + d0);
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
    }
}

// Narrow head dims (hyd_rope_params.head_dim = d < D, d % 16 == 0; 16-bit caches): q / k / v arrive from the GEMM as rows of d
// elements with head stride d, the rotate-half pairs are (i, i + d / 2) -- 8-element vectors, hence d % 16 == 0 --, K (rotated)
// and V go into the caches as rows of d elements at the caches' strides, and q_out keeps the attention kernels' pitch of D with
// exact zeros in its pad columns.  D / 16 threads per row as in the kernel above: the first d / 16 do its work on the narrow
// row, the others write the D - d pad columns of a q row (two vectors each) and have nothing to do for k / v.
template <typename T>
__global__ __launch_bounds__(256) void rope_append_narrow_kernel(const RopeNarrowArgs na) {
    const RopeArgs& a = na.a;
    const int D = na.D, d = na.d;
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
        const u32x4 lo = *reinterpret_cast<const u32x4*>(src + d0);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(src + half + d0);
        float c[8], s[8];
        const float* cr = a.cos + pos * a.cs_stride + d0;
        const float* sr = a.sin + pos * a.cs_stride + d0;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr), c1 = *reinterpret_cast<const f32x4*>(cr + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = c0[i];
            c[4 + i] = c1[i];
            s[i] = s0[i];
            s[4 + i] = s1[i];
        }
        u32x4 olo, ohi;
        rope8<T>(lo, hi, c, s, olo, ohi);
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

int launch_rope_append_narrow(const RopeNarrowArgs& na, int dtype, hipStream_t s) {
    const RopeArgs& a = na.a;
    if (na.D % 16 != 0 || na.d % 16 != 0 || na.d < 16 || na.d >= na.D) return (int)hipErrorInvalidValue;
    const int64_t threads = (int64_t)a.B * (a.Hq + 2 * a.Hkv) * (na.D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;
    if (dtype == HYD_F16) hipLaunchKernelGGL((rope_append_narrow_kernel<F16>), dim3(grid), dim3(256), 0, s, na);
    else hipLaunchKernelGGL((rope_append_narrow_kernel<BF16>), dim3(grid), dim3(256), 0, s, na);
    return (int)hipGetLastError();
}

// fp8 caches (hyd_kv_quant): the same kernel, but the rotated k -- the 16-bit value the kernel above writes -- and v are stored as
// quantize_kv(x, scale) (hydragen_amd/kv_quant.py): a correctly rounded x / scale[h], clamped to +-448 (NaN passes through the
// comparisons), then v_cvt_pk_fp8_f32 (round-half-even; the clamp keeps it away from the overflow encoding), 8 bytes per store.
__device__ __forceinline__ float fp8_prescale(float x, float s) {
    const float y = x / s;
    return y > 448.f ? 448.f : (y < -448.f ? -448.f : y);
}
__device__ __forceinline__ u32x2 quant_fp8x8(const float (&x)[8], float s) {
    u32x2 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(x[4 * i], s), fp8_prescale(x[4 * i + 1], s), 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_prescale(x[4 * i + 2], s), fp8_prescale(x[4 * i + 3], s), w, true);
        r[i] = (uint32_t)w;
    }
    return r;
}
template <typename T>
__device__ __forceinline__ void widen8x(const u32x4& v, float (&f)[8]) {
    using TR = Traits<T>;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = TR::lo(v[i]);
        f[2 * i + 1] = TR::hi(v[i]);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void rope_append_fp8_kernel(const RopeKvqArgs ka) {
    const RopeArgs& a = ka.a;
    constexpr int TPR = D / 16;
    const int rows_per_b = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / TPR;
    const int sub = (int)(gid % TPR);
    if (row >= (int64_t)a.B * rows_per_b) return;
    const int b = (int)(row / rows_per_b);
    const int h = (int)(row % rows_per_b);
    const int64_t pos_raw = a.pos[(int64_t)b * a.pos_stride];
    const int64_t idx = pos_raw - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0) a.seq_lens[b] = (int32_t)(idx + 1);
    const int d0 = sub * 8;
    u32x4 olo, ohi;
    float s;
    uint8_t* dst8;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_bs + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)(h - a.Hq) * D;
        const u32x4 lo = *reinterpret_cast<const u32x4*>(src + d0);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
        float c[8], sn[8];
        const float* cr = a.cos + pos * a.cs_stride + d0;
        const float* sr = a.sin + pos * a.cs_stride + d0;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr), c1 = *reinterpret_cast<const f32x4*>(cr + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = c0[i];
            c[4 + i] = c1[i];
            sn[i] = s0[i];
            sn[4 + i] = s1[i];
        }
        rope8<T>(lo, hi, c, sn, olo, ohi);
        if (isq) {
            uint16_t* dst = static_cast<uint16_t*>(a.q_out) + ((int64_t)b * a.Hq + h) * D;
            *reinterpret_cast<u32x4*>(dst + d0) = olo;
            *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = ohi;
            return;
        }
        if (idx < 0 || idx >= a.cache_len) return;  // out of the allocated cache: never write out of bounds
        const int hk = h - a.Hq;
        s = ka.k_scale ? ka.k_scale[hk] : 1.0f;
        dst8 = static_cast<uint8_t*>(a.k_cache) + (int64_t)b * a.kc_bs + idx * a.kc_ts + (int64_t)hk * a.kc_hs;
    } else {
        if (idx < 0 || idx >= a.cache_len) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hv * D;
        olo = *reinterpret_cast<const u32x4*>(src + d0);
        ohi = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
        s = ka.v_scale ? ka.v_scale[hv] : 1.0f;
        dst8 = static_cast<uint8_t*>(a.v_cache) + (int64_t)b * a.vc_bs + idx * a.vc_ts + (int64_t)hv * a.vc_hs;
    }
    float xl[8], xh[8];
    widen8x<T>(olo, xl);
    widen8x<T>(ohi, xh);
    *reinterpret_cast<u32x2*>(dst8 + d0) = quant_fp8x8(xl, s);
    *reinterpret_cast<u32x2*>(dst8 + D / 2 + d0) = quant_fp8x8(xh, s);
}

int launch_rope_append_fp8(const RopeKvqArgs& ka, int dtype, int D, hipStream_t s) {
    const RopeArgs& a = ka.a;
    const int64_t threads = (int64_t)a.B * (a.Hq + 2 * a.Hkv) * (D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;
#define HYD_ROPE(TT, DD) hipLaunchKernelGGL((rope_append_fp8_kernel<TT, DD>), dim3(grid), dim3(256), 0, s, ka)
    if (dtype == HYD_F16) {
        if (D == 128) HYD_ROPE(F16, 128);
        else if (D == 64) HYD_ROPE(F16, 64);
        else if (D == 256) HYD_ROPE(F16, 256);
        else return (int)hipErrorInvalidValue;
    } else {
        if (D == 128) HYD_ROPE(BF16, 128);
        else if (D == 64) HYD_ROPE(BF16, 64);
        else if (D == 256) HYD_ROPE(BF16, 256);
        else return (int)hipErrorInvalidValue;
    }
#undef HYD_ROPE
    return (int)hipGetLastError();
}

// Multi-token decode step (hyd_rope_append_multi): q / k / v are [B, T, H, D], the row's position is that of its FIRST token and
// token i is rotated at position + i and appended at cache index idx + i, idx = position - shared length; seq_lens[b] = idx + T.
// The thread layout of rope_append_kernel with the token as one more row index.  A row with idx < 0 (position shared_len - 1: a
// retired row) takes no part at all -- idx + i >= 0 for its later tokens must not write --, so the guard is on idx, then on the
// token's own index against cache_len.  K/V rows of drafts that the step rejects stay in the cache behind the row's next length:
// nothing reads them (every kernel stops at seq_len), and the next step, which starts behind the last accepted token and writes T
// rows again, overwrites them.
template <typename T, int D>
__global__ __launch_bounds__(256) void rope_append_multi_kernel(const hyd_rope_multi_params a) {
    constexpr int TPR = D / 16;
    const int rows_per_t = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / TPR;
    const int sub = (int)(gid % TPR);
    if (row >= (int64_t)a.B * a.T * rows_per_t) return;
    const int h = (int)(row % rows_per_t);
    const int64_t bt = row / rows_per_t;
    const int b = (int)(bt / a.T), i = (int)(bt % a.T);
    const int64_t pos0 = a.position_ids[(int64_t)b * a.pos_stride];
    const int64_t idx0 = pos0 - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t idx = idx0 + i, pos_raw = pos0 + i;
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0 && i == 0) a.seq_lens[b] = idx0 >= 0 ? (int32_t)(idx0 + a.T) : 0;
    const bool store_kv = idx0 >= 0 && idx < a.cache_len;  // never write out of bounds, never for a retired row
    const int d0 = sub * 8;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        if (!isq && !store_kv) return;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_batch_stride + (int64_t)i * a.q_tok_stride + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_batch_stride + (int64_t)i * a.k_tok_stride + (int64_t)(h - a.Hq) * D;
        const u32x4 lo = *reinterpret_cast<const u32x4*>(src + d0);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
        float c[8], s[8];
        const float* cr = a.cos + pos * a.cs_stride + d0;
        const float* sr = a.sin + pos * a.cs_stride + d0;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr), c1 = *reinterpret_cast<const f32x4*>(cr + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = c0[j];
            c[4 + j] = c1[j];
            s[j] = s0[j];
            s[4 + j] = s1[j];
        }
        u32x4 olo, ohi;
        rope8<T>(lo, hi, c, s, olo, ohi);
        uint16_t* dst = isq ? static_cast<uint16_t*>(a.q_out) + (bt * a.Hq + h) * D
                            : static_cast<uint16_t*>(a.k_cache) + (int64_t)b * a.kc_batch_stride + idx * a.kc_tok_stride + (int64_t)(h - a.Hq) * a.kc_head_stride;
        *reinterpret_cast<u32x4*>(dst + d0) = olo;
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = ohi;
    } else {
        if (!store_kv) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_batch_stride + (int64_t)i * a.v_tok_stride + (int64_t)hv * D;
        uint16_t* dst = static_cast<uint16_t*>(a.v_cache) + (int64_t)b * a.vc_batch_stride + idx * a.vc_tok_stride + (int64_t)hv * a.vc_head_stride;
        *reinterpret_cast<u32x4*>(dst + d0) = *reinterpret_cast<const u32x4*>(src + d0);
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
    }
}

int launch_rope_append_multi(const hyd_rope_multi_params& p, hipStream_t s) {
    const int64_t threads = (int64_t)p.B * p.T * (p.Hq + 2 * p.Hkv) * (p.D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;
#define HYD_ROPE(TT, DD) hipLaunchKernelGGL((rope_append_multi_kernel<TT, DD>), dim3(grid), dim3(256), 0, s, p)
    if (p.dtype == HYD_F16) {
        if (p.D == 128) HYD_ROPE(F16, 128);
        else if (p.D == 64) HYD_ROPE(F16, 64);
        else if (p.D == 256) HYD_ROPE(F16, 256);
        else return (int)hipErrorInvalidValue;
    } else {
        if (p.D == 128) HYD_ROPE(BF16, 128);
        else if (p.D == 64) HYD_ROPE(BF16, 64);
        else if (p.D == 256) HYD_ROPE(BF16, 256);
        else return (int)hipErrorInvalidValue;
    }
#undef HYD_ROPE
    return (int)hipGetLastError();
}

int launch_rope_append(const RopeArgs& a, int dtype, int D, hipStream_t s) {
    const int64_t threads = (int64_t)a.B * (a.Hq + 2 * a.Hkv) * (D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;
#define HYD_ROPE(TT, DD) hipLaunchKernelGGL((rope_append_kernel<TT, DD>), dim3(grid), dim3(256), 0, s, a)
    if (dtype == HYD_F16) {
        if (D == 128) HYD_ROPE(F16, 128);
        else if (D == 64) HYD_ROPE(F16, 64);
        else if (D == 256) HYD_ROPE(F16, 256);
        else return (int)hipErrorInvalidValue;
    } else {
        if (D == 128) HYD_ROPE(BF16, 128);
        else if (D == 64) HYD_ROPE(BF16, 64);
        else if (D == 256) HYD_ROPE(BF16, 256);
        else return (int)hipErrorInvalidValue;
    }
#undef HYD_ROPE
    return (int)hipGetLastError();
}

// Per-head q/k RMSNorm in front of the rotation (hyd_qk_norm; Qwen3's self_attn.q_norm / k_norm): for a q row and a k row
//   r = rsqrt(mean_d(x_d^2) + eps),  n_d = x_d * r * w_d,  out = the rotation above applied to n,
// everything in fp32 on the widened 16-bit GEMM output and ONE rounding to the 16-bit dtype at the end (the RMSNorm convention of
// layer_ops.hip: multiply in fp32, round once).  v rows are copied as they are.  A thread holds 16 of its row's D elements, so the
// sum of squares is 16 terms per lane and a butterfly over the row's TPR = D / 16 adjacent lanes -- DPP moves inside one 16-lane
// row of the wave, no LDS --, after which every lane of the row holds the same bits.  The lanes of a row enter the butterfly
// together: the bounds exit and the q / k / v branch are decided per row, and every cache-index guard sits behind it.  A ragged
// last wave ends on a row boundary (256 % TPR == 0), so no live lane reads one that has left.
struct RopeNormArgs {
    const void* q_weight;  // [D], the q dtype
    const void* k_weight;
    float eps;
};

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

// The normalised, rotated row the three kernels below share: a token gets the same bits from each of them.  src: the row's D
// elements, w: the gain vector, cr / sr: the position's table rows.  The products of the rotation are rope8's.
template <typename T, int D>
__device__ __forceinline__ void rope_norm_row(const uint16_t* src, const uint16_t* w, float eps, const float* cr, const float* sr, int d0,
                                              u32x4& olo, u32x4& ohi) {
    using TR = Traits<T>;
    const u32x4 lo = *reinterpret_cast<const u32x4*>(src + d0);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
    const u32x4 wlo = *reinterpret_cast<const u32x4*>(w + d0);
    const u32x4 whi = *reinterpret_cast<const u32x4*>(w + D / 2 + d0);
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr + d0), c1 = *reinterpret_cast<const f32x4*>(cr + d0 + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr + d0), s1 = *reinterpret_cast<const f32x4*>(sr + d0 + 4);
    float x[8], y[8], gx[8], gy[8];
    widen8x<T>(lo, x);
    widen8x<T>(hi, y);
    widen8x<T>(wlo, gx);
    widen8x<T>(whi, gy);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += x[i] * x[i] + y[i] * y[i];
    ss = row_sum<D / 16>(ss);
    const float r = __builtin_amdgcn_rsqf(ss * (1.0f / D) + eps);  // v_rsq_f32: 1 ulp
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = x[i] * r * gx[i];
        y[i] = y[i] * r * gy[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float ca = i < 2 ? c0[2 * i] : c1[2 * i - 4], cb = i < 2 ? c0[2 * i + 1] : c1[2 * i - 3];
        const float sa = i < 2 ? s0[2 * i] : s1[2 * i - 4], sb = i < 2 ? s0[2 * i + 1] : s1[2 * i - 3];
        olo[i] = TR::pack2(x[2 * i] * ca - y[2 * i] * sa, x[2 * i + 1] * cb - y[2 * i + 1] * sb);
        ohi[i] = TR::pack2(y[2 * i] * ca + x[2 * i] * sa, y[2 * i + 1] * cb + x[2 * i + 1] * sb);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void rope_append_norm_kernel(const RopeArgs a, const RopeNormArgs n) {
    constexpr int TPR = D / 16;
    const int rows_per_b = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / TPR;
    const int sub = (int)(gid % TPR);
    if (row >= (int64_t)a.B * rows_per_b) return;
    const int b = (int)(row / rows_per_b);
    const int h = (int)(row % rows_per_b);
    const int64_t pos_raw = a.pos[(int64_t)b * a.pos_stride];
    const int64_t idx = pos_raw - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0) a.seq_lens[b] = (int32_t)(idx + 1);
    const int d0 = sub * 8;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_bs + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)(h - a.Hq) * D;
        u32x4 olo, ohi;
        rope_norm_row<T, D>(src, static_cast<const uint16_t*>(isq ? n.q_weight : n.k_weight), n.eps, a.cos + pos * a.cs_stride,
                            a.sin + pos * a.cs_stride, d0, olo, ohi);
        uint16_t* dst;
        if (isq) {
            dst = static_cast<uint16_t*>(a.q_out) + ((int64_t)b * a.Hq + h) * D;
        } else {
            if (idx < 0 || idx >= a.cache_len) return;  // out of the allocated cache: never write out of bounds
            dst = static_cast<uint16_t*>(a.k_cache) + (int64_t)b * a.kc_bs + idx * a.kc_ts + (int64_t)(h - a.Hq) * a.kc_hs;
        }
        *reinterpret_cast<u32x4*>(dst + d0) = olo;
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = ohi;
    } else {
        if (idx < 0 || idx >= a.cache_len) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hv * D;
        uint16_t* dst = static_cast<uint16_t*>(a.v_cache) + (int64_t)b * a.vc_bs + idx * a.vc_ts + (int64_t)hv * a.vc_hs;
        *reinterpret_cast<u32x4*>(dst + d0) = *reinterpret_cast<const u32x4*>(src + d0);
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void rope_append_norm_fp8_kernel(const RopeKvqArgs ka, const RopeNormArgs n) {
    const RopeArgs& a = ka.a;
    constexpr int TPR = D / 16;
    const int rows_per_b = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / TPR;
    const int sub = (int)(gid % TPR);
    if (row >= (int64_t)a.B * rows_per_b) return;
    const int b = (int)(row / rows_per_b);
    const int h = (int)(row % rows_per_b);
    const int64_t pos_raw = a.pos[(int64_t)b * a.pos_stride];
    const int64_t idx = pos_raw - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0) a.seq_lens[b] = (int32_t)(idx + 1);
    const int d0 = sub * 8;
    u32x4 olo, ohi;
    float s;
    uint8_t* dst8;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_bs + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)(h - a.Hq) * D;
        rope_norm_row<T, D>(src, static_cast<const uint16_t*>(isq ? n.q_weight : n.k_weight), n.eps, a.cos + pos * a.cs_stride,
                            a.sin + pos * a.cs_stride, d0, olo, ohi);
        if (isq) {
            uint16_t* dst = static_cast<uint16_t*>(a.q_out) + ((int64_t)b * a.Hq + h) * D;
            *reinterpret_cast<u32x4*>(dst + d0) = olo;
            *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = ohi;
            return;
        }
        if (idx < 0 || idx >= a.cache_len) return;  // out of the allocated cache: never write out of bounds
        const int hk = h - a.Hq;
        s = ka.k_scale ? ka.k_scale[hk] : 1.0f;
        dst8 = static_cast<uint8_t*>(a.k_cache) + (int64_t)b * a.kc_bs + idx * a.kc_ts + (int64_t)hk * a.kc_hs;
    } else {
        if (idx < 0 || idx >= a.cache_len) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hv * D;
        olo = *reinterpret_cast<const u32x4*>(src + d0);
        ohi = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
        s = ka.v_scale ? ka.v_scale[hv] : 1.0f;
        dst8 = static_cast<uint8_t*>(a.v_cache) + (int64_t)b * a.vc_bs + idx * a.vc_ts + (int64_t)hv * a.vc_hs;
    }
    float xl[8], xh[8];
    widen8x<T>(olo, xl);
    widen8x<T>(ohi, xh);
    *reinterpret_cast<u32x2*>(dst8 + d0) = quant_fp8x8(xl, s);
    *reinterpret_cast<u32x2*>(dst8 + D / 2 + d0) = quant_fp8x8(xh, s);
}

template <typename T, int D>
__global__ __launch_bounds__(256) void rope_append_norm_multi_kernel(const hyd_rope_multi_params a, const RopeNormArgs n) {
    constexpr int TPR = D / 16;
    const int rows_per_t = a.Hq + 2 * a.Hkv;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / TPR;
    const int sub = (int)(gid % TPR);
    if (row >= (int64_t)a.B * a.T * rows_per_t) return;
    const int h = (int)(row % rows_per_t);
    const int64_t bt = row / rows_per_t;
    const int b = (int)(bt / a.T), i = (int)(bt % a.T);
    const int64_t pos0 = a.position_ids[(int64_t)b * a.pos_stride];
    const int64_t idx0 = pos0 - (a.shared_len ? a.shared_len[b] : 0);
    const int64_t idx = idx0 + i, pos_raw = pos0 + i;
    const int64_t pos = pos_raw < 0 ? 0 : (pos_raw >= a.max_pos ? (int64_t)a.max_pos - 1 : pos_raw);
    if (h == 0 && sub == 0 && i == 0) a.seq_lens[b] = idx0 >= 0 ? (int32_t)(idx0 + a.T) : 0;
    const bool store_kv = idx0 >= 0 && idx < a.cache_len;  // never write out of bounds, never for a retired row
    const int d0 = sub * 8;
    if (h < a.Hq + a.Hkv) {
        const bool isq = h < a.Hq;
        const uint16_t* src = isq ? static_cast<const uint16_t*>(a.q) + (int64_t)b * a.q_batch_stride + (int64_t)i * a.q_tok_stride + (int64_t)h * D
                                  : static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_batch_stride + (int64_t)i * a.k_tok_stride + (int64_t)(h - a.Hq) * D;
        u32x4 olo, ohi;
        rope_norm_row<T, D>(src, static_cast<const uint16_t*>(isq ? n.q_weight : n.k_weight), n.eps, a.cos + pos * a.cs_stride,
                            a.sin + pos * a.cs_stride, d0, olo, ohi);
        if (!isq && !store_kv) return;
        uint16_t* dst = isq ? static_cast<uint16_t*>(a.q_out) + (bt * a.Hq + h) * D
                            : static_cast<uint16_t*>(a.k_cache) + (int64_t)b * a.kc_batch_stride + idx * a.kc_tok_stride + (int64_t)(h - a.Hq) * a.kc_head_stride;
        *reinterpret_cast<u32x4*>(dst + d0) = olo;
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = ohi;
    } else {
        if (!store_kv) return;
        const int hv = h - a.Hq - a.Hkv;
        const uint16_t* src = static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_batch_stride + (int64_t)i * a.v_tok_stride + (int64_t)hv * D;
        uint16_t* dst = static_cast<uint16_t*>(a.v_cache) + (int64_t)b * a.vc_batch_stride + idx * a.vc_tok_stride + (int64_t)hv * a.vc_head_stride;
        *reinterpret_cast<u32x4*>(dst + d0) = *reinterpret_cast<const u32x4*>(src + d0);
        *reinterpret_cast<u32x4*>(dst + D / 2 + d0) = *reinterpret_cast<const u32x4*>(src + D / 2 + d0);
    }
}

// one dispatch over {f16, bf16} x {64, 128, 256} for the three norm kernels: KERNEL is the template's name, the rest its arguments
#define HYD_ROPE_NORM_DISPATCH(KERNEL, dtype, D, grid, s, ...)                                            \
    do {                                                                                                  \
        if ((dtype) == HYD_F16) {                                                                         \
            if ((D) == 128) hipLaunchKernelGGL((KERNEL<F16, 128>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);       \
            else if ((D) == 64) hipLaunchKernelGGL((KERNEL<F16, 64>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);    \
            else if ((D) == 256) hipLaunchKernelGGL((KERNEL<F16, 256>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);  \
            else return (int)hipErrorInvalidValue;                                                        \
        } else {                                                                                          \
            if ((D) == 128) hipLaunchKernelGGL((KERNEL<BF16, 128>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);      \
            else if ((D) == 64) hipLaunchKernelGGL((KERNEL<BF16, 64>), dim3(grid), dim3(256), 0, s, __VA_ARGS__);   \
            else if ((D) == 256) hipLaunchKernelGGL((KERNEL<BF16, 256>), dim3(grid), dim3(256), 0, s, __VA_ARGS__); \
            else return (int)hipErrorInvalidValue;                                                        \
        }                                                                                                 \
    } while (0)

int launch_rope_append_norm(const RopeArgs& a, const RopeKvqArgs* ka, const void* q_weight, const void* k_weight, float eps, int dtype, int D,
                            hipStream_t s) {
    const RopeNormArgs n = {q_weight, k_weight, eps};
    const int64_t threads = (int64_t)a.B * (a.Hq + 2 * a.Hkv) * (D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;
    if (ka) HYD_ROPE_NORM_DISPATCH(rope_append_norm_fp8_kernel, dtype, D, grid, s, *ka, n);
    else HYD_ROPE_NORM_DISPATCH(rope_append_norm_kernel, dtype, D, grid, s, a, n);
    return (int)hipGetLastError();
}

int launch_rope_append_norm_multi(const hyd_rope_multi_params& p, const void* q_weight, const void* k_weight, float eps, hipStream_t s) {
    const RopeNormArgs n = {q_weight, k_weight, eps};
    const int64_t threads = (int64_t)p.B * p.T * (p.Hq + 2 * p.Hkv) * (p.D / 16);
    const int grid = (int)((threads + 255) / 256);
    if (grid == 0) return 0;
    HYD_ROPE_NORM_DISPATCH(rope_append_norm_multi_kernel, p.dtype, p.D, grid, s, p, n);
    return (int)hipGetLastError();
}
#undef HYD_ROPE_NORM_DISPATCH

}  // namespace hyd
