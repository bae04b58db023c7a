// Suffix pass over fp8 unique caches (hyd_kv_quant, include/hydragen_hip.h): the token-row kernel of suffix_attn.hip with
// e4m3fn K / V bytes.  q, the prefix partials and the output stay 16-bit; only the per-sequence cache is quantized, with one
// fp32 scale per kv head and tensor (stored value = x / scale[h], hydragen_amd/kv_quant.py).
//
// Same mapping as suffix_attn_rows_kernel: a wave walks the token rows of ONE sequence for HPI = 64 / (D / 8) neighbouring heads,
// a lane group of D / 8 lanes owns one head, a lane owns 8 dims -- now 8 BYTES per token and tensor (one dwordx2 request; one
// wave instruction covers 512 contiguous bytes at D = 128).  q, finish_row, the partial prefetch, seq_order, the token split and
// NPRE 1 / 2 are those of the 16-bit kernel.
//   K: four v_cvt_scalef32_pk_{bf16,f16}_fp8 (scale 1) rebuild the u32x4 of 16-bit values the v_dot2 loop consumes;
//   V: four v_cvt_pk_f32_fp8 give the 8 floats widen8 gives the 16-bit kernel.
// Both conversions are exact (every e4m3fn value is a bf16 and an f16 value): the quantization is the only new rounding.
// The scales cost nothing per element: k_scale[h] is folded into the lane's score multiplier, v_scale[h] multiplies the
// accumulator once, after the token-split merge and before the epilogue.
// UT = 8 tokens per chunk (4 KB of K + V in flight per wave, half the 16-bit kernel's bytes): UT = 16 would keep the 16-bit
// kernel's bytes in flight, but hipcc then needs 152-166 VGPRs (spills at 4 waves per SIMD, 3 waves per SIMD without).
// Every cache length takes this kernel (the 16-bit rule that sends caches of more than 1024 rows to the one-unit-per-wave
// kernel is a 16-bit measurement; there is no fp8 one-unit kernel).
#include <type_traits>

#include "suffix_common.h"

namespace hyd {

typedef const __attribute__((address_space(1))) u32x2* gu32x2_p;

// 8 e4m3fn bytes -> 8 values of T packed as the 16-bit kernel's u32x4 (dims 2i, 2i + 1 in dword i)
template <typename T>
__device__ __forceinline__ u32x4 fp8x8_to_16(const u32x2& v) {
    u32x4 r;
    if constexpr (std::is_same<T, BF16>::value) {
        r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[0], 1.0f, false));
        r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[0], 1.0f, true));
        r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[1], 1.0f, false));
        r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[1], 1.0f, true));
    } else {
        r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[0], 1.0f, false));
        r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[0], 1.0f, true));
        r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[1], 1.0f, false));
        r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[1], 1.0f, true));
    }
    return r;
}

// 8 e4m3fn bytes -> 8 floats
__device__ __forceinline__ void fp8x8_to_f32(const u32x2& v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], true);
        f[4 * i] = lo[0];
        f[4 * i + 1] = lo[1];
        f[4 * i + 2] = hi[0];
        f[4 * i + 3] = hi[1];
    }
}

template <typename T, int D, int UT, int NPRE, int TS = 1>
__global__ __launch_bounds__(256, 4) void suffix_attn_rows_fp8_kernel(const SuffixKvqArgs ka) {
    using TR = Traits<T>;
    const SuffixArgs& a = ka.a;
    warm_kernargs_256();
    constexpr int LPK = D / 8, HPI = 64 / LPK;  // lanes per head row, heads per wave instruction
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane % LPK, hg = lane / LPK;
    constexpr int TL = TS == 4 ? 2 : TS == 2 ? 1 : 0;
    const int ts_id = wave & (TS - 1), wrest = wave >> TL;
    const int wl = a.rows_wps_log2;
    const int bslot = (int)(blockIdx.x << (2 - wl - TL)) + (wrest >> wl);
    const int h0 = (int)((blockIdx.y << wl) + (wrest & ((1 << wl) - 1))) * HPI;  // first head of this wave
    if (bslot >= a.B || h0 >= a.Hkv) return;  // (all TS waves of a group leave together: a barrier counts the waves that are left)

    // the length as a vector load (see suffix_attn_rows_kernel)
    int zero = 0;
    asm volatile("" : "+v"(zero));
    const int b = a.order ? __builtin_amdgcn_readfirstlane(a.order[bslot + zero]) : bslot;
    int lenv = a.kv_len;
    if (a.sl32) lenv = a.sl32[b + zero];
    else if (a.sl64) lenv = (int)a.sl64[b + zero];

    const int hk = h0 + hg;
    const int64_t ridx = (int64_t)b * a.Hq + hk;  // nq == 1, g == 1: [B, 1, Hq]
    const u32x4 qp = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(a.q) + ridx * D + sub * 8);
    const float ks = ka.k_scale ? ka.k_scale[hk] : 1.0f;
    const float vs = ka.v_scale ? ka.v_scale[hk] : 1.0f;
    PrePartials<NPRE> pp;
    const int npre = min(n_prefetched(a), NPRE);
    prefetch_partials(a, npre, ridx, sub, D, pp);

    // wave-uniform base (scalar registers) + per-lane 32-bit byte offset (head, dims); strides are in bytes here
    const gchar_p kbu = uniform_ptr(static_cast<const char*>(a.k) + (int64_t)b * a.k_bs + (int64_t)h0 * a.k_hs);
    const gchar_p vbu = uniform_ptr(static_cast<const char*>(a.v) + (int64_t)b * a.v_bs + (int64_t)h0 * a.v_hs);
    unsigned khg = (unsigned)hg * (unsigned)a.k_hs, vhg = (unsigned)hg * (unsigned)a.v_hs;
    asm volatile("" : "+v"(khg), "+v"(vhg));
    const unsigned klane = khg + sub * 8, vlane = vhg + sub * 8;
    const unsigned krs = (unsigned)a.k_ts, vrs = (unsigned)a.v_ts;

    u32x2 kreg[UT], vreg[UT];
    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const float sc = a.scale_log2e * ks;  // k = k8 * ks: the scale rides on the score multiplier

    const int len = max(0, min(__builtin_amdgcn_readfirstlane(lenv), a.kv_len));
    const int nch = (len + UT - 1) / UT;
    const int last = max(len - 1, 0);

    auto issue_k = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const unsigned tc = (unsigned)min(c * UT + u, last);
            kreg[u] = __builtin_nontemporal_load((gu32x2_p)(kbu + (tc * krs + klane)));
        }
    };
    auto issue_v = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const unsigned tc = (unsigned)min(c * UT + u, last);
            vreg[u] = __builtin_nontemporal_load((gu32x2_p)(vbu + (tc * vrs + vlane)));
        }
    };
    auto chunk = [&](int c, auto LAST) __attribute__((always_inline)) {
        constexpr bool is_last = decltype(LAST)::value;
        float sv[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const u32x4 kk = fp8x8_to_16<T>(kreg[u]);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) d = TR::dot2(qp[e], kk[e], d);
            d = group_sum<LPK>(d) * sc;
            sv[u] = (!is_last || c * UT + u < len) ? d : -INFINITY;  // wave-uniform condition
        }
        if constexpr (!is_last) {
            __builtin_amdgcn_sched_barrier(0);
            issue_k(c + TS);
            __builtin_amdgcn_sched_barrier(0);
        }
        float cmax = sv[0];
#pragma unroll
        for (int u = 1; u < UT; ++u) cmax = fmaxf(cmax, sv[u]);
        const float mnew = fmaxf(m, cmax);  // finite: every chunk that is processed starts with a valid key
        const float alpha = fast_exp2(m - mnew);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            sv[u] = fast_exp2(sv[u] - mnew);
            ps += sv[u];
        }
        l = l * alpha + ps;
        m = mnew;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] *= alpha;
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            float vf[8];
            fp8x8_to_f32(vreg[u], vf);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(sv[u], vf[j], acc[j]);
        }
        if constexpr (!is_last) {
            __builtin_amdgcn_sched_barrier(0);
            issue_v(c + TS);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (nch > ts_id) {  // (a wave without a chunk requests nothing: an empty sequence's cache may have no rows at all)
        issue_k(ts_id);
        issue_v(ts_id);
        __builtin_amdgcn_sched_barrier(0);
        int c = ts_id;
        for (; c + TS < nch; c += TS) chunk(c, std::integral_constant<bool, false>{});
        chunk(c, std::integral_constant<bool, true>{});
    }
    if constexpr (TS > 1) {
        __shared__ float xch[4][10][64];  // [wave of the workgroup][m, l, acc[8]][lane]
        if (ts_id > 0) {
            xch[wave][0][lane] = m;
            xch[wave][1][lane] = l;
#pragma unroll
            for (int j = 0; j < 8; ++j) xch[wave][2 + j][lane] = acc[j];
        }
        __syncthreads();
        if (ts_id > 0) return;
#pragma unroll
        for (int t = 1; t < TS; ++t) {
            float a2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a2[j] = xch[wave + t][2 + j][lane];
            merge_state(m, l, acc, xch[wave + t][0][lane], xch[wave + t][1][lane], a2);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= vs;  // v = v8 * vs, once per row
    finish_row<T, D, 2, NPRE>(a, ridx, sub, m, l, acc, npre, pp);
}

// shapes only (capture-safe): one query row per unit, whole lane groups, 32-bit byte offsets inside a sequence's cache
bool suffix_fp8_eligible(const SuffixArgs& a, int D) {
    if (D != 64 && D != 128 && D != 256) return false;
    const int hpi = 64 / (D / 8);
    const int64_t span = (int64_t)a.kv_len * (a.k_ts > a.v_ts ? a.k_ts : a.v_ts) +
                         (int64_t)a.Hkv * (a.k_hs > a.v_hs ? a.k_hs : a.v_hs);
    return a.rows == 1 && a.nq == 1 && a.g == 1 && a.Hkv % hpi == 0 && span < ((int64_t)1 << 31) && a.n_pre <= 2;
}

template <typename T, int D>
static int launch_rows_fp8(const SuffixKvqArgs& ka0, hipStream_t s) {
    constexpr int HPI = 64 / (D / 8), UT = 8;
    SuffixKvqArgs ka = ka0;
    SuffixArgs& a = ka.a;
    const int wps = a.Hkv / HPI;  // waves per sequence
    a.rows_wps_log2 = wps >= 3 ? 2 : wps == 2 ? 1 : 0;
    const int wl = a.rows_wps_log2;
    // token split as in the 16-bit kernel (one wave per sequence: share a sequence between 2 / 4 waves)
    int ts = 1;
    if (wl == 0 && a.n_pre < 2 && a.kv_len >= 32) ts = a.B <= 2048 ? 2 : 4;
    const int tl = ts == 4 ? 2 : ts == 2 ? 1 : 0;
    const dim3 grid((unsigned)((a.B + (4 >> (wl + tl)) - 1) >> (2 - wl - tl)), (unsigned)((wps + (1 << wl) - 1) >> wl), 1);
#define HYD_FP8_LAUNCH(KERNEL) \
    do { hipLaunchKernelGGL((KERNEL), grid, dim3(256), 0, s, ka); return (int)hipGetLastError(); } while (0)
    if (a.n_pre == 2) HYD_FP8_LAUNCH((suffix_attn_rows_fp8_kernel<T, D, UT, 2>));
    if (ts == 4) HYD_FP8_LAUNCH((suffix_attn_rows_fp8_kernel<T, D, UT, 1, 4>));
    if (ts == 2) HYD_FP8_LAUNCH((suffix_attn_rows_fp8_kernel<T, D, UT, 1, 2>));
    HYD_FP8_LAUNCH((suffix_attn_rows_fp8_kernel<T, D, UT, 1>));
#undef HYD_FP8_LAUNCH
}

int launch_suffix_fp8(const SuffixKvqArgs& a, int dtype, int D, hipStream_t s) {
    if (!suffix_fp8_eligible(a.a, D)) return (int)hipErrorInvalidValue;
    if (dtype == HYD_F16) {
        if (D == 128) return launch_rows_fp8<F16, 128>(a, s);
        if (D == 64) return launch_rows_fp8<F16, 64>(a, s);
        if (D == 256) return launch_rows_fp8<F16, 256>(a, s);
    } else {
        if (D == 128) return launch_rows_fp8<BF16, 128>(a, s);
        if (D == 64) return launch_rows_fp8<BF16, 64>(a, s);
        if (D == 256) return launch_rows_fp8<BF16, 256>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace hyd
