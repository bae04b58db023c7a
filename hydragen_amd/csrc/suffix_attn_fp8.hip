// Suffix pass over fp8 unique caches (hyd_kv_quant, include/hydragen_hip.h): the token-row kernel of suffix_rows.h instantiated
// for e4m3fn K / V bytes (this file holds the cache-format policy, its two conversions, the __global__ wrapper and the entry point).
// q, the prefix partials and the output stay 16-bit; only the per-sequence cache is quantized, with one fp32 scale per kv head
// and tensor (stored value = x / scale[h], hydragen_amd/kv_quant.py).
//
// The mapping is suffix_attn_rows_kernel's (the same body): a wave walks the token rows of ONE sequence for HPI = 64 / (D / 8) heads,
// a lane group of D / 8 lanes owns one head, a lane owns 8 dims -- now 8 BYTES per token and tensor (one dwordx2 request; one
// wave instruction covers 512 contiguous bytes at D = 128).
//   K: four v_cvt_scalef32_pk_{bf16,f16}_fp8 (scale 1) rebuild the u32x4 of 16-bit values the v_dot2 loop consumes;
//   V: four v_cvt_pk_f32_fp8 give the 8 floats widen8 gives the 16-bit kernel.
// Both conversions are exact (every e4m3fn value is a bf16 and an f16 value): the quantization is the only new rounding.
// The scales cost nothing per element: k_scale[h] is folded into the lane's score multiplier, v_scale[h] multiplies the
// accumulator once, after the token-split merge and before the epilogue.
// UT = 8 tokens per chunk (see suffix_rows.h).
// Every cache length takes this kernel (the 16-bit rule that sends caches of more than 1024 rows to the one-unit-per-wave
// kernel is a 16-bit measurement; there is no fp8 one-unit kernel).
#include <type_traits>

#include "suffix_rows.h"

namespace hyd {

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

struct RowsCacheFp8 {
    using elem = uint8_t;  // strides count bytes
    using vec = u32x2;     // 8 elements: one dwordx2 request
    static constexpr bool kScaled = true;
    template <typename T>
    static __device__ __forceinline__ u32x4 k_dot2(const u32x2& k) { return fp8x8_to_16<T>(k); }
    template <typename T>
    static __device__ __forceinline__ void v_f32(const u32x2& v, float (&f)[8]) { fp8x8_to_f32(v, f); }
};
template <typename T, int D, int UT, int NPRE, int TS = 1>
__global__ __launch_bounds__(256, 4) void suffix_attn_rows_fp8_kernel(const SuffixKvqArgs ka) {
    suffix_rows_body<T, D, UT, NPRE, TS, RowsCacheFp8>(ka.a, ka.k_scale, ka.v_scale);
}

// shapes only (capture-safe): one query row per unit, whole lane groups, 32-bit byte offsets inside a sequence's cache
bool suffix_fp8_eligible(const SuffixArgs& a, int D) {
    return (D == 64 || D == 128 || D == 256) && suffix_rows_shape_ok(a, D, 1);
}

template <typename T, int D>
static int launch_rows_fp8(const SuffixKvqArgs& ka, hipStream_t s) {
    return launch_suffix_rows<D>(ka, s, [](auto NPRE, auto TS) {
        return &suffix_attn_rows_fp8_kernel<T, D, 8, decltype(NPRE)::value, decltype(TS)::value>;
    });
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
