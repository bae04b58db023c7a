// Text shared by the skinny weight-streaming products (linear_w8.hip, moe.hip, moe_w8.hip): 256 threads = four waves per
// workgroup, W as the A operand of v_mfma_f32_16x16x32 with fp32 tiles per wave, e4m3fn codes widened in registers, and the
// waves' tiles meeting in LDS in wave order.
#pragma once
#include "hyd_kernels.h"

namespace hyd {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;

template <typename T>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma16<BF16>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma16<F16>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <typename T>
__device__ __forceinline__ uint32_t pack_exact(float lo, float hi);
template <>
__device__ __forceinline__ uint32_t pack_exact<BF16>(float lo, float hi) {  // the values are bf16 values: the upper halves
    return (__builtin_bit_cast(uint32_t, lo) >> 16) | (__builtin_bit_cast(uint32_t, hi) & 0xffff0000u);
}
template <>
__device__ __forceinline__ uint32_t pack_exact<F16>(float lo, float hi) {
    return Traits<F16>::pack2(lo, hi);
}

// 8 e4m3fn codes (the bytes of lo, then of hi) -> 8 values of T, element j in half j % 2 of dword j / 2
template <typename T>
__device__ __forceinline__ u32x4 widen_codes(uint32_t lo, uint32_t hi) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    return u32x4{pack_exact<T>(a[0], a[1]), pack_exact<T>(b[0], b[1]), pack_exact<T>(c[0], c[1]), pack_exact<T>(d[0], d[1])};
}

// [2][MT] fp32 tiles per wave: waves 1 .. 3 leave theirs in LDS; wave 0 (after the barrier) adds them to its own in wave order
template <int MT>
__device__ __forceinline__ void park_tiles(float* red, const f32x4 (&acc)[2][MT], int wave, int lane) {
    if (wave == 0) return;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(((wave - 1) * 2 + t) * MT + i) * 256 + r * 64 + lane] = acc[t][i][r];
}
template <int MT>
__device__ __forceinline__ void add_tiles(const float* red, f32x4 (&acc)[2][MT], int lane) {
#pragma unroll
    for (int w = 0; w < kWaves - 1; ++w)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][i][r] += red[((w * 2 + t) * MT + i) * 256 + r * 64 + lane];
}

}  // namespace

}  // namespace hyd
