// What the K/V copy kernels share (kv_promote.hip, kv_gather.hip): the launch-constant division and the widening of e4m3fn unique
// rows to a 16-bit shared level (kv_quant.dequantize_kv: float(q8) * scale[h] as an fp32 product, rounded once, ties to even).
#pragma once
#include "hyd_kernels.h"

namespace hyd {

namespace {

enum { kCopy16 = 0, kFp8ToF16 = 1, kFp8ToBf16 = 2 };

__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv& f) {
    const unsigned t = __umulhi(n, f.mul);
    return (t + ((n - t) >> (f.sh & 0xffu))) >> (f.sh >> 8);
}

// One value of the destination dtype from the fp32 product x of e4m3fn code `byte`: round to nearest, ties to even -- bf16 by the
// integer rule, f16 by the hardware conversion.  The NaN codes (0x7f, 0xff) get the encodings torch's casts give them, which
// dequantize_kv is defined by: bf16 the one quiet NaN 0x7fc0; f16 the sign of the code and the payload its fp32 widening
// (0x7ff00000) truncates to, 0x7f80 / 0xff80.
template <int MODE>
__device__ __forceinline__ uint32_t cvt1(float x, uint32_t byte) {
    const bool nan_code = (byte & 0x7fu) == 0x7fu;
    if (MODE == kFp8ToBf16) {
        const uint32_t u = __builtin_bit_cast(uint32_t, x);
        return (nan_code || x != x) ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
    const uint32_t h = __builtin_bit_cast(uint16_t, (_Float16)x);
    return nan_code ? (((byte & 0x80u) << 8) | 0x7f80u) : h;
}

// 8 e4m3fn bytes -> 8 values of the destination dtype (element j of the row in half j % 2 of dword j / 2)
template <int MODE>
__device__ __forceinline__ u32x4 widen8(const u32x2& v, float s) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t w = v[i];
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
        r[2 * i] = cvt1<MODE>(lo[0] * s, w & 0xffu) | (cvt1<MODE>(lo[1] * s, (w >> 8) & 0xffu) << 16);
        r[2 * i + 1] = cvt1<MODE>(hi[0] * s, (w >> 16) & 0xffu) | (cvt1<MODE>(hi[1] * s, w >> 24) << 16);
    }
    return r;
}

}  // namespace

}  // namespace hyd
