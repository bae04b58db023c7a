// Calibrate the fp8 unique caches' per-kv-head scales (hyd_kv_absmax, hyd_kv_scales_from_absmax; include/hydragen_hip.h states
// the rules, hydragen_amd/kv_quant.py holds the definitions in torch).
//
// kv_absmax_kernel: max |x| per kv head over a strided 16-bit view [n_outer, n_rows, Hkv, d], K and V in one launch.  A read,
// HBM bound.  A token row is vpr = Hkv * d / 8 16-byte pieces; a lane owns ONE piece column for the whole launch -- so one head:
// its running maximum stays in registers across the rows -- and a workgroup covers kPasses row steps of its column block, kUnroll
// loads in flight per lane.  Narrow rows (vpr < 256) put 256 / vpr rows side by side in a workgroup.  |x| of a finite 16-bit float
// orders as its 15 low bits do as an integer, so the loop is integer work on packed halves: clear the sign, zero NaN / inf
// (exponent all ones), unsigned max.  Then lanes of one head meet by wave shuffles (the largest power of two that divides the
// head's pieces), waves through LDS, and ONE integer atomic max per (workgroup, head, tensor) on the fp32 bit pattern of the
// widened maximum goes to amax [2, Hkv]: a maximum does not depend on the order, the result is exact.  Rows at or past
// row_lens[o] and columns at or past d are never read.  No scratch, no assembly, plain vector atomics.
//
// kv_scales_kernel: amax [2, Hkv] -> k_scale / v_scale [Hkv] by exponent arithmetic on the bits of amax * c.
#include "hyd_kernels.h"

namespace hyd {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 8;                  // 16-byte loads in flight per lane
constexpr int kPasses = HYD_KV_ABSMAX_PASSES;  // row steps per workgroup (two batches of kUnroll)
constexpr int kHeadSlots = kThreads + 8;    // heads a workgroup's 256 piece columns can touch: <= 256 / pph + 2
static_assert(kPasses % kUnroll == 0, "whole batches");

__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv& f) {
    const unsigned t = __umulhi(n, f.mul);
    return (t + ((n - t) >> (f.sh & 0xffu))) >> (f.sh >> 8);
}

// two 16-bit floats in one dword -> their magnitudes' bit patterns, 0 for NaN / inf.  kInf: the exponent mask (f16 0x7c00, bf16
// 0x7f80); a + (0x8000 - kInf) carries into bit 15 of its half exactly when a >= kInf, and never out of the half (a <= 0x7fff)
template <uint32_t kInf>
__device__ __forceinline__ uint32_t finite_abs2(uint32_t w) {
    const uint32_t a = w & 0x7fff7fffu;
    const uint32_t over = ((a + (0x8000u - kInf) * 0x00010001u) >> 15) & 0x00010001u;
    return a & ~(over * 0xffffu);
}

__device__ __forceinline__ uint32_t max_u16x2(uint32_t a, uint32_t b) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

}  // namespace

// grid (row chunks x outer, column blocks, tensors)
template <typename T>
__global__ __launch_bounds__(kThreads) void kv_absmax_kernel(const KvAbsmaxArgs a) {
    constexpr uint32_t kInf = __is_same(T, _Float16) ? 0x7c00u : 0x7f80u;  // the exponent mask: at or above it, NaN / inf
    __shared__ unsigned smax[kHeadSlots];
    const unsigned t = threadIdx.x;
    const unsigned o = fdiv(blockIdx.x, a.div_chunks), chunk = blockIdx.x - o * (unsigned)a.chunks;
    const int len = a.row_lens ? min(max(a.row_lens[o], 0), a.n_rows) : a.n_rows;
    const int row0 = (int)chunk * (kPasses * a.rstep);
    if (row0 >= len) return;  // (uniform per workgroup: nothing of this chunk is inside the length)

    for (unsigned i = t; i < (unsigned)kHeadSlots; i += kThreads) smax[i] = 0u;
    __syncthreads();

    const bool is_v = a.only ? a.only == 2 : blockIdx.z != 0;
    const char* src = static_cast<const char*>(is_v ? a.v : a.k);
    const int64_t os = is_v ? a.v_os : a.k_os, rs = is_v ? a.v_rs : a.k_rs, hs = is_v ? a.v_hs : a.k_hs;

    // this lane's piece column c of the token row (head h, piece c - h * pph) and its row within a step of rstep rows
    const unsigned rsub = fdiv(t, a.div_cols);
    const unsigned c0 = (unsigned)blockIdx.y * (unsigned)a.cols;
    const unsigned c = c0 + (t - rsub * (unsigned)a.cols);
    const bool active = rsub < (unsigned)a.rstep && c < (unsigned)a.vpr;
    const unsigned h = fdiv(c, a.div_pph), h0 = fdiv(c0, a.div_pph);

    u32x4 m = u32x4{0u, 0u, 0u, 0u};
    if (active) {
        const char* p = src + ((int64_t)o * os + (int64_t)h * hs + (int64_t)(c - h * (unsigned)a.pph) * 8) * 2;
        const int64_t step = (int64_t)a.rstep * rs * 2;
        int row = row0 + (int)rsub;
        p += (int64_t)row * rs * 2;
#pragma unroll 1
        for (int b = 0; b < kPasses / kUnroll; ++b) {
            if (row >= len) break;
            u32x4 x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                x[u] = u32x4{0u, 0u, 0u, 0u};
                if (row + u * a.rstep < len) x[u] = *reinterpret_cast<const u32x4*>(p + u * step);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = max_u16x2(m[j], finite_abs2<kInf>(x[u][j]));
            }
            row += kUnroll * a.rstep;
            p += kUnroll * step;
        }
    }
    // eight magnitudes -> one, widened to the fp32 that holds it exactly: non-negative floats order as their bits do
    uint32_t m2 = max_u16x2(max_u16x2(m[0], m[1]), max_u16x2(m[2], m[3]));
    const uint32_t m1 = max(m2 & 0xffffu, m2 >> 16);
    unsigned bits;
    if (kInf == 0x7c00u)
        bits = __builtin_bit_cast(unsigned, (float)__builtin_bit_cast(_Float16, (uint16_t)m1));
    else
        bits = m1 << 16;
    // lanes of one head: aligned groups of `group` lanes hold pieces of one head (group divides pph, cols and the column base)
    for (int off = a.group >> 1; off > 0; off >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, off));
    if (active && (t & (unsigned)(a.group - 1)) == 0u && bits != 0u) atomicMax(&smax[h - h0], bits);
    __syncthreads();
    for (unsigned i = t; i < (unsigned)kHeadSlots; i += kThreads) {
        const unsigned v = smax[i];
        if (v != 0u) atomicMax(a.amax + (is_v ? a.Hkv : 0) + (int)(h0 + i), v);  // (v != 0: a column of head h0 + i < Hkv was read)
    }
}

// one lane per (tensor, head)
__global__ void kv_scales_kernel(const KvScalesArgs a) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= 2 * a.Hkv) return;
    const float amax = a.amax[i];
    float* out = i < a.Hkv ? a.k_scale + i : a.v_scale + (i - a.Hkv);
    if ((__builtin_bit_cast(unsigned, amax) & 0x7fffffffu) == 0u) {  // nothing observed, or an all-zero head (bits: a subnormal is not 0)
        *out = 1.0f;
        return;
    }
    const float t = amax * a.c;
    if (!a.pow2) {
        *out = fminf(fmaxf(t, 0x1p-100f), 0x1p100f);
        return;
    }
    // the smallest power of two >= t: the exponent field, one more unless the mantissa is zero.  A subnormal or zero t has field 0
    // and inf has 255: the clamp to [2^-100, 2^100] covers both
    const unsigned u = __builtin_bit_cast(unsigned, t);
    int e = (int)((u >> 23) & 0xffu) - 127 + ((u & 0x7fffffu) != 0u ? 1 : 0);
    e = min(max(e, -100), 100);
    *out = __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

int launch_kv_absmax(const KvAbsmaxArgs& a, int dtype, hipStream_t s) {
    const int64_t gx = (int64_t)a.chunks * a.n_outer;
    const int gy = (a.vpr + a.cols - 1) / a.cols;
    if (gx <= 0 || gx > 0x7fffffffLL || gy <= 0 || gy > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy, a.only ? 1 : 2), block(kThreads);
    if (dtype == HYD_F16)
        hipLaunchKernelGGL(kv_absmax_kernel<_Float16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(kv_absmax_kernel<__bf16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_kv_scales(const KvScalesArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(kv_scales_kernel, dim3((2 * a.Hkv + 255) / 256), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
