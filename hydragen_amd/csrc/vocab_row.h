// The one statement of what the logits kernels do to a vocabulary row, 1024 threads per row: Philox4x32-10 and the Gumbel noise of
// every sampling draw, order-preserving keys of the logits' bits, 8-element chunk loads, block reductions, fixed-point masses and
// the 256-bin select, and the closing log-prob expression.  Included by layer_ops.hip (sample_kernel: the noise), sample_select.h
// (sample_row: all of it; through it sample_filter.hip, sample_penalty_map.h, sample_penalty.hip, sample_constrain.hip) and
// token_logprob.hip (keys, masses, the select, the log-prob).  Five launches give the same bits because they read this text.
#pragma once
#include "hyd_kernels.h"

namespace hyd {

namespace {

constexpr int kFT = 1024;  // threads per row
constexpr int kFW = kFT / 64;
constexpr float kBinScale = 8.0f;     // first-level bins per unit of (max - l)
constexpr float kBinLast = 31.875f;   // 255 / kBinScale: from here on, the last bin
constexpr uint64_t kOne = 1ull << 40; // the max's mass

__device__ __forceinline__ void philox10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// standard Gumbel noise from 23 random bits: u = (k + 1/2) 2^-23 for k in [0, 2^23), strictly inside (0, 1) and exact in
// fp32 (24 significant bits).  (The former 24-bit form (k 2^-24 + 2^-25) rounded to exactly 1.0 for k = 2^24 - 1 -- a tie
// that rounds to even -- where -ln u = 0 and the noise is +inf: that column won the argmax whatever its logit, about two
// tokens per decode step at a batch of 1024 and a vocabulary of 32000.)  g = -ln(-ln u), finite for every k -- also on
// hardware whose approximate log2 returns 0 for the largest u (1 - 2^-24, true -ln u = 2^-24): -ln u is held at >= 2^-25.
__device__ __forceinline__ float gumbel_noise(uint32_t bits) {
    const float u = ((float)(bits >> 9) + 0.5f) * 0x1p-23f;
    const float e = fmaxf(-kLn2 * fast_log2(u), 0x1p-25f);
    return -kLn2 * fast_log2(e);
}

// order-preserving unsigned keys of the logit's bits; -0 is folded onto +0 (equal values, equal keys)
__device__ __forceinline__ uint32_t key16(uint32_t h) {
    h = h == 0x8000u ? 0u : h;
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
__device__ __forceinline__ uint32_t key32(uint32_t b) {
    b = b == 0x80000000u ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ bool valid(float f) { return f == f && f != -INFINITY; }

template <int DT>
__device__ __forceinline__ float h2f(uint32_t h) {
    return DT == HYD_F16 ? Traits<F16>::lo(h) : Traits<BF16>::lo(h);
}

// one 8-element chunk of 16-bit logits as 4 packed words (positions past n hold -inf)
template <int DT>
__device__ __forceinline__ u32x4 load16(const uint16_t* row, int c, int n, int vec) {
    if (vec && 8 * c + 8 <= n) return reinterpret_cast<const u32x4*>(row)[c];
    const uint32_t pad = DT == HYD_F16 ? 0xfc00u : 0xff80u;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = 8 * c + i < n ? row[8 * c + i] : pad;
    return u32x4{h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16};
}
template <int DT>
__device__ __forceinline__ void decode16(const u32x4& u, float (&f)[8], uint32_t (&k)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = u[i] & 0xffffu, hi = u[i] >> 16;
        f[2 * i] = h2f<DT>(lo);
        f[2 * i + 1] = h2f<DT>(hi);
        k[2 * i] = key16(lo);
        k[2 * i + 1] = key16(hi);
    }
}
__device__ __forceinline__ void load32(const float* row, int c, int n, int vec, float (&f)[8], uint32_t (&k)[8]) {
    uint32_t b[8];
    if (vec && 8 * c + 8 <= n) {
        const u32x4 u0 = reinterpret_cast<const u32x4*>(row)[2 * c], u1 = reinterpret_cast<const u32x4*>(row)[2 * c + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b[i] = u0[i];
            b[4 + i] = u1[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = 8 * c + i < n ? __builtin_bit_cast(uint32_t, row[8 * c + i]) : 0xff800000u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f[i] = __builtin_bit_cast(float, b[i]);
        k[i] = key32(b[i]);
    }
}

// Calls fn(chunk, f[8], key[8]) for every chunk this thread owns, read from memory (L2 / MALL after the first pass).
template <int DT, typename F>
__device__ __forceinline__ void visit(const void* row, int n, int vec, F&& fn) {
    const int nchunk = (n + 7) >> 3;
    for (int c = threadIdx.x; c < nchunk; c += kFT) {
        float f[8];
        uint32_t k[8];
        if constexpr (DT == HYD_F32) load32(static_cast<const float*>(row), c, n, vec, f, k);
        else decode16<DT>(load16<DT>(static_cast<const uint16_t*>(row), c, n, vec), f, k);
        fn(c, f, k);
    }
}

__device__ __forceinline__ float block_max(float x, float* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = red[0];
#pragma unroll
    for (int w = 1; w < kFW; ++w) x = fmaxf(x, red[w]);
    __syncthreads();
    return x;
}
__device__ __forceinline__ uint64_t block_sum(uint64_t x, uint64_t* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = 0;
#pragma unroll
    for (int w = 0; w < kFW; ++w) x += red[w];
    __syncthreads();
    return x;
}

// distance-to-max bin of the first select level; monotone: a larger logit never lands in a later bin
__device__ __forceinline__ int bin0(float f, float m) {
    const float d = f == m ? 0.f : m - f;
    return d < kBinLast ? (int)(d * kBinScale) : 255;
}
__device__ __forceinline__ uint64_t mass(float f, float m) {
    return f == m ? kOne : (uint64_t)(fast_exp2((f - m) * kLog2e) * 0x1p40f);
}
// log-prob of a logit l of a row with max m and mass sum `total` (the u64 sum, or that sum as a double): l - m - ln(total 2^-40)
template <typename Sum>
__device__ __forceinline__ float logprob_of(float l, float m, Sum total) {
    const double d = l == m ? 0.0 : (double)l - (double)m;
    return (float)(d - (log((double)total) - 40.0 * 0.6931471805599453));
}

struct Pick {
    int bin;
    uint64_t above;  // weight of the bins before `bin`, cum included
};

// First bin b (bin 0 = the largest logits) with cum + hist[0..b] >= target, by the first wave (4 bins per lane, one scan
// over the lanes); fill_last: hist[255] is not counted, it is `total` minus the other 255 bins.  Every thread gets it.
// The second form also stores hist[b] to *at: AT(x) is x there and nothing in the first form.  (One text as a macro, not as an
// inlined template: most kernels call pick_bin as a real function, and hipcc orders that function's instructions differently once
// its body arrives by inlining.)
#define HYD_PICK_BIN_BODY(AT)                                                   \
    if (threadIdx.x < 64) {                                                     \
        const int lane = threadIdx.x;                                           \
        uint64_t h[4];                                                          \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) h[i] = hist[4 * lane + i]; \
        if (fill_last && lane == 63) h[3] = 0;                                  \
        uint64_t s = h[0] + h[1] + h[2] + h[3];                                 \
        uint64_t incl = s;                                                      \
        _Pragma("unroll") for (int off = 1; off < 64; off <<= 1) {              \
            const uint64_t t = __shfl_up(incl, off);                            \
            if (lane >= off) incl += t;                                         \
        }                                                                       \
        if (fill_last) {                                                        \
            const uint64_t all = __shfl(incl, 63);                              \
            if (lane == 63) {                                                   \
                h[3] = total - all;                                             \
                incl += h[3];                                                   \
            }                                                                   \
        }                                                                       \
        const uint64_t cross = __ballot(cum + incl >= target);                  \
        const int first = cross ? __ffsll((long long)cross) - 1 : 63;           \
        if (lane == first) {                                                    \
            uint64_t c = cum + incl - (h[0] + h[1] + h[2] + h[3]);              \
            int b = 4 * lane + 3;                                               \
            AT(uint64_t hb = h[3];)                                             \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                     \
                if (c + h[i] >= target) {                                       \
                    b = 4 * lane + i;                                           \
                    AT(hb = h[i];)                                              \
                    break;                                                      \
                }                                                               \
                if (i < 3) c += h[i];                                           \
            }                                                                   \
            shared_pick->bin = b;                                               \
            shared_pick->above = c;                                             \
            AT(*at = hb;)                                                       \
        }                                                                       \
    }                                                                           \
    __syncthreads();                                                            \
    const Pick p = *shared_pick;                                                \
    __syncthreads();                                                            \
    return p;
#define HYD_PICK_AT(x) x
#define HYD_PICK_NO_AT(x)
__device__ Pick pick_bin(const uint64_t* hist, uint64_t cum, uint64_t target, bool fill_last, uint64_t total, Pick* shared_pick) {
    HYD_PICK_BIN_BODY(HYD_PICK_NO_AT)
}
__device__ Pick pick_bin(const uint64_t* hist, uint64_t cum, uint64_t target, bool fill_last, uint64_t total, Pick* shared_pick,
                         uint64_t* at) {
    HYD_PICK_BIN_BODY(HYD_PICK_AT)
}
#undef HYD_PICK_BIN_BODY
#undef HYD_PICK_AT
#undef HYD_PICK_NO_AT

}  // namespace

}  // namespace hyd
