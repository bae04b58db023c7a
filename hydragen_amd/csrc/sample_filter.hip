// Token sampling with top-k / top-p / min-p cuts and the sampled token's log-probability, one workgroup per row
// (hyd_sample_tokens_filtered, include/hydragen_hip.h).
//
//   * The cuts act on the UNSCALED distribution p = softmax(l) (the reference's apply_top_p, llama.py `apply_top_p`):
//     top-k keeps l >= the k-th largest logit (ties kept), top-p then keeps the smallest top set of the top-k survivors whose
//     renormalised mass reaches top_p (the crossing token and its ties kept), min-p keeps l - max >= ln(min_p).  Every cut
//     keeps a top set of the row, so the kept set is "key >= one threshold" plus the min-p test.
//   * The draw is argmax(l * (1/T) + g) over the kept tokens with the Gumbel noise g of sample_kernel (layer_ops.hip) bit for
//     bit: Philox4x32-10 counter (2 (j / 8) + (j % 8) / 4, row, offset lo, offset hi), key seed, word j % 4.
//   * Masses are fixed point, floor(exp(l - max) 2^40) in u64: integer sums do not depend on their order, so the kept set,
//     the token and the log-prob are the same for every run (LDS integer atomics, no float atomics).  n <= 2^22 keeps every
//     sum below 2^62.
//   * Thresholds are found by a select over 256-bin LDS histograms: a first level bins the distance to the max in steps of
//     1/8 (bin 255 = 31.875 and beyond, counted from the total instead of with atomics), then 8-bit radix levels over the
//     order-preserving key of the logit's own bits (2 levels for 16-bit logits, 4 for fp32) resolve the bin to one value.
// Mapping: 1024 threads; thread t owns the 8-element chunks t + 1024 j (16-byte loads when the row allows).  Every pass
// re-reads the row: it is 64-512 KB, so the passes after the first hit L2 / MALL.  (Keeping 16-bit rows in VGPRs across
// the passes -- up to 16 chunks per thread -- spilled to scratch at 4 and 8 chunks with this hipcc: DESIGN.md 4.11.)
#include "hyd_kernels.h"

namespace hyd {

namespace {

constexpr int kFT = 1024;  // threads per row
constexpr int kFW = kFT / 64;
constexpr float kBinScale = 8.0f;     // first-level bins per unit of (max - l)
constexpr float kBinLast = 31.875f;   // 255 / kBinScale: from here on, the last bin
constexpr uint64_t kOne = 1ull << 40; // the max's mass

__device__ __forceinline__ void philox10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {  // = layer_ops.hip philox4x32_10
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
__device__ __forceinline__ float gumbel_noise(uint32_t bits) {  // = layer_ops.hip gumbel
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

struct Pick {
    int bin;
    uint64_t above;  // weight of the bins before `bin`, cum included
};

// First bin b (bin 0 = the largest logits) with cum + hist[0..b] >= target, by the first wave (4 bins per lane, one scan
// over the lanes); fill_last: hist[255] is not counted, it is `total` minus the other 255 bins.  Every thread gets it.
__device__ Pick pick_bin(const uint64_t* hist, uint64_t cum, uint64_t target, bool fill_last, uint64_t total, Pick* shared_pick) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        uint64_t h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = hist[4 * lane + i];
        if (fill_last && lane == 63) h[3] = 0;
        uint64_t s = h[0] + h[1] + h[2] + h[3];
        uint64_t incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (fill_last) {
            const uint64_t all = __shfl(incl, 63);
            if (lane == 63) {
                h[3] = total - all;
                incl += h[3];
            }
        }
        const uint64_t cross = __ballot(cum + incl >= target);
        const int first = cross ? __ffsll((long long)cross) - 1 : 63;
        if (lane == first) {
            uint64_t c = cum + incl - (h[0] + h[1] + h[2] + h[3]);
            int b = 4 * lane + 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (c + h[i] >= target) {
                    b = 4 * lane + i;
                    break;
                }
                if (i < 3) c += h[i];
            }
            shared_pick->bin = b;
            shared_pick->above = c;
        }
    }
    __syncthreads();
    const Pick p = *shared_pick;
    __syncthreads();
    return p;
}

}  // namespace

template <int DT>
__global__ __launch_bounds__(1024) void sample_filter_kernel(const FilterArgs a) {
    constexpr int KB = DT == HYD_F32 ? 32 : 16;  // key bits
    __shared__ uint64_t hist[256];
    __shared__ float redf[kFW];
    __shared__ uint64_t redu[kFW];
    __shared__ float bestv[kFW];
    __shared__ int besti_w[kFW];
    __shared__ Pick pick;
    const int row = blockIdx.x;
    const int n = a.n;
    const int esz = DT == HYD_F32 ? 4 : 2;
    const void* rowp = static_cast<const char*>(a.logits) + (int64_t)row * a.row_stride * esz;

    // pass 1: max and the number of finite (or +inf) logits
    float m = -INFINITY;
    uint64_t nvalid = 0;
    visit<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (valid(f[i])) {
                m = fmaxf(m, f[i]);
                ++nvalid;
            }
        }
    });
    m = block_max(m, redf);
    nvalid = block_sum(nvalid, redu);
    if (nvalid == 0) {  // no finite logit: token 0, as sample_kernel
        if (threadIdx.x == 0) {
            a.out[row] = 0;
            if (a.kept) a.kept[row] = 0;
            if (a.logprobs) a.logprobs[row] = __builtin_nanf("");
        }
        return;
    }
    const bool topk = a.top_k > 0 && (uint64_t)a.top_k < nvalid;
    const bool topp = a.top_p < 1.0f;

    // pass 2: the softmax denominator (log-prob) and the first top-k level (counts per distance bin)
    uint64_t total = 0;
    if (topk) {
        for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
        __syncthreads();
    }
    if (topk || a.logprobs) {
        visit<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&)[8]) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (valid(f[i])) {
                    total += mass(f[i], m);
                    if (topk) {
                        const int b = bin0(f[i], m);
                        if (b < 255) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[b]), 1ull);
                    }
                }
            }
        });
        total = block_sum(total, redu);  // (its barriers also order the histogram before the pick)
    }

    // top-k: the k-th largest key
    uint32_t thr = 0;  // keep key >= thr (0: no cut on keys)
    if (topk) {
        const uint64_t k = (uint64_t)a.top_k;
        Pick p = pick_bin(hist, 0, k, true, nvalid, &pick);
        const int b = p.bin;
        uint32_t prefix = 0;
#pragma unroll
        for (int lvl = 0; lvl < KB / 8; ++lvl) {
            for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
            __syncthreads();
            const int sh = KB - 8 * (lvl + 1);
            visit<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (valid(f[i]) && bin0(f[i], m) == b && (lvl == 0 || (key[i] >> (sh + 8)) == prefix))
                        atomicAdd(reinterpret_cast<unsigned long long*>(&hist[255 - ((key[i] >> sh) & 255u)]), 1ull);
                }
            });
            __syncthreads();
            p = pick_bin(hist, p.above, k, false, 0, &pick);
            prefix = (prefix << 8) | (uint32_t)(255 - p.bin);
        }
        thr = prefix;
    }

    // top-p over the top-k survivors: the largest key whose top set holds ceil(top_p * their mass)
    if (topp) {
        for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
        __syncthreads();
        uint64_t tot1 = 0;
        const uint32_t kthr = thr;
        visit<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (valid(f[i]) && key[i] >= kthr) {
                    const uint64_t q = mass(f[i], m);
                    tot1 += q;
                    const int b = bin0(f[i], m);
                    if (b < 255 && q) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[b]), (unsigned long long)q);
                }
            }
        });
        tot1 = block_sum(tot1, redu);
        const uint64_t target = (uint64_t)ceil((double)a.top_p * (double)tot1);
        Pick p = pick_bin(hist, 0, target, true, tot1, &pick);
        const int b = p.bin;
        uint32_t prefix = 0;
#pragma unroll
        for (int lvl = 0; lvl < KB / 8; ++lvl) {
            for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
            __syncthreads();
            const int sh = KB - 8 * (lvl + 1);
            visit<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (valid(f[i]) && key[i] >= kthr && bin0(f[i], m) == b && (lvl == 0 || (key[i] >> (sh + 8)) == prefix)) {
                        const uint64_t q = mass(f[i], m);
                        if (q) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[255 - ((key[i] >> sh) & 255u)]), (unsigned long long)q);
                    }
                }
            });
            __syncthreads();
            p = pick_bin(hist, p.above, target, false, 0, &pick);
            prefix = (prefix << 8) | (uint32_t)(255 - p.bin);
        }
        thr = prefix > thr ? prefix : thr;
    }

    // last pass: count the kept tokens and draw among them
    const bool minp = a.log_min_p > -INFINITY;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    uint64_t kept = 0;
    visit<DT>(rowp, n, a.vec_ok, [&](int c, const float (&f)[8], const uint32_t (&key)[8]) {
        bool keep[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            keep[i] = valid(f[i]) && key[i] >= thr && (!minp || f[i] == m || f[i] - m >= a.log_min_p);
            kept += keep[i];
        }
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = f[i];
        if (a.inv_temperature > 0.f) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (keep[4 * k] || keep[4 * k + 1] || keep[4 * k + 2] || keep[4 * k + 3]) {
                    uint32_t ctr[4] = {(uint32_t)(2 * c + k), (uint32_t)row, (uint32_t)a.offset, (uint32_t)(a.offset >> 32)};
                    philox10(ctr, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[4 * k + i] = f[4 * k + i] * a.inv_temperature + gumbel_noise(ctr[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (keep[i] && v[i] > best) {  // strictly greater: the lowest index of equal keys wins inside a thread
                best = v[i];
                besti = 8 * c + i;
            }
        }
    });
    kept = block_sum(kept, redu);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(besti, off);
        if (ov > best || (ov == best && oi < besti)) {
            best = ov;
            besti = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        bestv[threadIdx.x >> 6] = best;
        besti_w[threadIdx.x >> 6] = besti;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kFW; ++w) {
            if (bestv[w] > best || (bestv[w] == best && besti_w[w] < besti)) {
                best = bestv[w];
                besti = besti_w[w];
            }
        }
        const int tok = besti == 0x7fffffff ? 0 : besti;  // (the max is always kept: only a kept-nothing row has none)
        a.out[row] = tok;
        if (a.kept) a.kept[row] = (int32_t)kept;
        if (a.logprobs) {
            const float lt = DT == HYD_F32 ? static_cast<const float*>(rowp)[tok] : h2f<DT>(static_cast<const uint16_t*>(rowp)[tok]);
            const double d = lt == m ? 0.0 : (double)lt - (double)m;
            a.logprobs[row] = (float)(d - (log((double)total) - 40.0 * 0.6931471805599453));
        }
    }
}

int launch_sample_filter(const FilterArgs& a, int dtype, hipStream_t s) {
    if (a.rows == 0) return 0;
    const dim3 grid((unsigned)a.rows), block(kFT);
    if (dtype == HYD_F16) hipLaunchKernelGGL((sample_filter_kernel<HYD_F16>), grid, block, 0, s, a);
    else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_filter_kernel<HYD_BF16>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sample_filter_kernel<HYD_F32>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
