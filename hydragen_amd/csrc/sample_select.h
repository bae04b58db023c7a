// The vocabulary-row machinery of sample_penalty.hip: sample_filter.hip's helpers (Philox / Gumbel noise of sample_kernel,
// order-preserving keys, 8-element chunk loads, block reductions, fixed-point masses, the 256-bin select) and its kernel body as
// a function of a Map that rewrites every chunk before the select sees it (sample_row).  COPIED from sample_filter.hip, not
// moved: that file's gfx950 assembly is pinned by tests/test_scoring.py, so it keeps its own text.  A change to the sampling
// rules is made in both; tests/test_sampling_penalties_gpu.py holds them bit-equal on unpenalised rows.
#pragma once
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

// What a sampling kernel does to a row before the select sees it.  chunk(c, f, key): rewrites the 8 logits of chunk c and
// their keys (keys of KB bits); one(tok, l): the same map for a single token.  NoMap: the logits as they are.
struct NoMap {
    __device__ __forceinline__ void chunk(int, float (&)[8], uint32_t (&)[8]) const {}
    __device__ __forceinline__ float one(int, float l) const { return l; }
};
template <int DT, typename Map, typename F>
__device__ __forceinline__ void visit_mapped(const void* row, int n, int vec, const Map& map, F&& fn) {
    visit<DT>(row, n, vec, [&](int c, float (&f)[8], uint32_t (&k)[8]) {
        map.chunk(c, f, k);
        fn(c, f, k);
    });
}

// One row of hyd_sample_tokens_filtered (workgroup blockIdx.x, 1024 threads) over map(logits), keys of KB bits.  Returns the
// token on thread 0 (every thread of a row without a valid logit: 0), -1 on the others.
template <int DT, int KB, typename Map>
__device__ __forceinline__ int sample_row(const FilterArgs& a, const Map& map) {
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
    visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int, const float (&f)[8], const uint32_t (&)[8]) {
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
        return 0;
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
        visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int, const float (&f)[8], const uint32_t (&)[8]) {
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
            visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
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
        visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
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
            visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
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
    visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int c, const float (&f)[8], const uint32_t (&key)[8]) {
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
            const float lt = map.one(tok, DT == HYD_F32 ? static_cast<const float*>(rowp)[tok] : h2f<DT>(static_cast<const uint16_t*>(rowp)[tok]));
            const double d = lt == m ? 0.0 : (double)lt - (double)m;
            a.logprobs[row] = (float)(d - (log((double)total) - 40.0 * 0.6931471805599453));
        }
        return tok;
    }
    return -1;
}

}  // namespace

}  // namespace hyd
