// sample_row<DT, KB, Map>: one row of the filtered sampler -- top-k / top-p / min-p cuts, the Gumbel draw and the token's log-prob
// (sample_filter.hip's header comment describes the algorithm) -- over map(logits), a Map that rewrites every
// chunk before the select sees it: the kernel body of sample_penalty.hip and sample_constrain.hip, on the row primitives of
// vocab_row.h.  (sample_filter_kernel spells the same passes out with no map: sharing the helpers moved no instruction of it, making
// it sample_row<DT, KB>(a, NoMap{}) rescheduled it and cost fp32 rows about half a percent, profiles/vocab_row_header.md.  A
// change to the passes is made in both; tests/test_sampling_penalties_gpu.py holds them bit-equal.  Per-row values -- RowVals
// below -- are no change to the passes: sample_rows.hip instantiates sample_row with them, sample_filter.hip has no such form.)
#pragma once
#include "vocab_row.h"

namespace hyd {

namespace {

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

// The values a row samples with, block-uniform locals read once at the top of the row.  The scalar launches (NoRowParams) take
// them from the argument block as the host prepared them.  hyd_sample_tokens_rows (RowParams) replaces each one whose array is
// given by the row's own entry, sanitised (no host can check device values; none of them ever forms an address) and prepared
// with the host's expressions (api_logits.hip fill_filter_args):
//   temperature  NaN or < 0 -> 0;  inv_temperature = T > 0 ? 1.0f / T : 0
//   top_k        < 0 -> 0;  >= n -> 0 (no cut)
//   top_p        outside (0, 1] or NaN -> 1
//   min_p        outside [0, 1] or NaN -> 0;  log_min_p = min_p > 0 ? (float)log((double)min_p) : -inf
//   seed         the row draws as ROW 0 of a launch with that seed: Philox counter (chunk, 0, offset lo, offset hi), key seed[row]
struct RowVals {
    float inv_temperature;
    int32_t top_k;
    float top_p, log_min_p;
    uint64_t seed;
    uint32_t noise_row;  // the Philox counter's second word
};
__device__ __forceinline__ float uniform_f(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
__device__ __forceinline__ RowVals row_vals(const FilterArgs& a, const RowParams& r, int row) {
    RowVals v{a.inv_temperature, a.top_k, a.top_p, a.log_min_p, a.seed, (uint32_t)row};
    if (r.temperature) {
        const float t = r.temperature[row];
        v.inv_temperature = uniform_f(t > 0.f ? 1.0f / t : 0.f);  // (uniform_f: computed by the vector unit, kept in a scalar register)
    }
    if (r.top_k) {
        const int k = __builtin_amdgcn_readfirstlane(r.top_k[row]);
        v.top_k = (k > 0 && k < a.n) ? k : 0;
    }
    if (r.top_p) {
        const float p = uniform_f(r.top_p[row]);
        v.top_p = (p > 0.f && p <= 1.f) ? p : 1.f;
    }
    if (r.min_p) {
        const float p = r.min_p[row];
        v.log_min_p = uniform_f((p > 0.f && p <= 1.f) ? (float)log((double)p) : -INFINITY);
    }
    if (r.seed) {
        const uint64_t s = r.seed[row];
        v.seed = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s) |
                 (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(s >> 32)) << 32;
        v.noise_row = 0;
    }
    return v;
}
template <typename Rows>
constexpr bool kPerRow = false;
template <>
constexpr bool kPerRow<RowParams> = true;
// a value of the row: its own (hyd_sample_tokens_rows), else the argument block's, read where the scalar kernels always read it
// (a constant condition: the other arm is not compiled)
#define HYD_ROW(field) (kPerRow<Rows> ? rv.field : a.field)

// One row of hyd_sample_tokens_filtered (workgroup blockIdx.x, 1024 threads) over map(logits), keys of KB bits.  Returns the
// token on thread 0 (every thread of a row without a valid logit: 0), -1 on the others.  rows: NoRowParams, or the per-row
// values of hyd_sample_tokens_rows (an instantiation of its own: the scalar one compiles as it did without them).
template <int DT, int KB, typename Map, typename Rows = NoRowParams>
__device__ __forceinline__ int sample_row(const FilterArgs& a, const Map& map, const Rows& rows = Rows{}) {
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
    RowVals rv;  // (the scalar launches never read it)
    if constexpr (kPerRow<Rows>) rv = row_vals(a, rows, row);

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
    const bool topk = HYD_ROW(top_k) > 0 && (uint64_t)HYD_ROW(top_k) < nvalid;
    const bool topp = HYD_ROW(top_p) < 1.0f;

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
        const uint64_t k = (uint64_t)HYD_ROW(top_k);
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
        const uint64_t target = (uint64_t)ceil((double)HYD_ROW(top_p) * (double)tot1);
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
    const bool minp = HYD_ROW(log_min_p) > -INFINITY;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    uint64_t kept = 0;
    visit_mapped<DT>(rowp, n, a.vec_ok, map, [&](int c, const float (&f)[8], const uint32_t (&key)[8]) {
        bool keep[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            keep[i] = valid(f[i]) && key[i] >= thr && (!minp || f[i] == m || f[i] - m >= HYD_ROW(log_min_p));
            kept += keep[i];
        }
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = f[i];
        if (HYD_ROW(inv_temperature) > 0.f) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (keep[4 * k] || keep[4 * k + 1] || keep[4 * k + 2] || keep[4 * k + 3]) {
                    uint32_t ctr[4] = {(uint32_t)(2 * c + k), (kPerRow<Rows> ? rv.noise_row : (uint32_t)row), (uint32_t)a.offset, (uint32_t)(a.offset >> 32)};
                    philox10(ctr, (uint32_t)HYD_ROW(seed), (uint32_t)(HYD_ROW(seed) >> 32));
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[4 * k + i] = f[4 * k + i] * HYD_ROW(inv_temperature) + gumbel_noise(ctr[i]);
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
            a.logprobs[row] = logprob_of(lt, m, (double)total);  // (the same value either way; converted here, this body compiles as before)
        }
        return tok;
    }
    return -1;
}

#undef HYD_ROW

}  // namespace

}  // namespace hyd
