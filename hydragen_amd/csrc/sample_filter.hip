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
// The helpers are vocab_row.h's (through sample_select.h); the kernel body below is also sample_select.h's sample_row, there as a
// template over a logit map: a change to the passes is made in both (why: sample_select.h's header comment).
#include "sample_select.h"

namespace hyd {

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
