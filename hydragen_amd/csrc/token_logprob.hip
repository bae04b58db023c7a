// Log-probabilities of GIVEN tokens, greedy flags and the top-N alternatives of every row, one workgroup per row
// (hyd_token_logprobs, include/hydragen_hip.h).
//
//   * logprob = l_t - m - ln sum exp(l - m) over the valid logits (not NaN, not -inf), with sample_filter.hip's fixed-point
//     masses floor(exp(l - m) 2^40) summed in u64 and its closing expression: the same bits as hyd_sample_tokens_filtered's
//     log-prob of that token, for every run and every launch geometry.
//   * greedy = t is the lowest-index maximum of the valid logits (torch.argmax's tie rule, hyd_sample_tokens at T = 0).
//   * top-N (N <= HYD_TOP_LOGPROBS_MAX): the N largest valid logits by (value descending, index ascending).  Every element is
//     ranked by a unique composite (order-preserving key of its bits, then its index), so the N-th is one threshold.  The
//     threshold is narrowed until few enough candidates remain to sit in LDS (kCap), then the candidates are gathered and
//     ranked against each other:
//       1. the distance-to-max histogram of sample_filter.hip (bins of 1/8, built during the sum pass): the bin holding the
//          N-th largest value; usually that bin and the ones above it hold a few dozen logits -> gather them;
//       2. otherwise 8-bit radix levels over the key inside that bin (2 for 16-bit logits, 4 for fp32) -> the N-th key;
//       3. otherwise (more than kCap logits tie at the N-th key) 8-bit levels over the index among the ties -> the cut.
// Mapping: 1024 threads; thread t owns the 8-element chunks t + 1024 j (16-byte loads when the row allows), read kU chunks at a
// time so that several loads are in flight.  Every pass re-reads the row (64-512 KB): the passes after the first hit L2 /
// MALL.  N = 0 is its own instantiation: no histogram, no LDS beyond the reductions.
#include "vocab_row.h"  // keys, masses, bins, block_sum, pick_bin, logprob_of: the samplers' own

namespace hyd {

namespace {

constexpr int kU = 4;       // chunks loaded per thread before any is used
constexpr int kCap = 1024;  // LDS candidates of the top-N gather

// Raw words of one 8-element chunk: 16-bit logits as 4 packed words (w[4..7] unused), fp32 as 8 words; past n: -inf.
template <int DT>
__device__ __forceinline__ void load_chunk(const void* row, int c, int n, int vec, uint32_t (&w)[8]) {
    if constexpr (DT == HYD_F32) {
        const float* r = static_cast<const float*>(row);
        if (vec && 8 * c + 8 <= n) {
            const u32x4 u0 = reinterpret_cast<const u32x4*>(r)[2 * c], u1 = reinterpret_cast<const u32x4*>(r)[2 * c + 1];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = u0[i];
                w[4 + i] = u1[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = 8 * c + i < n ? __builtin_bit_cast(uint32_t, r[8 * c + i]) : 0xff800000u;
        }
    } else {
        const uint16_t* r = static_cast<const uint16_t*>(row);
        if (vec && 8 * c + 8 <= n) {
            const u32x4 u = reinterpret_cast<const u32x4*>(r)[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = u[i];
        } else {
            const uint32_t pad = DT == HYD_F16 ? 0xfc00u : 0xff80u;
            uint32_t h[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = 8 * c + i < n ? r[8 * c + i] : pad;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = h[2 * i] | h[2 * i + 1] << 16;
        }
#pragma unroll
        for (int i = 4; i < 8; ++i) w[i] = 0;
    }
}
template <int DT>
__device__ __forceinline__ void decode_chunk(const uint32_t (&w)[8], float (&f)[8], uint32_t (&k)[8]) {
    if constexpr (DT == HYD_F32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f[i] = __builtin_bit_cast(float, w[i]);
            k[i] = key32(w[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t lo = w[i] & 0xffffu, hi = w[i] >> 16;
            f[2 * i] = h2f<DT>(lo);
            f[2 * i + 1] = h2f<DT>(hi);
            k[2 * i] = key16(lo);
            k[2 * i + 1] = key16(hi);
        }
    }
}

// Calls fn(first index, f[8], key[8]) for every chunk this thread owns, in increasing index order, kU loads ahead.
template <int DT, typename F>
__device__ __forceinline__ void visit_ahead(const void* row, int n, int vec, F&& fn) {
    const int nchunk = (n + 7) >> 3;
    for (int c0 = threadIdx.x; c0 < nchunk; c0 += kU * kFT) {
        uint32_t w[kU][8];
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (c0 + u * kFT < nchunk) load_chunk<DT>(row, c0 + u * kFT, n, vec, w[u]);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (c0 + u * kFT < nchunk) {
                float f[8];
                uint32_t k[8];
                decode_chunk<DT>(w[u], f, k);
                fn(8 * (c0 + u * kFT), f, k);
            }
        }
    }
}

// (value, index) with the larger value, the lower index on equal values (valid values only: no NaN reaches here)
__device__ __forceinline__ void better(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

}  // namespace

template <int DT, bool TOPN>
__global__ __launch_bounds__(1024) void token_logprob_kernel(const TokenLogprobArgs a) {
    constexpr int KB = DT == HYD_F32 ? 32 : 16;  // key bits
    __shared__ uint64_t redu[kFW];
    __shared__ float bestv[kFW];
    __shared__ int besti_w[kFW];
    const int64_t row = a.row0 + blockIdx.x;
    const int n = a.n;
    const int esz = DT == HYD_F32 ? 4 : 2;
    const void* rowp = static_cast<const char*>(a.logits) + row * a.row_stride * esz;

    // pass 1: max, its lowest index, and the number of valid logits
    float best = -INFINITY;
    int besti = 0x7fffffff;
    uint64_t nvalid = 0;
    visit_ahead<DT>(rowp, n, a.vec_ok, [&](int i0, const float (&f)[8], const uint32_t (&)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (valid(f[i])) {
                ++nvalid;
                if (f[i] > best) {  // strictly greater: the lowest index of equal values inside a thread (valid: f > -inf)
                    best = f[i];
                    besti = i0 + i;
                }
            }
        }
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) better(best, besti, __shfl_xor(best, off), __shfl_xor(besti, off));
    if ((threadIdx.x & 63) == 0) {
        bestv[threadIdx.x >> 6] = best;
        besti_w[threadIdx.x >> 6] = besti;
    }
    __syncthreads();
    best = bestv[0];
    besti = besti_w[0];
#pragma unroll
    for (int w = 1; w < kFW; ++w) better(best, besti, bestv[w], besti_w[w]);
    nvalid = block_sum(nvalid, redu);  // (its barriers also retire bestv / besti_w)
    const float m = best;
    const int64_t t = a.targets[row];
    const bool tin = t >= 0 && t < n;
    const int N = TOPN ? a.top_n : 0;
    if (nvalid == 0) {
        if (threadIdx.x == 0) {
            a.logprobs[row] = __builtin_nanf("");
            a.greedy[row] = 0;
        }
        if (TOPN && (int)threadIdx.x < N) {
            a.top_ids[row * N + threadIdx.x] = -1;
            a.top_logprobs[row * N + threadIdx.x] = -INFINITY;
        }
        return;
    }

    // pass 2: the softmax denominator; with top-N, the distance-to-max histogram of the first select level
    __shared__ uint64_t hist[TOPN ? 256 : 1];
    __shared__ Pick pick;
    __shared__ uint64_t pick_at;
    const bool select = TOPN && nvalid > (uint64_t)N;  // fewer valid logits than N: every valid logit is a candidate
    if (select) {
        for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
        __syncthreads();
    }
    uint64_t total = 0;
    visit_ahead<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (valid(f[i])) {
                total += mass(f[i], m);
                if (select) {
                    const int b = bin0(f[i], m);
                    if (b < 255) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[b]), 1ull);
                }
            }
        }
    });
    total = block_sum(total, redu);  // (its barriers also order the histogram before the pick)

    if (threadIdx.x == 0) {
        float lp = __builtin_nanf("");
        if (tin) {
            const float lt = DT == HYD_F32 ? static_cast<const float*>(rowp)[t] : h2f<DT>(static_cast<const uint16_t*>(rowp)[t]);
            lp = logprob_of(lt, m, total);
        }
        a.logprobs[row] = lp;
        a.greedy[row] = tin && t == (int64_t)besti;
    }
    if constexpr (TOPN) {
        // candidates: mode 0 every valid logit; 1 bin0 <= b; 2 key >= thr; 3 key > thr, or key == thr and index <= icut
        int mode = 0, b = 255;
        uint32_t thr = 0, icut = 0;
        if (select) {
            Pick p = pick_bin(hist, 0, (uint64_t)N, true, nvalid, &pick, &pick_at);
            b = p.bin;
            mode = 1;
            if (p.above + pick_at > (uint64_t)kCap) {
                uint32_t prefix = 0;
#pragma unroll
                for (int lvl = 0; lvl < KB / 8; ++lvl) {
                    for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
                    __syncthreads();
                    const int sh = KB - 8 * (lvl + 1);
                    visit_ahead<DT>(rowp, n, a.vec_ok, [&](int, const float (&f)[8], const uint32_t (&key)[8]) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            if (valid(f[i]) && bin0(f[i], m) == b && (lvl == 0 || (key[i] >> (sh + 8)) == prefix))
                                atomicAdd(reinterpret_cast<unsigned long long*>(&hist[255 - ((key[i] >> sh) & 255u)]), 1ull);
                        }
                    });
                    __syncthreads();
                    p = pick_bin(hist, p.above, (uint64_t)N, false, 0, &pick, &pick_at);
                    prefix = (prefix << 8) | (uint32_t)(255 - p.bin);
                }
                thr = prefix;
                mode = 2;
                if (p.above + pick_at > (uint64_t)kCap) {  // p.above logits above thr, pick_at tied at it: the lowest indices win
                    const uint64_t need = (uint64_t)N - p.above;
                    uint64_t cum = 0;
                    uint32_t ip = 0;
#pragma unroll
                    for (int lvl = 0; lvl < 3; ++lvl) {  // indices < 2^22 <= 2^24
                        for (int i = threadIdx.x; i < 256; i += kFT) hist[i] = 0;
                        __syncthreads();
                        const int sh = 16 - 8 * lvl;
                        visit_ahead<DT>(rowp, n, a.vec_ok, [&](int i0, const float (&f)[8], const uint32_t (&key)[8]) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                const uint32_t idx = (uint32_t)(i0 + i);
                                if (valid(f[i]) && key[i] == thr && (lvl == 0 || (idx >> (sh + 8)) == ip))
                                    atomicAdd(reinterpret_cast<unsigned long long*>(&hist[(idx >> sh) & 255u]), 1ull);
                            }
                        });
                        __syncthreads();
                        const Pick q = pick_bin(hist, cum, need, false, 0, &pick, &pick_at);
                        cum = q.above;
                        ip = (ip << 8) | (uint32_t)q.bin;
                    }
                    icut = ip;
                    mode = 3;
                }
            }
        }
        // gather the candidates (at most kCap) into LDS, then rank them by (key desc, index asc): the composite is unique
        __shared__ uint32_t ckey[kCap];
        __shared__ int cidx[kCap];
        __shared__ float cval[kCap];
        __shared__ int ccount;
        if (threadIdx.x == 0) ccount = 0;
        __syncthreads();
        visit_ahead<DT>(rowp, n, a.vec_ok, [&](int i0, const float (&f)[8], const uint32_t (&key)[8]) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                bool take = valid(f[i]);
                if (mode == 1) take = take && bin0(f[i], m) <= b;
                else if (mode == 2) take = take && key[i] >= thr;
                else if (mode == 3) take = take && (key[i] > thr || (key[i] == thr && (uint32_t)(i0 + i) <= icut));
                if (take) {
                    const int s = atomicAdd(&ccount, 1);
                    if (s < kCap) {  // (always: the selection above bounds the count)
                        ckey[s] = key[i];
                        cidx[s] = i0 + i;
                        cval[s] = f[i];
                    }
                }
            }
        });
        __syncthreads();
        const int cnt = ccount < kCap ? ccount : kCap;
        for (int s = threadIdx.x; s < cnt; s += kFT) {
            const uint32_t ks = ckey[s];
            const int is = cidx[s];
            int rank = 0;
            for (int j = 0; j < cnt && rank < N; ++j) rank += ckey[j] > ks || (ckey[j] == ks && cidx[j] < is);
            if (rank < N) {
                a.top_ids[row * N + rank] = is;
                a.top_logprobs[row * N + rank] = logprob_of(cval[s], m, total);
            }
        }
        for (int r = cnt + (int)threadIdx.x; r < N; r += kFT) {  // fewer valid logits than N
            a.top_ids[row * N + r] = -1;
            a.top_logprobs[row * N + r] = -INFINITY;
        }
    }
}

int launch_token_logprob(const TokenLogprobArgs& args, int dtype, hipStream_t s) {
    constexpr int64_t kRowsPerLaunch = 1 << 20;  // grid x stays far below 2^31 / 1024 threads
    for (int64_t r0 = 0; r0 < args.rows; r0 += kRowsPerLaunch) {
        TokenLogprobArgs a = args;
        a.row0 = r0;
        const int64_t rows = args.rows - r0 < kRowsPerLaunch ? args.rows - r0 : kRowsPerLaunch;
        const dim3 grid((unsigned)rows), block(kFT);
        const bool topn = a.top_n > 0;
        if (dtype == HYD_F16) {
            if (topn) hipLaunchKernelGGL((token_logprob_kernel<HYD_F16, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((token_logprob_kernel<HYD_F16, false>), grid, block, 0, s, a);
        } else if (dtype == HYD_BF16) {
            if (topn) hipLaunchKernelGGL((token_logprob_kernel<HYD_BF16, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((token_logprob_kernel<HYD_BF16, false>), grid, block, 0, s, a);
        } else {
            if (topn) hipLaunchKernelGGL((token_logprob_kernel<HYD_F32, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((token_logprob_kernel<HYD_F32, false>), grid, block, 0, s, a);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace hyd
