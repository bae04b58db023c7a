// hyd_sample_tokens_penalized: sample_filter.hip's row (sample_select.h sample_row) over PENALISED logits -- repetition /
// presence / frequency penalties and a sparse logit bias (include/hydragen_hip.h) -- and
// hyd_token_bitmap_build, the presence bitmap of a prompt's token ids.
//
//   * Nothing of size [rows, n] exists.  What a row needs to turn (index, logit) into x lives in the workgroup's LDS, built
//     by a prologue:
//       ctx   the row's context bitmap, the OR of its row of every context bitmap (a shared prompt is ONE bitmap row for all
//             the rows below it): n / 8 bytes, 16 KB at n = 128256.  Rows wider than kCtxWords * 32 tokens keep it in global
//             memory and OR the levels' bytes at every read;
//       tab   an open-addressing table (kSlots keys, linear probing, LDS compare-and-swap) of the row's generated tokens with
//             their counts and of the bias ids with their list positions: at most HYD_SAMPLE_GEN_MAX + HYD_SAMPLE_BIAS_MAX
//             = 3072 of 4096 slots.  Counts are integer atomics: the table's CONTENT does not depend on the insertion order;
//       slow  one bit per 8-token chunk (folded modulo kSlowBits) that says "a token of this chunk may be in tab".
//   * Every pass maps a chunk before the select sees it.  A chunk with no ctx byte and no slow bit -- the bulk of the
//     vocabulary -- costs one LDS byte, one LDS bit and, for 16-bit rows, the fp32 keys.  A touched token is evaluated in
//     double from its logit and rounded once to fp32.
//   * x is an fp32 value even for 16-bit rows: the keys are the fp32 ones and the select runs 4 radix levels.
// 1024 threads per row as sample_filter.hip; LDS 70.4 KB per workgroup: two rows per CU (160 KB).
#include "sample_select.h"

namespace hyd {

namespace {

constexpr int kCtxWords = 8192;   // context bitmap words kept in LDS: rows of up to 262144 tokens
constexpr int kSlots = 4096;      // table slots (power of two)
constexpr int kSlowBits = 32768;  // chunk bits: exact up to 262144 tokens, folded beyond
constexpr int kEmpty = -1;
static_assert(HYD_SAMPLE_GEN_MAX + HYD_SAMPLE_BIAS_MAX <= kSlots * 3 / 4, "table load");
static_assert(HYD_SAMPLE_GEN_MAX < (1 << 16) && HYD_SAMPLE_BIAS_MAX < (1 << 15), "count | (bias position + 1) << 16");

__device__ __forceinline__ uint32_t slot_of(int v) { return ((uint32_t)v * 0x9E3779B1u) >> 20; }  // top 12 bits

struct PenaltyMap {
    const PenaltyArgs& a;
    const uint32_t* ctx;   // LDS, or null: read the levels in global memory
    const uint32_t* slow;  // LDS
    const int* keys;       // LDS
    const uint32_t* vals;  // LDS: count | (bias position + 1) << 16
    int row;

    __device__ __forceinline__ uint32_t ctx_byte(int c) const {
        if (ctx) return reinterpret_cast<const uint8_t*>(ctx)[c];
        uint32_t b = 0;
        for (int l = 0; l < a.n_ctx; ++l)
            b |= reinterpret_cast<const uint8_t*>(a.ctx[l] + (int64_t)(row / a.ctx_rpg[l]) * a.words)[c];
        return b;
    }
    __device__ __forceinline__ uint32_t find(int v) const {
        for (uint32_t h = slot_of(v);; h = (h + 1) & (kSlots - 1)) {
            const int k = keys[h];
            if (k == v) return vals[h];
            if (k == kEmpty) return 0;
        }
    }
    // the definition's three steps, in double, one rounding
    __device__ __forceinline__ float apply(float l, bool in_ctx, uint32_t val) const {
        const uint32_t cnt = val & 0xffffu, bpos = val >> 16;
        double x = (double)l;
        if (in_ctx || cnt) x = x * (x > 0.0 ? a.inv_rep : a.rep);  // (1 / r in double: 2^-53 relative, far below the fp32 rounding)
        if (cnt) x -= a.freq * (double)cnt + a.pres;
        if (bpos && bpos <= (uint32_t)a.n_bias) x += (double)a.bias_values[bpos - 1];  // (repeated ids OR their positions)
        return (float)x;
    }
    __device__ __forceinline__ float one(int tok, float l) const {
        const int c = tok >> 3;
        const bool in_ctx = (ctx_byte(c) >> (tok & 7)) & 1u;
        const bool s = (slow[(c & (kSlowBits - 1)) >> 5] >> (c & 31)) & 1u;
        const uint32_t val = s ? find(tok) : 0u;
        return (in_ctx || val) ? apply(l, in_ctx, val) : l;
    }
};

// 16-bit rows come with 16-bit keys: every key becomes the fp32 one.  fp32 rows: only the touched tokens' keys change.
template <int DT>
struct PenaltyMapT : PenaltyMap {
    __device__ __forceinline__ void chunk(int c, float (&f)[8], uint32_t (&k)[8]) const {
        const uint32_t cb = ctx_byte(c);
        const bool s = (slow[(c & (kSlowBits - 1)) >> 5] >> (c & 31)) & 1u;
        if (cb || s) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool in_ctx = (cb >> i) & 1u;
                const uint32_t val = s ? find(8 * c + i) : 0u;
                if (in_ctx || val) {
                    f[i] = apply(f[i], in_ctx, val);
                    if (DT == HYD_F32) k[i] = key32(__builtin_bit_cast(uint32_t, f[i]));
                }
            }
        }
        if (DT != HYD_F32) {
#pragma unroll
            for (int i = 0; i < 8; ++i) k[i] = key32(__builtin_bit_cast(uint32_t, f[i]));
        }
    }
};

}  // namespace

template <int DT>
__global__ __launch_bounds__(1024) void sample_penalty_kernel(const PenaltyArgs a) {
    __shared__ uint32_t ctx[kCtxWords];
    __shared__ uint32_t slow[kSlowBits / 32];
    __shared__ int keys[kSlots];
    __shared__ uint32_t vals[kSlots];
    const int row = blockIdx.x, t = threadIdx.x;
    const bool ctx_lds = a.words <= kCtxWords;

    // prologue: the row's context bitmap (plain stores: one thread per word), an empty table
    if (ctx_lds) {
        for (int w = t; w < a.words; w += kFT) {
            uint32_t b = 0;
            for (int l = 0; l < a.n_ctx; ++l) b |= a.ctx[l][(int64_t)(row / a.ctx_rpg[l]) * a.words + w];
            ctx[w] = b;
        }
    }
    for (int i = t; i < kSlowBits / 32; i += kFT) slow[i] = 0;
    for (int i = t; i < kSlots; i += kFT) {
        keys[i] = kEmpty;
        vals[i] = 0;
    }
    __syncthreads();
    int glen = 0;
    if (a.gen) {
        glen = a.gen_len[row];
        glen = glen < 0 ? 0 : (glen > a.gen_stride ? a.gen_stride : glen);
    }
    // generated tokens (count + 1) and bias ids (position + 1 in the high half): ids outside [0, n) are ignored
    for (int i = t; i < glen + a.n_bias; i += kFT) {
        const bool is_gen = i < glen;
        const int64_t v64 = is_gen ? (int64_t)a.gen[(int64_t)row * a.gen_stride + i] : a.bias_ids[i - glen];
        if (v64 < 0 || v64 >= a.f.n) continue;
        const int v = (int)v64;
        uint32_t h = slot_of(v);
        for (;; h = (h + 1) & (kSlots - 1)) {
            const int old = atomicCAS(&keys[h], kEmpty, v);
            if (old == kEmpty || old == v) break;
        }
        if (is_gen) atomicAdd(&vals[h], 1u);
        else atomicOr(&vals[h], (uint32_t)(i - glen + 1) << 16);
        const int c = v >> 3;
        atomicOr(&slow[(c & (kSlowBits - 1)) >> 5], 1u << (c & 31));
    }
    __syncthreads();

    PenaltyMapT<DT> map{{a, ctx_lds ? ctx : nullptr, slow, keys, vals, row}};
    const int tok = sample_row<DT, 32>(a.f, map);
    if (t == 0 && a.append_out) {  // (every read of gen / gen_len above is behind sample_row's barriers)
        const int len = a.gen_len[row];
        if (len >= 0 && len < a.gen_stride) a.gen[(int64_t)row * a.gen_stride + len] = tok;
        a.gen_len[row] = len + 1;
    }
}

int launch_sample_penalty(const PenaltyArgs& a, int dtype, hipStream_t s) {
    if (a.f.rows == 0) return 0;
    const dim3 grid((unsigned)a.f.rows), block(kFT);
    if (dtype == HYD_F16) hipLaunchKernelGGL((sample_penalty_kernel<HYD_F16>), grid, block, 0, s, a);
    else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_penalty_kernel<HYD_BF16>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sample_penalty_kernel<HYD_F32>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

// bits[g, v / 32] |= 1 << (v % 32) for the ids of group g: 256 threads per (group, 1024-id slice), one atomic OR per id
__global__ __launch_bounds__(256) void token_bitmap_kernel(const BitmapArgs a) {
    const int g = blockIdx.y;
    const int64_t len = a.lens ? (a.lens[g] < a.L ? a.lens[g] : a.L) : a.L;
    const int64_t j0 = (int64_t)blockIdx.x * 1024;  // (64-bit: L may sit within 1024 of INT32_MAX)
    for (int64_t j = j0 + threadIdx.x; j < j0 + 1024 && j < len; j += 256) {
        const int64_t v = a.ids[(int64_t)g * a.id_stride + j];
        if (v >= 0 && v < a.n) atomicOr(&a.bits[(int64_t)g * a.words + (v >> 5)], 1u << (v & 31));
    }
}

int launch_token_bitmap(const BitmapArgs& a, hipStream_t s) {
    if (a.groups == 0 || a.L == 0) return 0;
    const dim3 grid((unsigned)((a.L + 1023) / 1024), (unsigned)a.groups), block(256);
    hipLaunchKernelGGL(token_bitmap_kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
