// The penalty map of sample_penalty.hip -- what turns (index, logit) into the penalised logit x from tables in the workgroup's
// LDS -- and the prologue that builds those tables, shared with sample_constrain.hip (MOVED here from sample_penalty.hip, not
// copied: that file's kernels compile to the same instructions as before the move).  sample_penalty.hip's header comment
// describes ctx / tab / slow.
#pragma once
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

// The three penalties of a row of hyd_sample_tokens_rows, block-uniform: the row's fp32 entries widened to double exactly (so
// that a per-row f behaves bit for bit like the scalar (double)f) and sanitised -- a repetition penalty that is <= 0 or not
// finite -> 1, a frequency / presence penalty that is not finite -> 0 --, inv_rep = 1.0 / rep (one IEEE fp64 division per row:
// the host's expression).  An array that is not given leaves the launch's scalar.
struct PenVals {
    double rep, inv_rep, freq, pres;
};
struct ArgPen {  // the scalar launches: the argument block's (these are never read)
    static constexpr double rep = 0, inv_rep = 0, freq = 0, pres = 0;
};
__device__ __forceinline__ double uniform_d(double x) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    return __builtin_bit_cast(double, (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u) |
                                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32)) << 32);
}
__device__ __forceinline__ PenVals pen_vals(const PenaltyArgs& a, const RowParams& r, int row) {
    PenVals v{a.rep, a.inv_rep, a.freq, a.pres};
    if (r.rep) {
        const float f = r.rep[row];
        v.rep = uniform_d((f > 0.f && f < INFINITY) ? (double)f : 1.0);
        v.inv_rep = uniform_d(1.0 / v.rep);
    }
    if (r.freq) {
        const float f = r.freq[row];
        v.freq = uniform_d(fabsf(f) < INFINITY ? (double)f : 0.0);
    }
    if (r.pres) {
        const float f = r.pres[row];
        v.pres = uniform_d(fabsf(f) < INFINITY ? (double)f : 0.0);
    }
    return v;
}

// Pen: ArgPen, or the row's PenVals (pen_vals)
template <typename Pen>
struct PenaltyMapP {
    const PenaltyArgs& a;
    const uint32_t* ctx;   // LDS, or null: read the levels in global memory
    const uint32_t* slow;  // LDS
    const int* keys;       // LDS
    const uint32_t* vals;  // LDS: count | (bias position + 1) << 16
    int row;
    Pen pen;
    static constexpr bool kRows = !__is_same(Pen, ArgPen);  // (constant conditions below: the other arm is not compiled)

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
        if (in_ctx || cnt) x = x * (x > 0.0 ? (kRows ? pen.inv_rep : a.inv_rep) : (kRows ? pen.rep : a.rep));  // (1 / r in double: 2^-53 relative, far below the fp32 rounding)
        if (cnt) x -= (kRows ? pen.freq : a.freq) * (double)cnt + (kRows ? pen.pres : a.pres);
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
using PenaltyMap = PenaltyMapP<ArgPen>;
template <int DT, typename Pen = ArgPen>
struct PenaltyMapT : PenaltyMapP<Pen> {
    __device__ __forceinline__ void chunk(int c, float (&f)[8], uint32_t (&k)[8]) const {
        const uint32_t cb = this->ctx_byte(c);
        const uint32_t* slow = this->slow;
        const bool s = (slow[(c & (kSlowBits - 1)) >> 5] >> (c & 31)) & 1u;
        if (cb || s) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool in_ctx = (cb >> i) & 1u;
                const uint32_t val = s ? this->find(8 * c + i) : 0u;
                if (in_ctx || val) {
                    f[i] = this->apply(f[i], in_ctx, val);
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

// The prologue of a penalised row (every thread of workgroup blockIdx.x): the row's context bitmap (when it fits the LDS
// copy), an empty table, then the generated tokens and the bias ids.  Ends behind a barrier.
__device__ __forceinline__ void penalty_tables(const PenaltyArgs& a, const int row, const int t, const bool ctx_lds, uint32_t (&ctx)[kCtxWords],
                                               uint32_t (&slow)[kSlowBits / 32], int (&keys)[kSlots], uint32_t (&vals)[kSlots]) {

    // the row's context bitmap (plain stores: one thread per word), an empty table
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
}

// after the draw, thread 0: the token goes behind the row's list of generated tokens (append_out)
__device__ __forceinline__ void penalty_append(const PenaltyArgs& a, int row, int tok) {
    const int len = a.gen_len[row];
    if (len >= 0 && len < a.gen_stride) a.gen[(int64_t)row * a.gen_stride + len] = tok;
    a.gen_len[row] = len + 1;
}

}  // namespace

}  // namespace hyd
