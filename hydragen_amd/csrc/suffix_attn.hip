// Suffix pass (K2 + K3 of SURVEY.md, with K4/K5 fused into the epilogue): every query row of
// sequence b against the first seq_len[b] keys of b's own (unique) K/V.  ~1 flop/byte: this is an
// HBM-bandwidth kernel, so it is built around wide coalesced loads and many bytes in flight, not MFMA.
//
// Replaces /root/reference/hydragen/flash.py:163-281 flash_attention_seqlen
//   (= hydragen/xformers_stuff.py:189-428 _fwd_kernel_splitK + hydragen/flash.py:76-160 _splitK_reduce)
// and, when partials are passed, hydragen/attention.py:352 combine_lse (:21-43 semantics, N partials).
//
// Mapping (wave64): a "unit" is one (sequence b, kv head).  D/8 lanes cover one key row with a 16-byte
// load each, so one wave instruction fetches 64/(D/8) consecutive keys (4 at D=128).  WPU waves share a
// unit (key iterations interleaved across them); 4/WPU units per 256-thread workgroup, consecutive
// waves = consecutive kv heads of the same sequence, i.e. neighbouring 2*D-byte pieces of the same token
// rows.  q.k partial dot products use v_dot2 and are reduced across the D/8 lanes with DPP adds; each
// lane group runs its own online softmax over its keys; groups, then waves, are merged at the end.
// The decode shape with one query row per kv head takes the token-row kernel instead (suffix_rows.h: body and launcher, shared
// with the fp8 caches' kernel of suffix_attn_fp8.hip); the online-softmax step of a key chunk is suffix_common.h's softmax_step.
#include <type_traits>

#include <cstdlib>
#include <cstring>

#include "suffix_unit.h"

namespace hyd {

// The token-row kernel on 16-bit caches: the body, its measurements and its launcher are in suffix_rows.h (shared with the fp8
// caches' kernel of suffix_attn_fp8.hip).
struct RowsCache16 {
    using elem = uint16_t;  // strides count 16-bit elements
    using vec = u32x4;      // 8 elements: one dwordx4 request
    static constexpr bool kScaled = false;
    template <typename T>
    static __device__ __forceinline__ u32x4 k_dot2(const u32x4& k) { return k; }
    template <typename T>
    static __device__ __forceinline__ void v_f32(const u32x4& v, float (&f)[8]) { widen8<T>(v, f); }
};
// NARROW: cache rows of a.kv_dim < D elements per head (suffix_rows.h)
template <typename T, int D, int UT, int NPRE, int TS = 1, bool NARROW = false>
__global__ __launch_bounds__(256, 4) void suffix_attn_rows_kernel(const SuffixArgs a) {
    suffix_rows_body<T, D, UT, NPRE, TS, RowsCache16, NARROW>(a, nullptr, nullptr);
}

template <typename T, int D, int R>
static int launch_suffix_r(const SuffixArgs& a, hipStream_t s) {
    // Shapes-only choice: spread one unit over the 4 waves of a workgroup when there are too few
    // units to fill 256 CUs with one wave each (C3-like shapes).
    const int row_chunks = (a.rows + R - 1) / R;
    const bool few_units = (int64_t)a.units * row_chunks < 2 * 256 * 4 && a.kv_len >= 64;
    if (few_units) {
        dim3 grid(a.B, a.Hkv, row_chunks);
        hipLaunchKernelGGL((suffix_attn_kernel<T, D, R, 4>), grid, dim3(256), 0, s, a);
    } else {
        dim3 grid(a.B, (a.Hkv + 3) / 4, row_chunks);
        if constexpr (R == 1) {
            if (a.n_pre == 2) {
                hipLaunchKernelGGL((suffix_attn_kernel<T, D, R, 1, 2>), grid, dim3(256), 0, s, a);
                return (int)hipGetLastError();
            }
        }
        if constexpr (R == 1) {
            if (a.kv_len > 1024) {  // long caches: rotated requests (see PIPE in the kernel)
                hipLaunchKernelGGL((suffix_attn_kernel<T, D, R, 1, 1, 4, 6, 1>), grid, dim3(256), 0, s, a);
                return (int)hipGetLastError();
            }
        }
        hipLaunchKernelGGL((suffix_attn_kernel<T, D, R, 1>), grid, dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

// packed path: one query row per unit (nq == 1, Hq == Hkv), 32-bit offsets inside a sequence's cache
static bool suffix_packed_eligible(const SuffixArgs& a, int D) {
    const int hpw = 64 / (D / 8);
    return a.rows == 1 && a.nq == 1 && a.g == 1 && a.Hkv >= hpw && D == 128 && cache_span_fits_32bit(a, 2);
}

template <typename T, int D>
static int launch_suffix_t(const SuffixArgs& a0, hipStream_t s) {
    SuffixArgs a = a0;
    if (a.kv_dim) {
        // narrow unique caches (hyd_suffix_params.kv_dim): the token-row kernel whenever its shapes hold -- the D-wide rule's
        // exceptions below hand work to the one-unit-per-wave kernel, which has no narrow form
        if (!suffix_rows_shape_ok(a, D, 2)) return (int)hipErrorInvalidValue;  // (the entry points ask suffix_narrow_eligible first)
        return launch_suffix_rows<D>(a, s, [](auto NPRE, auto TS) {
            return &suffix_attn_rows_kernel<T, D, 8, decltype(NPRE)::value, decltype(TS)::value, true>;
        });
    }
    a.packed = suffix_packed_eligible(a, D) ? 1 : 0;
    {
        // token-row kernel (shapes only, capture-safe: suffix_rows_shape_ok): measured faster wherever the one-unit-per-wave kernel would run with one wave per unit
        // (launch_suffix_r's few_units rule spreads a unit over four waves below 2048 units)
        // ... and whose caches hold at most 1024 token rows: on longer rows a wave start costs little, and the one-unit-per-wave kernel
        // streams them as fast or faster (2176-row caches, profiles/r06_suffix_rows_capacity.txt)
        bool rows = suffix_rows_shape_ok(a, D, 2) && !((int64_t)a.units < 2 * 256 * 4 && a.kv_len >= 64) && a.kv_len <= 1024;
#ifdef HYD_ABLATION_BUILD
        if (const char* e = getenv("HYD_SUFFIX_ROWS")) rows = atoi(e) != 0 && suffix_rows_shape_ok(a, D, 2);
#endif
        if (rows)
            return launch_suffix_rows<D>(a, s, [](auto NPRE, auto TS) {
                return &suffix_attn_rows_kernel<T, D, 8, decltype(NPRE)::value, decltype(TS)::value>;
            });
    }
    if (a.rows <= 1) return launch_suffix_r<T, D, 1>(a, s);
    if (a.rows <= 2) return launch_suffix_r<T, D, 2>(a, s);
    if (a.rows <= 4) return launch_suffix_r<T, D, 4>(a, s);
    return launch_suffix_r<T, D, 8>(a, s);
}

// shapes only: a call with narrow unique caches (a.kv_dim set) that the narrow token-row kernel takes
bool suffix_narrow_eligible(const SuffixArgs& a, int D) {
    return a.kv_dim >= 16 && a.kv_dim < D && a.kv_dim % 16 == 0 && suffix_rows_shape_ok(a, D, 2);
}

int launch_suffix(const SuffixArgs& a, int dtype, int D, hipStream_t s) {
    // grouped-query shapes go to the matrix-core kernel (suffix_attn_gqa.hip).  Development builds only
    // (HYD_ABLATION_BUILD): HYD_SUFFIX_IMPL=valu keeps them here, =gqa sends every addressable shape there.
#ifdef HYD_ABLATION_BUILD
    static const int force = [] {
        const char* e = getenv("HYD_SUFFIX_IMPL");
        return !e ? 0 : !strcmp(e, "valu") ? 1 : !strcmp(e, "gqa") ? 2 : 0;
    }();
#else
    constexpr int force = 0;
#endif
    if (!a.kv_dim && force != 1 && suffix_gqa_eligible(a, D, force == 2)) return launch_suffix_gqa(a, dtype, D, s);
    if (dtype == HYD_F16) {
        if (D == 128) return launch_suffix_t<F16, 128>(a, s);
        if (D == 64) return launch_suffix_t<F16, 64>(a, s);
        if (D == 256) return launch_suffix_t<F16, 256>(a, s);
    } else {
        if (D == 128) return launch_suffix_t<BF16, 128>(a, s);
        if (D == 64) return launch_suffix_t<BF16, 64>(a, s);
        if (D == 256) return launch_suffix_t<BF16, 256>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace hyd
