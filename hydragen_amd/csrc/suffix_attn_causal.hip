// Causal-tail suffix pass (hyd_suffix_attn_causal_fwd, hyd_decode_params.causal_tail): the suffix pass of a MULTI-TOKEN decode step.
// The nq = T query tokens of sequence b are its last T tokens and their K/V already sit in the cache (hyd_rope_append_multi), so
// token i attends the keys below clamp(seq_len[b], 0, kv_len) - (T - 1 - i) -- bottom-right aligned, what flash_attention(causal=True)
// computes when the new keys are part of the key tensor.  The unique K/V is still streamed ONCE for all T tokens of a row; the only
// difference from the plain pass is a per-row key limit in the score mask.
//
// The two kernels that can receive nq > 1 are compiled here a second time with that limit (HYD_SUFFIX_CAUSAL_TAIL: suffix_gqa_kernel.h,
// suffix_unit.h); the instantiations of suffix_attn_gqa.hip and suffix_attn.hip are not touched.  The forms WITHOUT the limit -- the
// token-row kernel, the packed path, the one-launch walk over a shared segment, narrow rows -- all need nq == 1 or are refused by the
// entry points (api.hip), so a causal call can never run non-causally: what no kernel here takes is an error.
#define HYD_SUFFIX_CAUSAL_TAIL 1
#include "suffix_gqa_kernel.h"
#include "suffix_unit.h"

namespace hyd {

// matrix-core kernel: the plain launcher's choices (gqa_launch_plan), unique keys only
template <typename T, int D>
static int launch_causal_gqa_t(const SuffixArgs& a, hipStream_t s) {
    const int chunks = (a.rows + 15) / 16;
    const GqaLaunchPlan plan = gqa_launch_plan(a, D);
    dim3 grid((unsigned)a.B * (unsigned)(a.Hkv / plan.hpw), chunks, 1);
    if constexpr (D == 256) {
        if (plan.few_units) return (int)hipErrorInvalidValue;  // (not eligible: suffix_gqa_eligible)
    } else {
        if (plan.few_units) return launch_gqa_k<T, D, 4, true, 1>(a, grid, 0, s);
    }
    switch (plan.hpw) {
        case 4:
            if constexpr (D < 256) return launch_gqa_k<T, D, 1, true, 4>(a, grid, 0, s);
            else return (int)hipErrorInvalidValue;
        case 2: return launch_gqa_k<T, D, 1, true, 2>(a, grid, 0, s);
        default: return launch_gqa_k<T, D, 1, true, 1>(a, grid, 0, s);
    }
}

// one-unit-per-wave kernel: launch_suffix_r's rule (suffix_attn.hip)
template <typename T, int D, int R>
static int launch_causal_unit_r(const SuffixArgs& a, hipStream_t s) {
    const int row_chunks = (a.rows + R - 1) / R;
    const bool few_units = (int64_t)a.units * row_chunks < 2 * 256 * 4 && a.kv_len >= 64;
    if (few_units) {
        dim3 grid(a.B, a.Hkv, row_chunks);
        hipLaunchKernelGGL((suffix_attn_causal_kernel<T, D, R, 4>), grid, dim3(256), 0, s, a);
    } else {
        dim3 grid(a.B, (a.Hkv + 3) / 4, row_chunks);
        hipLaunchKernelGGL((suffix_attn_causal_kernel<T, D, R, 1>), grid, dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

template <typename T, int D>
static int launch_causal_t(const SuffixArgs& a, hipStream_t s) {
    if (suffix_gqa_eligible(a, D, false)) return launch_causal_gqa_t<T, D>(a, s);
    // what the matrix-core kernel leaves: 2-row units, and head dim 256 with few units
    if (a.rows <= 2) return launch_causal_unit_r<T, D, 2>(a, s);
    if constexpr (D == 256) {
        if (a.rows <= 4) return launch_causal_unit_r<T, D, 4>(a, s);
        return launch_causal_unit_r<T, D, 8>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

// shapes only: a call the causal kernels take -- 2..8 query tokens, rows of D elements, no shared segment in the same launch
bool suffix_causal_eligible(const SuffixArgs& a, int D) {
    if (a.nq < 2 || a.nq > 8 || a.kv_dim || a.pk || a.shared_kv) return false;
    if (D != 64 && D != 128 && D != 256) return false;
    return suffix_gqa_eligible(a, D, false) || a.rows <= 2 || D == 256;
}

int launch_suffix_causal(const SuffixArgs& a, int dtype, int D, hipStream_t s) {
    if (!suffix_causal_eligible(a, D)) return (int)hipErrorInvalidValue;
    if (dtype == HYD_F16) {
        if (D == 128) return launch_causal_t<F16, 128>(a, s);
        if (D == 64) return launch_causal_t<F16, 64>(a, s);
        return launch_causal_t<F16, 256>(a, s);
    }
    if (D == 128) return launch_causal_t<BF16, 128>(a, s);
    if (D == 64) return launch_causal_t<BF16, 64>(a, s);
    return launch_causal_t<BF16, 256>(a, s);
}

}  // namespace hyd
