// Causal-tail suffix pass over fp8 (e4m3fn) unique caches (hyd_suffix_attn_causal_fwd_kvq, hyd_decode_attn_fused_kvq with
// hyd_decode_params.causal_tail and HYD_KVQ_CAUSAL): the suffix pass of a MULTI-TOKEN decode step on a cache of half the bytes.  The
// fp8 matrix-core kernel (suffix_gqa_fp8_kernel.h) compiled a second time with the per-row key limit, exactly as suffix_attn_causal.hip
// compiles the 16-bit kernel a second time; the instantiations of suffix_attn_gqa_fp8.hip are not touched.
//
// Contract: wherever both kernels take the shape, `out` and `lse` are bit-identical to suffix_attn_gqa_causal_kernel run on
// dequantize_kv(k8, k_scale, q dtype) / dequantize_kv(v8, v_scale, q dtype) (tests/test_fp8_causal_gpu.py).
#define HYD_SUFFIX_CAUSAL_TAIL 1
#include "suffix_gqa_fp8_kernel.h"

namespace hyd {

// Shapes only (capture-safe): 2..8 query tokens, rows of D bytes, no shared segment in the same launch, and the matrix-core kernel's
// own limits.  any_shape: there is no fp8 one-unit-per-wave kernel, so units of 2 rows (multi-head models with one draft) run on the
// matrix cores as well, as they do in the 16-bit one-launch small form.  With 16-bit caches such units go to the one-unit-per-wave
// causal kernel, because the plain matrix-core kernel loses to it below 64 keys (suffix_gqa_eligible).  The rule here was written
// unmeasured; measured since (profiles/speculative_fp8.md; 32/32 heads, T = 2, D = 128): this kernel takes 0.52-0.85 x the time of the
// 16-bit one-unit-per-wave causal kernel at S = 64 / 256 / 1024 and B = 32 / 128 / 1024.  Below 64 keys: NOT measured.
// Head dim 256 with few units stays out, as in the 16-bit plan.
bool suffix_gqa_fp8_causal_eligible(const SuffixArgs& a, int D) {
    if (a.nq < 2 || a.nq > 8 || a.kv_dim || a.pk || a.shared_kv) return false;
    return suffix_gqa_eligible(a, D, /*any_shape=*/true);
}

int launch_suffix_gqa_fp8_causal(const SuffixKvqArgs& ka, int dtype, int D, hipStream_t s) {
    if (!suffix_gqa_fp8_causal_eligible(ka.a, D)) return (int)hipErrorInvalidValue;
    return launch_gqa8(ka, dtype, D, s);
}

}  // namespace hyd
