// Suffix pass for grouped-query shapes over fp8 (e4m3fn) unique caches (hyd_kv_quant, include/hydragen_hip.h): the matrix-core
// kernel of suffix_attn_gqa.hip with K / V rows of D BYTES.  q, the prefix partials and the output stay 16-bit.
//
// Contract: for every shape it takes, `out` and `lse` are bit-identical to suffix_attn_gqa_kernel run on
// dequantize_kv(k8, k_scale, q dtype) / dequantize_kv(v8, v_scale, q dtype) (hydragen_amd/kv_quant.py).  So every K and V element
// is widened by that rule when a tile is emptied -- float(fp8) * scale[h] as an fp32 product, rounded once more to the q dtype,
// ties to even, the scale read on the device -- and the unchanged 16-bit MFMAs consume the result in the unchanged order; the
// launcher takes the 16-bit launcher's shapes-only choices (gqa_launch_plan).  The scales are NOT folded into the score multiplier or
// the accumulator: cheaper, but another rounding.
//
// What differs from the 16-bit kernel is the way from HBM to the MFMA operands:
//   K, V: LDS-DMA of whole fp8 rows into a 32-key landing tile each, 32 * D bytes: half a 16-bit step.  The 16-bit kernel is bound
//         by the bytes a wave keeps in flight (profiles/r06_head_dim_rates.txt), so D <= 128 keeps TWO steps in flight (NSET, the
//         16-bit D = 64 scheme with its counted wait); D = 256 has the byte geometry of 16-bit D = 128 and keeps one.
//   K:    the A operand is read straight from the landing tile: one ds_read_b64 (8 dims) per fragment, widened in registers.
//   V:    the landing tile is widened into a wave-private 16-bit tile in the 16-bit kernel's swizzled layout, and V^T is read from it
//         with the 16-bit transposing reads.  (ds_read_b64_tr_b8 exists on gfx950, but whether its lane map fits the
//         accumulator-permuted key order of P^T has not been established; one more LDS pass buys the unchanged, tested layout.)
// The stream is this file's own: the tiles, the DMA geometry, the number of steps in flight, the collect with its widening, the
// scale loads and their settle point differ from the 16-bit kernel's, which is most of what the stream loop is.  What is around
// it -- requesting, fetching and folding the prefix partials, the softmax step on a collected tile, the four-wave merge, the
// epilogue and the raise-the-LDS-limit launch -- is the 16-bit kernel's own code, shared through suffix_gqa_unit.h (the asm
// primitives: suffix_gqa_common.h).  Written out here as there: the two loops over a wave's partials; here only: the query load
// (profiles/gqa_unit_frame.md has the measurements behind both).  tests/test_fp8_gqa_gpu.py holds the two kernels bit-equal.
// The kernel's text, the widening rule (fp8x8_dequant) and the launcher templates live in suffix_gqa_fp8_kernel.h, which
// suffix_attn_gqa_fp8_causal.hip compiles a second time with the causal tail's per-row key limit; this file instantiates the plain form.
#include "suffix_gqa_fp8_kernel.h"

namespace hyd {

// Shapes only (capture-safe): exactly the shapes launch_suffix sends to the grouped-query kernel for a sequence's own 16-bit cache
// of the same logical shape (strides count bytes here, elements there: the same numbers).
bool suffix_gqa_fp8_eligible(const SuffixArgs& a, int D) {
    return !a.shared_kv && !a.pk && suffix_gqa_eligible(a, D, /*any_shape=*/false);
}

int launch_suffix_gqa_fp8(const SuffixKvqArgs& ka, int dtype, int D, hipStream_t s) {
    if (!suffix_gqa_fp8_eligible(ka.a, D)) return (int)hipErrorInvalidValue;
    return launch_gqa8(ka, dtype, D, s);
}

}  // namespace hyd
