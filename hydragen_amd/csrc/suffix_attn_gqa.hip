// Suffix pass for grouped-query shapes (nq * g >= 4 query rows per (sequence, kv head)): the same operator as
// suffix_attn.hip -- attention of the unit's rows over the first seq_len[b] keys of the sequence's own cache
// plus the fused LSE combine with the prefix partials -- but with the two contractions on the matrix cores.
//
// Replaces _fwd_kernel_splitK + _splitK_reduce (/root/reference/hydragen/flash.py:76-281,
// hydragen/xformers_stuff.py:189-428) and combine_lse (hydragen/attention.py:21-174) for GQA configurations
// such as the reference microbenchmark's default Hq = 8, Hkv = 1 (scripts/microbenchmark.py:136-138).
//
// Why a second kernel: with R rows per unit the wave-level dot-product kernel issues ~R * 12 VALU instructions
// per 4 keys and stops being HBM-bound at R = 8 (measured 2.1 TB/s at B = 2048, Hq/Hkv = 8/1, S = 256).  Here a
// wave owns one unit and walks its keys 32 at a time:
//   K, V: LDS-DMA (buffer_load ... lds: whole rows, zero fill past seq_len) into one swizzled 32-key landing tile each;
//        once a step has landed its tiles are emptied into registers -- K as MFMA A operands (ds_read_b128), V^T with
//        ds_read_b64_tr_b16 -- and handed straight to the next step's DMA
//   S^T = K . Q^T      2 * D/32 x v_mfma_f32_16x16x32 (Q rows padded to 16, kept in registers)
//   online softmax in base 2, one query row per lane & 15, 8 scores per lane, two cross-lane exchanges
//   O^T += V^T . P^T   D/16 x MFMA, P^T converted in registers (the contraction index is permuted to the
//        accumulator layout, keys {4j..4j+3, 16+4j..}, so no data moves)
// Producer and consumer of a wave's tiles are the same wave: no barriers.
//
// Software pipeline: collect(j) -> issue(j + 1) -> compute(j): one 16 KiB step in flight per wave while the previous one is
// computed out of registers, 16 KiB of LDS per wave, 8 waves per CU.  Round 4's form double-buffered in LDS (V) and in
// asm-owned AGPRs (K, loaded straight into operand layout: 16 rows x 64 B per instruction, every quarter wave 16 different
// cache lines); a timing experiment of this round showed that a coalesced route for K alone is worth 10 % on 8-kv-head shapes
// (whole-job C5, S = 128: 222 -> 198 us), which is what the landing tiles are for.
#include "suffix_gqa_kernel.h"

namespace hyd {

// Shapes-only eligibility (capture-safe): enough query rows per unit for the matrix cores to pay, enough units to
// fill the chip with one wave each, and byte offsets inside a unit's cache that fit the 32-bit buffer addressing.
bool suffix_gqa_eligible(const SuffixArgs& a, int D, bool any_shape) {
    if (D != 64 && D != 128 && D != 256) return false;
    const int64_t chunks = (a.rows + 15) / 16;
    // measured on MI355X (tools/kbench.py, HYD_SUFFIX_IMPL=valu|gqa; round 5's kernel): from 3 rows per unit the matrix cores win at
    // every suffix length (12/4 heads, B = 1024: 10.2 / 23.4 / 82.5 us at S = 8 / 64 / 256 against 12.0 / 30.6 / 104); with 2 rows they win
    // from S = 64 on and lose below (16/8 heads: 20 vs 14 us at S = 8), with 1 row only from S = 128: those stay on the dot-product kernel
    if (!any_shape && a.rows < 3) return false;
    // head dim 256 (32 KB of tiles and one SIMD per wave): measured against the dot-product kernel, 7 x faster with one wave per
    // unit (B = 2048, 8/1 heads, S = 256: 667 -> 90 us) but 15 % slower in the four-waves-per-unit form that few units take
    if (D == 256 && gqa_few_units(a, (int)chunks)) return false;
    const int64_t span = (int64_t)a.kv_len * (a.k_ts > a.v_ts ? a.k_ts : a.v_ts) * 2;
    return span < (int64_t)1 << 31 && a.Hkv <= 65535 && chunks <= 65535;
}

template <typename T, int D>
static int launch_gqa_t(const SuffixArgs& a_in, hipStream_t s) {
    SuffixArgs a = a_in;
    const int chunks = (a.rows + 15) / 16;
    // waves per unit and kv heads per workgroup, from shapes: gqa_launch_plan (suffix_gqa_common.h; the fp8 kernel takes the same)
    const GqaLaunchPlan plan = gqa_launch_plan(a, D);
    bool few_units = plan.few_units;
    int hpw = plan.hpw;
#ifdef HYD_ABLATION_BUILD
    if (const char* e = getenv("HYD_GQA_BLIND")) a.dbg_blind = atoi(e);
    if (const char* e = getenv("HYD_GQA_WPU")) {  // (the heads per workgroup follow the forced choice, as they follow the measured one)
        few_units = atoi(e) == 4;
        hpw = 1;
        if (!few_units && !a.shared_kv && !a.pk && a.Hkv <= 8) {
            hpw = a.Hkv % 4 == 0 ? 4 : a.Hkv % 2 == 0 ? 2 : 1;
            if (D == 256 && hpw > 2) hpw = 2;
        }
    }
    if (const char* e = getenv("HYD_GQA_HPW")) hpw = few_units ? 1 : atoi(e);
#endif
    dim3 grid((unsigned)a.B * (unsigned)(a.Hkv / hpw), chunks, 1);
    size_t pad = 0;  // development: dynamic LDS that only lowers the occupancy (waves per CU = 160 KiB / (16 KiB + pad))
#ifdef HYD_ABLATION_BUILD
    if (const char* e = getenv("HYD_GQA_LDS_PAD")) pad = (size_t)atoi(e);
#endif
    if constexpr (D == 256) {
        if (few_units || a.shared_kv) return (int)hipErrorInvalidValue;  // (not eligible: suffix_gqa_eligible, level_is_small)
    } else {
        if (a.shared_kv) {  // a small shared level: its keys are read by several workgroups, default cache policy
            if (few_units) return launch_gqa_k<T, D, 4, false, 1>(a, grid, 0, s);
            return launch_gqa_k<T, D, 1, false, 1>(a, grid, pad, s);
        }
        if (few_units) return launch_gqa_k<T, D, 4, true, 1>(a, grid, 0, s);
    }
    switch (hpw) {
#ifdef HYD_ABLATION_BUILD
        case 8:  // (A/B only: not chosen from shapes any more)
            if constexpr (D < 256) return launch_gqa_k<T, D, 1, true, 8>(a, grid, 0, s);
            else return (int)hipErrorInvalidValue;
#endif
        case 4:
            if constexpr (D < 256) return launch_gqa_k<T, D, 1, true, 4>(a, grid, 0, s);
            else return (int)hipErrorInvalidValue;
        case 2: return launch_gqa_k<T, D, 1, true, 2>(a, grid, 0, s);
        default: return launch_gqa_k<T, D, 1, true, 1>(a, grid, pad, s);
    }
}

int launch_suffix_gqa(const SuffixArgs& a, int dtype, int D, hipStream_t s) {
    if (dtype == HYD_F16) {
        if (D == 128) return launch_gqa_t<F16, 128>(a, s);
        if (D == 64) return launch_gqa_t<F16, 64>(a, s);
        if (D == 256) return launch_gqa_t<F16, 256>(a, s);
    } else {
        if (D == 128) return launch_gqa_t<BF16, 128>(a, s);
        if (D == 64) return launch_gqa_t<BF16, 64>(a, s);
        if (D == 256) return launch_gqa_t<BF16, 256>(a, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace hyd
