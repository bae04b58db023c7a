// The token-row suffix kernel: ONE body and ONE launcher for 16-bit caches (suffix_attn.hip, suffix_attn_rows_kernel) and
// e4m3fn caches (suffix_attn_fp8.hip, suffix_attn_rows_fp8_kernel).  The two differ in a cache-format policy FMT only:
//   elem                     stride unit of the cache (uint16_t: strides count 2-byte elements; uint8_t: bytes)
//   vec                      a lane's 8 elements of one token row = one request (u32x4: dwordx4; u32x2: dwordx2)
//   k_dot2<T>(vec)           the u32x4 of 16-bit pairs the v_dot2 loop consumes (identity; fp8x8_to_16<T>)
//   v_f32<T>(vec, float[8])  the 8 floats P.V consumes (widen8<T>; fp8x8_to_f32)
//   kScaled                  per-kv-head scales: k_scale[h] folded into the lane's score multiplier, v_scale[h] applied to the
//                            accumulator once, after the token-split merge and before the epilogue (false: none read)
#pragma once
#include <type_traits>
#ifdef HYD_ABLATION_BUILD
#include <cstdlib>
#endif

#include "suffix_common.h"

namespace hyd {

// Token-row form of the one-query-row decode shape (nq == 1, Hq == Hkv, Hkv a multiple of the 64 / (D / 8) heads one wave
// instruction covers -- C2 and its tensor-parallel shards): a wave walks the token rows of ONE sequence for HPI neighbouring
// heads.  A lane group of D / 8 lanes owns one head outright (all of its keys arrive in the same lanes): one wave instruction
// fetches 1 KB contiguous (16-bit caches), the waves of a workgroup sit side by side on the token row (4 KB contiguous per token
// and tensor), UT tokens x 2 tensors (16 KB at UT = 8) per wave.  No merge across lane groups or waves at the end, and a quarter
// of the waves (wave starts, page touches, epilogues, q / partial / output rows of 256 B) of the one-unit-per-wave kernel
// of suffix_attn.hip, which splits the keys of ONE head over a wave's four lane groups.
// Measured at C2 (profiles/r06_suffix_rows_*.txt; same box, same arena, alternating), first form (all of a chunk's loads,
// then all of its arithmetic): 165 vs 173 us at S = 64, 318 vs 337 at S = 128, 87.6 vs 90.8 at S = 32, equal at S <= 16; UT = 8
// beats 4 / 12 / 16, two heads per lane group, a second buffer, eight-wave workgroups and head-major launch order all measured
// equal or worse.
// Shapes with fewer than 4 waves per sequence put 4 / wps sequences into one workgroup (a.rows_wps_log2).
//
// The product form rotates the two register sets instead of doubling them: K of chunk c + 1 is requested as soon as the scores
// of chunk c are out of the K registers, V of chunk c + 1 as soon as P.V of chunk c is out of the V registers -- the registers
// of the single-buffer form (116 VGPRs, 4 waves per SIMD), but a wave always has 8 KB in flight while it computes.  The last,
// partial chunk rides the same pipeline with clamped token indices (never a predicated load).  The sequence's length travels
// as a VECTOR load in front of q and the prefetched partial (a scalar load's lgkmcnt(0) would serialise it with every later
// kernel-argument fetch), the argument block's four scalar-cache lines are touched at once, and the lane offsets are computed
// so that the first K request does not wait for the partial's LSE (see `khg`).  Measured against the first form, one process,
// alternating (profiles/r06_suffix_rows_pipelined_ab.txt): S = 8 28.5 -> 27.9 us, S = 16 50.3 -> 48.5, S = 32 92.0 -> 90.2,
// S = 64 175.8 -> 172.8 (-1.7 %), S = 128 340 -> 337; equal at S <= 4.
// Variants measured and not shipped (their code left the tree with commit b959a95, the last one that holds it; the tables stay
// in profiles/r06_suffix_rows_*.txt and profiles/r06_suffix_stride_sweep.txt): requesting (half of) chunk 0's K BEFORE the length
// is known adds nothing on top (the launch is throughput-bound, not start-latency-bound) and costs 1.5 us at S = 1..2 (rows past
// the length are fetched for nothing); walking a sequence's full chunks from a per-sequence starting chunk rescues pathological
// cache strides (129 rows between sequences: 193 vs 212 us at S = 64, the one-unit-per-wave kernel 243) and costs 2-10 % on the
// strides cache allocations have (128 / 256 / 512 / 2048 rows, S = 128: 345 vs 332, 350 vs 318).
//
// fp8 caches: 8 BYTES per lane, token and tensor (one wave instruction covers 512 contiguous bytes at D = 128); UT = 8 tokens per
// chunk is 4 KB of K + V in flight per wave, half the 16-bit kernel's bytes: UT = 16 would keep them, but hipcc then needs
// 152-166 VGPRs (spills at 4 waves per SIMD, 3 waves per SIMD without).
//
// NARROW (16-bit caches only): the cache rows hold a.kv_dim < D elements per head (a.kv_dim % 16 == 0; head dims 80 / 96 / 192
// without a zero-padded copy of the cache) while q, the partials, `out` and the LSE keep their pitch of D with zero pad columns.
// The lane geometry stays that of D.  A lane whose 8 columns start below kv_dim works as always; a PAD lane (sub * 8 >= kv_dim)
// requests the first 16 bytes of its own head's row -- an address an active lane of the same instruction fetches anyway: no new
// cache line, never a predicated load, never a byte past column kv_dim --, multiplies them by q registers that are zero (exactly
// +0 into the v_dot2 chain, so the 16-lane group sum sees what it sees on a zero-padded cache) and drops what it accumulated
// behind its last chunk: the merges and the epilogue then carry exact zeros into the pad columns of `out`.  Results are bit-identical to the D-wide form
// on zero-padded tensors for finite caches.
template <typename T, int D, int UT, int NPRE, int TS, typename FMT, bool NARROW = false>
__device__ __forceinline__ void suffix_rows_body(const SuffixArgs& a, const float* k_scale, const float* v_scale) {
    using TR = Traits<T>;
    using elem = typename FMT::elem;
    using vec = typename FMT::vec;
    typedef const __attribute__((address_space(1))) vec* gvec_p;
    constexpr int EB = (int)sizeof(elem);
    warm_kernargs_256();  // the fields in front of partials[1] span four scalar-cache lines: one miss time instead of five in a row
    constexpr int LPK = D / 8, HPI = 64 / LPK;  // lanes per head row, heads per wave instruction
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane % LPK, hg = lane / LPK;
    // waves per sequence inside a workgroup: 4 (then blockIdx.y walks further head slices), 2 or 1
    // TS > 1 (shapes with too few waves to fill the chip: a TP rank's shard, a small batch): TS waves share a (sequence, head slice)
    // and deal its 8-token chunks round-robin -- wave t takes chunks t, t + TS, ... -- then hand their (m, l, acc) to wave 0 through LDS.
    constexpr int TL = TS == 4 ? 2 : TS == 2 ? 1 : 0;
    const int ts_id = wave & (TS - 1), wrest = wave >> TL;
    const int wl = a.rows_wps_log2;
    const int bslot = (int)(blockIdx.x << (2 - wl - TL)) + (wrest >> wl);
    const int h0 = (int)((blockIdx.y << wl) + (wrest & ((1 << wl) - 1))) * HPI;  // first head of this wave
    if (bslot >= a.B || h0 >= a.Hkv) return;  // (all TS waves of a group leave together: a barrier counts the waves that are left)

    // the length as a vector load: every lane the same address; an opaque zero keeps hipcc from making it a scalar load
    int zero = 0;
    asm volatile("" : "+v"(zero));
    // dispatch slot -> sequence: the caller's schedule (hyd_suffix_params.seq_order: longest first when lengths are ragged) or the index
    const int b = a.order ? __builtin_amdgcn_readfirstlane(a.order[bslot + zero]) : bslot;
    int lenv = a.kv_len;
    if (a.sl32) lenv = a.sl32[b + zero];
    else if (a.sl64) lenv = (int)a.sl64[b + zero];

    const int64_t ridx = (int64_t)b * a.Hq + h0 + hg;  // nq == 1, g == 1: [B, 1, Hq]
    u32x4 qp = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(a.q) + ridx * D + sub * 8);
    bool pad_lane = false;
    if constexpr (NARROW) {
        pad_lane = sub * 8 >= a.kv_dim;
        if (pad_lane) qp = u32x4{0u, 0u, 0u, 0u};
    }
    float ks = 1.0f, vs = 1.0f;
    if constexpr (FMT::kScaled) {
        ks = k_scale ? k_scale[h0 + hg] : 1.0f;
        vs = v_scale ? v_scale[h0 + hg] : 1.0f;
    }
    PrePartials<NPRE> pp;
    const int npre = min(n_prefetched(a), NPRE);
    prefetch_partials(a, npre, ridx, sub, D, pp);

    // wave-uniform base (scalar registers) + per-lane 32-bit byte offset (head, dims) -> SADDR-form loads
    const gchar_p kbu = uniform_ptr(reinterpret_cast<const char*>(static_cast<const elem*>(a.k) + (int64_t)b * a.k_bs + (int64_t)h0 * a.k_hs));
    const gchar_p vbu = uniform_ptr(reinterpret_cast<const char*>(static_cast<const elem*>(a.v) + (int64_t)b * a.v_bs + (int64_t)h0 * a.v_hs));
    // (product and sum kept apart: fused, hipcc emits a 64-bit multiply-add whose unused high addend lands in the register the
    // partial's LSE is being loaded into, and the first K request waits for that load)
    unsigned khg = (unsigned)hg * (unsigned)(a.k_hs * EB), vhg = (unsigned)hg * (unsigned)(a.v_hs * EB);
    asm volatile("" : "+v"(khg), "+v"(vhg));
    const int csub = NARROW && pad_lane ? 0 : sub;  // a pad lane asks for the head's first columns (see NARROW above)
    const unsigned klane = khg + csub * (8 * EB), vlane = vhg + csub * (8 * EB);
    const unsigned krs = (unsigned)(a.k_ts * EB), vrs = (unsigned)(a.v_ts * EB);  // token stride in bytes

    vec kreg[UT], vreg[UT];
    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    float sc = a.scale_log2e;
    if constexpr (FMT::kScaled) sc *= ks;  // k = k8 * ks: the scale rides on the score multiplier

    const int len = max(0, min(__builtin_amdgcn_readfirstlane(lenv), a.kv_len));
    const int nch = (len + UT - 1) / UT;  // chunks with at least one key
    const int last = max(len - 1, 0);

    // requests of a chunk: token indices clamped to the last valid key (never a predicated load); its score is masked below
    auto issue_k = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const unsigned tc = (unsigned)min(c * UT + u, last);
            kreg[u] = __builtin_nontemporal_load((gvec_p)(kbu + (tc * krs + klane)));
        }
    };
    auto issue_v = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const unsigned tc = (unsigned)min(c * UT + u, last);
            vreg[u] = __builtin_nontemporal_load((gvec_p)(vbu + (tc * vrs + vlane)));
        }
    };
    // one chunk out of the registers.  LAST = false: a full chunk that is not the sequence's last one (all UT keys valid; the
    // next chunk's K / V are requested as soon as this one's are out of their registers).  LAST = true: the sequence's final
    // chunk, masked by the length, nothing requested behind it.
    auto chunk = [&](int c, auto LAST) __attribute__((always_inline)) {
        constexpr bool is_last = decltype(LAST)::value;
        float sv[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const u32x4 kk = FMT::template k_dot2<T>(kreg[u]);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) d = TR::dot2(qp[e], kk[e], d);
            d = group_sum<LPK>(d) * sc;
            sv[u] = (!is_last || c * UT + u < len) ? d : -INFINITY;  // wave-uniform condition
        }
        if constexpr (!is_last) {
            __builtin_amdgcn_sched_barrier(0);
            issue_k(c + TS);
            __builtin_amdgcn_sched_barrier(0);
        }
        softmax_step<false>(sv, m, l, acc);  // the new maximum is finite: every chunk that is processed starts with a valid key
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            float vf[8];
            FMT::template v_f32<T>(vreg[u], vf);
            pv_accumulate(sv[u], vf, acc);
        }
        if constexpr (!is_last) {
            __builtin_amdgcn_sched_barrier(0);
            issue_v(c + TS);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (nch > ts_id) {  // (a wave without a chunk requests nothing: an empty sequence's cache may have no rows at all)
        issue_k(ts_id);  // this wave's first chunk in the steady state's order: K, then V
        issue_v(ts_id);
        __builtin_amdgcn_sched_barrier(0);
        int c = ts_id;
        for (; c + TS < nch; c += TS) chunk(c, std::integral_constant<bool, false>{});
        chunk(c, std::integral_constant<bool, true>{});  // this wave's last chunk: masked (it may be the sequence's last)
    }
    if constexpr (NARROW) {
        // a pad lane drops what it accumulated.  HERE, in front of the token-split merge (0 * a1 + 0 * a2 stays 0), so that the merge
        // and the epilogue are the D-wide kernel's code with nothing in between: hipcc then contracts them the same way (with the
        // zeroing behind the merge it fused the merge of l in this instantiation alone, and the LSE differed in its last bit)
        if (pad_lane) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        }
    }
    if constexpr (TS > 1) {
        __shared__ float xch[4][10][64];  // [wave of the workgroup][m, l, acc[8]][lane]
        if (ts_id > 0) {
            xch[wave][0][lane] = m;
            xch[wave][1][lane] = l;
#pragma unroll
            for (int j = 0; j < 8; ++j) xch[wave][2 + j][lane] = acc[j];
        }
        __syncthreads();
        if (ts_id > 0) return;
#pragma unroll
        for (int t = 1; t < TS; ++t) {
            float a2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a2[j] = xch[wave + t][2 + j][lane];
            merge_state(m, l, acc, xch[wave + t][0][lane], xch[wave + t][1][lane], a2);
        }
    }
    if constexpr (FMT::kScaled) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] *= vs;  // v = v8 * vs, once per row
    }
    finish_row<T, D, 2, NPRE>(a, ridx, sub, m, l, acc, npre, pp);
}

// shapes only (capture-safe): one query row per unit, whole lane groups, 32-bit byte offsets inside a sequence's cache
inline bool suffix_rows_shape_ok(const SuffixArgs& a, int D, int elem_bytes) {
    const int hpi = 64 / (D / 8);
    return a.rows == 1 && a.nq == 1 && a.g == 1 && a.Hkv % hpi == 0 && cache_span_fits_32bit(a, elem_bytes) && a.n_pre <= 2;
}

// Launch geometry and the choice of the instantiation, for both cache formats.  ARGS is the kernel's argument block (SuffixArgs or
// SuffixKvqArgs; copied and completed here), kernel_of(NPRE, TS) the format's __global__ instantiation.
inline SuffixArgs& suffix_args_of(SuffixArgs& a) { return a; }
inline SuffixArgs& suffix_args_of(SuffixKvqArgs& ka) { return ka.a; }
template <int D, typename ARGS, typename KERNEL_OF>
static int launch_suffix_rows(const ARGS& args0, hipStream_t s, KERNEL_OF kernel_of) {
    constexpr int HPI = 64 / (D / 8);
    ARGS args = args0;
    SuffixArgs& a = suffix_args_of(args);
    const int wps = a.Hkv / HPI;  // waves per sequence
    a.rows_wps_log2 = wps >= 3 ? 2 : wps == 2 ? 1 : 0;
    const int wl = a.rows_wps_log2;
    // Token split (shapes only).  When one wave covers all heads of a token (Hkv = the 64 / (D / 8) heads of a wave instruction: a
    // 1 KB token row, a TP = 8 shard of C2), the 4 waves of a workgroup used to walk 4 different sequences, 8 KB of each at a time;
    // sharing ONE sequence between 2 (4) of them -- 16 (32) KB of the same contiguous cache requested together -- streams 6-13 %
    // faster from S = 16 on at every batch size (profiles/r06_suffix_rows_token_split_ab.txt: B = 1024, S = 64 28.5 -> 25.8 us,
    // S = 128 51.4 -> 44.9; B = 8192, S = 64 183 -> 167); 2 is the better split up to 2048 sequences, 4 above (and the cheaper one at
    // S = 8: + 0.5 us).  With two or more waves per sequence already (8 or more kv heads at D = 128) it changes nothing: not used.
    int ts = 1;
    if (wl == 0 && a.n_pre < 2 && a.kv_len >= 32) ts = a.B <= 2048 ? 2 : 4;
#ifdef HYD_ABLATION_BUILD
    if (const char* e = getenv("HYD_ROWS_TS")) { ts = atoi(e); if (wl + (ts == 4 ? 2 : ts == 2 ? 1 : 0) > 2 || a.n_pre >= 2) ts = 1; }
#endif
    const int tl = ts == 4 ? 2 : ts == 2 ? 1 : 0;
    const dim3 grid((unsigned)((a.B + (4 >> (wl + tl)) - 1) >> (2 - wl - tl)), (unsigned)((wps + (1 << wl) - 1) >> wl), 1);
    auto launch = [&](auto NPRE, auto TS) {
        hipLaunchKernelGGL(kernel_of(NPRE, TS), grid, dim3(256), 0, s, args);
        return (int)hipGetLastError();
    };
    using std::integral_constant;
    if (a.n_pre == 2) return launch(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    if (ts == 4) return launch(integral_constant<int, 1>{}, integral_constant<int, 4>{});
    if (ts == 2) return launch(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    return launch(integral_constant<int, 1>{}, integral_constant<int, 1>{});
}

}  // namespace hyd
