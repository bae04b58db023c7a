// The one-unit-per-wave suffix kernel of suffix_attn.hip (the design notes are there) and its packed short-sequence path: the body in a
// header so that suffix_attn_causal.hip can instantiate the causal-tail form without touching the instantiations of suffix_attn.hip.
#pragma once
#include <type_traits>

#include "suffix_rows.h"

namespace hyd {

// Packed path for SHORT sequences with one query row per unit (decode with Hq == Hkv, nq == 1 -- C2): a LANE GROUP of
// D/8 lanes owns one (sequence, kv head) unit, so a wave works on 64 / (D/8) consecutive kv heads of one sequence (4 at
// D = 128) and walks their keys together: one wave instruction fetches one token's K (or V) rows of those heads = 1 KiB
// contiguous.  The one-unit-per-wave path spends ~300 instructions per unit outside its key loop (three quarters of a
// load instruction idle at short lengths, two rounds of cross-lane-group merges, a per-wave epilogue); at C2 that is
// 32768 waves and 16 us of pure issue time, the whole cost of a step with a short suffix (22 us at S = 1 for 6 us of
// HBM traffic).  Here a lane group keeps its own (m, l, acc): no cross-group merge at all, a quarter of the waves
// (measured at C2, fused entry: S = 1 22.2 -> 7.4 us, S = 4 22.4 -> 16.0 us, S = 8 29.9 -> 27.0 us; from S = 16 on the
// one-unit-per-wave path streams 2-4 % faster -- more loads in flight -- so the choice is made per sequence at RUN time
// from its length, inside the one kernel the shapes select: capture-safe, no device read on the host).
constexpr int kPackedMaxLen = 12;
template <typename T, int D, int NPRE>
__device__ __forceinline__ void suffix_packed_body(const SuffixArgs& a, int b, int ygroup, int len) {
    using TR = Traits<T>;
    constexpr int LPK = D / 8;     // lanes per unit
    constexpr int HPW = 64 / LPK;  // units (kv heads) per wave
    constexpr int U = 2;           // keys in flight per wave and tensor (x 1 KiB); sequences here are at most kPackedMaxLen long
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane % LPK, hg = lane / LPK;
    const int h0 = (ygroup * 4 + wave) * HPW;  // first head of this wave
    if (h0 >= a.Hkv) return;
    const int hk = h0 + hg;
    const bool hvalid = hk < a.Hkv;
    const int hkc = hvalid ? hk : a.Hkv - 1;  // idle lane groups shadow the last head and never store

    const int64_t ridx = (int64_t)b * a.Hq + hkc;  // nq == 1, g == 1: [B, 1, Hq]
    const u32x4 qp = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(a.q) + ridx * D + sub * 8);
    // the first 16-bit partials (the usual single prefix level; a second level), fetched under the K/V stream
    const int npre = min(n_prefetched(a), NPRE);
    PrePartials<NPRE> pp;
    prefetch_partials(a, npre, ridx, sub, D, pp);

    // wave-uniform sequence base (scalar registers) + per-lane 32-bit byte offset (head, dims) -> SADDR-form loads
    const gchar_p kbu = uniform_ptr(reinterpret_cast<const char*>(static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs));
    const gchar_p vbu = uniform_ptr(reinterpret_cast<const char*>(static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs));
    const unsigned klane = (unsigned)(hkc * a.k_hs * 2 + sub * 16), vlane = (unsigned)(hkc * a.v_hs * 2 + sub * 16);
    const unsigned krs = (unsigned)(a.k_ts * 2), vrs = (unsigned)(a.v_ts * 2);  // token stride in bytes

    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const float sc = a.scale_log2e;
    auto chunk = [&](auto UU_C, int t0) __attribute__((always_inline)) {
        constexpr int UU = decltype(UU_C)::value;
        u32x4 kreg[UU], vreg[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            // never predicate the loads: clamp to the last valid key, its score is forced to -inf below
            const unsigned tc = (unsigned)min(t0 + u, len - 1);
            kreg[u] = __builtin_nontemporal_load((gu32x4_p)(kbu + (tc * krs + klane)));
            vreg[u] = __builtin_nontemporal_load((gu32x4_p)(vbu + (tc * vrs + vlane)));
        }
        float s[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) d = TR::dot2(qp[i], kreg[u][i], d);
            d = group_sum<LPK>(d);
            s[u] = (t0 + u < len) ? d * sc : -INFINITY;  // wave-uniform condition
        }
        softmax_step<false>(s, m, l, acc);  // the new maximum is finite: t0 < len
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            float vf[8];
            widen8<T>(vreg[u], vf);
            pv_accumulate(s[u], vf, acc);
        }
    };
    int t = 0;
    for (; t + U <= len; t += U) chunk(std::integral_constant<int, U>{}, t);
    for (; t < len; ++t) chunk(std::integral_constant<int, 1>{}, t);

    if (hvalid) finish_row<T, D, 2, NPRE>(a, ridx, sub, m, l, acc, npre, pp);
}

// NPRE: 16-bit partials fetched under the K/V stream (suffix_common.h); 2 is instantiated for the decode shape only
// (R = 1, one wave per unit) and launched when the call has two such partials (a two-level hierarchy).
// CT: causal tail (hyd_suffix_attn_causal_fwd, hyd_decode_params.causal_tail; R >= 2): the nq query tokens of a sequence are its LAST
// nq tokens, their keys already in the cache, and token iq sees the keys below len - (nq - 1 - iq): the key test becomes per row.
// With len >= nq key 0 stays visible to every row; a row that has seen no key yet (its lane group's keys lie past its limit, or
// len < nq) is what softmax_step's GUARD already handles.
// The including source picks the form with HYD_SUFFIX_CAUSAL_TAIL (one form per translation unit): the plain kernel keeps the name,
// the template arguments and the text it has always had, so the instantiations of suffix_attn.hip compile as before.
#ifndef HYD_SUFFIX_CAUSAL_TAIL
#define HYD_SUFFIX_CAUSAL_TAIL 0
#endif
#if HYD_SUFFIX_CAUSAL_TAIL
#define HYD_UNIT_KERNEL suffix_attn_causal_kernel
#else
#define HYD_UNIT_KERNEL suffix_attn_kernel
#endif
template <typename T, int D, int R, int WPU, int NPRE = 1, int U_ = 4, int OCC = (R == 1 ? 6 : 1), int PIPE = 0>
__global__ __launch_bounds__(256, OCC) void HYD_UNIT_KERNEL(const SuffixArgs a) {
    constexpr bool CT = HYD_SUFFIX_CAUSAL_TAIL != 0;
    static_assert(!CT || (PIPE == 0 && R >= 2), "causal tail: units of two or more rows, the plain key loop");
    using TR = Traits<T>;
    constexpr int LPK = D / 8;    // lanes per key row
    constexpr int KPI = 64 / LPK; // keys per wave instruction
    constexpr int U = U_;  // key iterations in flight per wave (x2 tensors x 1 KiB); occupancy supplies the rest
    __shared__ float xbuf[WPU > 1 ? (WPU - 1) * R * (2 + D) : 1];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = lane % LPK, ks = lane / LPK;
    const int wv = wave % WPU;
    // grid = (sequence, kv-head group, row chunk): no integer division on the way to (b, hk).  Sequence
    // is the fastest-varying index on purpose: measured A/B on MI355X (same run, S = 128..256), spreading
    // concurrently running workgroups over different sequences streams 5-10 % faster than walking the
    // head groups of one sequence (whose rows share HBM channels).
    const int b = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;  // dispatch slot -> sequence (hyd_suffix_params.seq_order)
    const int hk = blockIdx.y * (4 / WPU) + wave / WPU;
    if (hk >= a.Hkv) return;  // uniform per unit (all WPU waves of a unit leave together)
    const int row0 = blockIdx.z * R;

    int len = a.kv_len;
    if (a.sl32) len = a.sl32[b];
    else if (a.sl64) len = (int)a.sl64[b];
    len = max(0, min(len, a.kv_len));
    if constexpr (R == 1 && WPU == 1 && D == 128) {
        // short sequence and a packable shape (a.packed, shapes only): the first of every 4 workgroups of this
        // sequence serves the 16 (D = 128) kv heads of all four with the lane-group layout, the other three leave
        if (a.packed && len <= kPackedMaxLen) {
            if ((blockIdx.y & 3) == 0) suffix_packed_body<T, D, NPRE>(a, b, blockIdx.y >> 2, len);
            return;
        }
    }

    // ---- query rows (packed 16-bit pairs, 8 dims per lane) -------------------------------------
    u32x4 qp[R];
    [[maybe_unused]] int back[R];  // CT: the newest keys row r's token does not see
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        u32x4 z = {0u, 0u, 0u, 0u};
        if constexpr (CT) back[r] = row < a.rows ? a.nq - 1 - row / a.g : 0;
        if (row < a.rows) {
            const int iq = a.nq == 1 ? 0 : row / a.g, gq = a.nq == 1 ? row : row % a.g;
            const uint16_t* qr = static_cast<const uint16_t*>(a.q) +
                                 (((int64_t)b * a.nq + iq) * a.Hq + hk * a.g + gq) * D + sub * 8;
            qp[r] = *reinterpret_cast<const u32x4*>(qr);
        } else {
            qp[r] = z;
        }
    }
    // ---- prefetch the first 16-bit partials (the usual single prefix level; a second level) for the rows this lane
    // group will finish in the epilogue, so their HBM latency overlaps the K/V stream instead of following it -----
    constexpr int RPG = (R + KPI - 1) / KPI;  // epilogue rows per lane group
    PrePartials<NPRE> pp[RPG];
    const int npre = min(n_prefetched(a), NPRE);
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
        const int r = ks + j * KPI;
        const int row = row0 + r;
        const bool live = r < R && row < a.rows;
        const int rowc = live ? row : 0;
        const int iq = a.nq == 1 ? 0 : rowc / a.g, gq = a.nq == 1 ? rowc : rowc % a.g;
        const int64_t ridx = ((int64_t)b * a.nq + iq) * a.Hq + hk * a.g + gq;
        prefetch_partials(a, live ? npre : 0, ridx, sub, D, pp[j]);
    }

    // wave-uniform unit base (scalar registers) + 32-bit per-lane byte offsets -> SADDR-form loads
    const char* kb_ = reinterpret_cast<const char*>(static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)hk * a.k_hs);
    const char* vb_ = reinterpret_cast<const char*>(static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hk * a.v_hs);
    const gchar_p kbu = uniform_ptr(kb_), vbu = uniform_ptr(vb_);
    const unsigned krs = (unsigned)(a.k_ts * 2), vrs = (unsigned)(a.v_ts * 2);  // token stride in bytes

    float m[R], l[R], acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = -INFINITY;
        l[r] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
    }

    const int niter = (len + KPI * WPU - 1) / (KPI * WPU);
    const float sc = a.scale_log2e;
    // One chunk = UU key iterations (UU wave instructions per tensor in flight): loads first, then scores,
    // one online-softmax update, then the P.V accumulation.  Full chunks use UU = U; the tail (and every
    // short sequence) runs one iteration at a time, so a wave never issues loads or arithmetic for
    // iterations beyond ceil(len / keys-per-iteration) -- at small S the kernel is bound by exactly this
    // per-wave instruction overhead, not by HBM.
    auto chunk = [&](auto UU_C, int it) __attribute__((always_inline)) {
        constexpr int UU = decltype(UU_C)::value;
        u32x4 kreg[UU], vreg[UU];
        bool valid[UU];
        [[maybe_unused]] int keys[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            const int key = ((it + u) * WPU + wv) * KPI + ks;
            valid[u] = key < len;
            if constexpr (CT) keys[u] = key;
            // never predicate the loads (a branch per load serialises them): clamp to the last valid key,
            // its score is forced to -inf below so it contributes exactly 0
            const int kc = min(key, len - 1);
            kreg[u] = __builtin_nontemporal_load((gu32x4_p)(kbu + ((unsigned)kc * krs + sub * 16)));
            vreg[u] = __builtin_nontemporal_load((gu32x4_p)(vbu + ((unsigned)kc * vrs + sub * 16)));
        }
        float s[R][UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) d = TR::dot2(qp[r][i], kreg[u][i], d);
                d = group_sum<LPK>(d);
                if constexpr (CT) s[r][u] = keys[u] < len - back[r] ? d * sc : -INFINITY;
                else s[r][u] = valid[u] ? d * sc : -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) softmax_step<true>(s[r], m[r], l[r], acc[r]);
        // V is widened one key at a time, right where it is consumed (keeps the register footprint,
        // hence the occupancy that hides HBM latency, independent of UU).  The loop is written out here and in the rotated form
        // below rather than through pv_accumulate: behind a function hipcc allocates registers differently in five bf16
        // instantiations of this kernel (profiles/r07_suffix_refactor_isa.md)
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            float vf[8];
            widen8<T>(vreg[u], vf);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fmaf(s[r][u], vf[j], acc[r][j]);
        }
    };
    int it = 0;
    if constexpr (PIPE != 0) {
        static_assert(!(CT && PIPE != 0), "the rotated full-chunk path masks with `valid` only: it has no per-row key limit");
        // Long caches (more than 1024 rows: the token-row kernel does not take them): the full chunks with rotated requests, as in the
        // token-row kernel -- K of chunk c + 1 goes out as soon as the scores of chunk c have left the K registers, V of chunk c + 1
        // behind P.V of chunk c -- the same registers, never an empty queue.  2176-row caches, C2 heads, one process, alternating
        // (profiles/r06_unit_kernel_rotated_ab.txt): S = 64 188.7 -> 183.6 us, S = 512 1319 -> 1298, S = 2176 5401 -> 5337;
        // on 128- and 1024-row caches it loses 1-4 %, so only caches beyond 1024 rows take it.
        const int nfull = niter / U;
        if (nfull > 0) {
            u32x4 kreg[U], vreg[U];
            auto key_of = [&](int c, int u) __attribute__((always_inline)) { return ((c * U + u) * WPU + wv) * KPI + ks; };
            auto issue_k = [&](int c) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    kreg[u] = __builtin_nontemporal_load((gu32x4_p)(kbu + ((unsigned)min(key_of(c, u), len - 1) * krs + sub * 16)));
            };
            auto issue_v = [&](int c) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    vreg[u] = __builtin_nontemporal_load((gu32x4_p)(vbu + ((unsigned)min(key_of(c, u), len - 1) * vrs + sub * 16)));
            };
            auto body = [&](int c, auto MORE) __attribute__((always_inline)) {
                constexpr bool more = decltype(MORE)::value;
                float s[R][U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool valid = key_of(c, u) < len;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        float d = 0.f;
#pragma unroll
                        for (int i = 0; i < 4; ++i) d = TR::dot2(qp[r][i], kreg[u][i], d);
                        d = group_sum<LPK>(d);
                        s[r][u] = valid ? d * sc : -INFINITY;
                    }
                }
                if constexpr (more) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue_k(c + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) softmax_step<true>(s[r], m[r], l[r], acc[r]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float vf[8];
                    widen8<T>(vreg[u], vf);
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fmaf(s[r][u], vf[j], acc[r][j]);
                }
                if constexpr (more) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue_v(c + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            issue_k(0);
            issue_v(0);
            __builtin_amdgcn_sched_barrier(0);
            int c = 0;
            for (; c + 1 < nfull; ++c) body(c, std::integral_constant<bool, true>{});
            body(c, std::integral_constant<bool, false>{});
            it = nfull * U;
        }
    } else {
        for (; it + U <= niter; it += U) chunk(std::integral_constant<int, U>{}, it);
    }
    for (; it < niter; ++it) chunk(std::integral_constant<int, 1>{}, it);

    // ---- merge the KPI lane groups of the wave (butterfly: every lane ends with the total) -----
#pragma unroll
    for (int r = 0; r < R; ++r) merge_lane_groups<LPK>(m[r], l[r], acc[r]);

    // ---- merge the WPU waves of the unit through LDS -------------------------------------------
    if (WPU > 1) {
        float* xb = xbuf;  // [(WPU-1)][R][2 + D]
        if (wv > 0 && ks == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float* p = xb + ((wv - 1) * R + r) * (2 + D);
                if (sub == 0) {
                    p[0] = m[r];
                    p[1] = l[r];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) p[2 + sub * 8 + j] = acc[r][j];
            }
        }
        __syncthreads();
        if (wv > 0) return;
#pragma unroll
        for (int w = 1; w < WPU; ++w)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float* p = xb + ((w - 1) * R + r) * (2 + D);
                float a2[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) a2[j] = p[2 + sub * 8 + j];
                merge_state(m[r], l[r], acc[r], p[0], p[1], a2);
            }
    }

    // ---- epilogue: normalise, merge with the prefix partials (attention.py:21-43), store -------
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        if (row >= a.rows || ks != (r % KPI)) continue;
        const int iq = a.nq == 1 ? 0 : row / a.g, gq = a.nq == 1 ? row : row % a.g;
        const int64_t ridx = ((int64_t)b * a.nq + iq) * a.Hq + hk * a.g + gq;  // [B, nq, Hq]
        finish_row<T, D, 4, NPRE>(a, ridx, sub, m[r], l[r], acc[r], npre, pp[r / KPI]);
    }
}

}  // namespace hyd
