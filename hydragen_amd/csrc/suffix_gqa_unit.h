// What the matrix-core suffix kernels share around their K/V streams: the 16-bit kernel (suffix_gqa_kernel.h, plain and causal-tail)
// and the fp8 kernel (suffix_attn_gqa_fp8.hip) differ in the way from HBM to the MFMA operands -- tiles, DMA geometry, steps in flight,
// collect -- and keep that to themselves.  The lane's query row, the prefix partials, the softmax step on a collected tile, the
// four-wave merge, the epilogue and the launch are ONE text, here, so the numerics rules (the -inf guards, the keys-only LSE) and the
// hipcc wait discipline around the loads the compiler cannot see are fixed in one place.  Plain function templates on the lane's
// state (o, m_run, l_run, the pre-partial buffers) by reference; every one is inlined into its kernel.
// The cut of the pieces is the one at which every instantiation keeps the parent's scratch, spills, occupancy, LDS, load and wait
// counts (profiles/gqa_unit_frame.md): the two loops over a wave's partials stay written out in the kernels, around the pieces here.
#pragma once
#include "suffix_gqa_common.h"

namespace hyd {

namespace {

// partials of a wave requested in front of the stream (a split level's two slices at C5; 2 of 4 at C3)
template <int D>
constexpr int gqa_npre() { return D == 256 ? 1 : 2; }

// ---- this lane's query row (B operand of S^T = K Q^T: column = row l15, 8 dims of every 32-dim chunk) ----
// back (CT, the causal tail): the newest keys this row's token does not see
template <int D, bool CT>
__device__ __forceinline__ void gqa_load_query(const SuffixArgs& a, int b, int hk, int row0, int l15, int g4, bool& rvalid, int64_t& ridx,
                                               int& back, u32x4 (&qf)[D / 32]) {
    const int row = row0 + l15;
    rvalid = row < a.rows;
    const int iq = a.nq == 1 ? 0 : (rvalid ? row / a.g : 0), gq = a.nq == 1 ? (rvalid ? row : 0) : (rvalid ? row % a.g : 0);
    ridx = ((int64_t)b * a.nq + iq) * a.Hq + hk * a.g + gq;  // [B, nq, Hq]
    back = CT && rvalid ? a.nq - 1 - iq : 0;
    const uint16_t* qr = static_cast<const uint16_t*>(a.q) + ridx * D + 8 * g4;
#pragma unroll
    for (int c = 0; c < D / 32; ++c) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        qf[c] = rvalid ? *reinterpret_cast<const u32x4*>(qr + 32 * c) : z;
    }
}

// ---- prefix partials (attention.py:21-43) are dealt to the unit's waves: wave w folds partials w, w + WPU, ... into
// its own (m, l, O) state -- a normalised partial (O_p, lse_p) IS a state (m = lse_p * log2 e, l = 1, O = O_p) -- and the
// merge of the waves then combines everything; no partial is left for the final epilogue.  The wave's first TWO partials (16-bit,
// fp32, or a split level's fp32 slices) are requested in front of the K/V stream and folded when the first key step
// has landed; the others are fetched behind the loop, two per round trip.  (hipcc counts only its own loads.  A plain load
// that is still pending inside the loop makes it insert counted waits that also wait for the next step's DMAs, which it
// does not know about -- one plain request before the stream, settled at the first wait, is what stays exact.  Round 5
// tried one partial per key step through an asm-owned register buffer: 1 us at the paper default, nothing at C3 / C5.)
// Not when the suffix pass's own LSE is asked for (a.lse: the unfused form), which needs the keys-only state at the end.

// request one partial in front of the stream.  buf: its row piece of this lane, dims [16 db + 4 g4, +4) as fp32, or as 16-bit in the
// low half
template <int D>
__device__ __forceinline__ void gqa_request_partial(const PartialDev& pd, int64_t ridx, int g4, bool& is_f32, u32x4 (&buf)[D / 16], float& lse) {
    is_f32 = pd.is_f32 != 0;
    lse = pd.lse[ridx];
    if (is_f32) {
        const float* po = static_cast<const float*>(pd.out) + ridx * D + 4 * g4;
#pragma unroll
        for (int db = 0; db < D / 16; ++db) buf[db] = *reinterpret_cast<const u32x4*>(po + 16 * db);
    } else {
        const uint16_t* po = static_cast<const uint16_t*>(pd.out) + ridx * D + 4 * g4;
#pragma unroll
        for (int db = 0; db < D / 16; ++db) {  // (upper half undefined: no move, hence no wait, between the load and its register)
            const u32x2 u = *reinterpret_cast<const u32x2*>(po + 16 * db);
            buf[db] = __builtin_shufflevector(u, u, 0, 1, -1, -1);
        }
    }
}

// folding a prefix partial into this wave's state
template <int D>
__device__ __forceinline__ void gqa_fold(float lse_p, const f32x4 (&x)[D / 16], f32x4 (&o)[D / 16], float& m_run, float& l_run) {
    const float m_p = lse_p * 1.4426950408889634f;
    const float mf = fmaxf(m_run, m_p);
    const float ms = (mf == -INFINITY) ? 0.f : mf;
    const float a1 = fast_exp2(m_run - ms), a2 = fast_exp2(m_p - ms);
    l_run = l_run * a1 + a2;
    m_run = mf;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) o[db] = o[db] * a1 + x[db] * a2;
}

// the pre-requested partials have landed (the caller waited for every outstanding load): fold them
template <typename T, int D>
__device__ __forceinline__ void gqa_fold_pre(int npre, const bool (&pre_f32)[gqa_npre<D>()], u32x4 (&pbuf)[gqa_npre<D>()][D / 16],
                                             float (&plse)[gqa_npre<D>()], f32x4 (&o)[D / 16], float& m_run, float& l_run) {
    using TR = Traits<T>;
    constexpr int NDB = D / 16;
#pragma unroll
    for (int k = 0; k < gqa_npre<D>(); ++k) {
        // opaque: hipcc must not hoist the conversions below (and with them its wait for the request) in front of the stream
        asm volatile("" : "+v"(plse[k]));
#pragma unroll
        for (int db = 0; db < NDB; ++db) asm volatile("" : "+v"(pbuf[k][db]));
        if (k < npre) {
            f32x4 x[NDB];
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const f32x4 xf = __builtin_bit_cast(f32x4, pbuf[k][db]);
                const f32x4 xh = f32x4{TR::lo(pbuf[k][db][0]), TR::hi(pbuf[k][db][0]), TR::lo(pbuf[k][db][1]), TR::hi(pbuf[k][db][1])};
                x[db] = pre_f32[k] ? xf : xh;
            }
            gqa_fold<D>(plse[k], x, o, m_run, l_run);
        }
    }
}

template <typename T, int D>
__device__ __forceinline__ void gqa_widen(const u32x2 (&u)[D / 16], f32x4 (&x)[D / 16]) {
    using TR = Traits<T>;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) x[db] = f32x4{TR::lo(u[db][0]), TR::hi(u[db][0]), TR::lo(u[db][1]), TR::hi(u[db][1])};
}
// one partial's row piece of this lane behind the stream, as fp32
template <typename T, int D>
__device__ __forceinline__ void gqa_fetch(const PartialDev& pd, int64_t ridx, int g4, f32x4 (&x)[D / 16]) {
    constexpr int NDB = D / 16;
    if (pd.is_f32) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            x[db] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(pd.out) + ridx * D + 16 * db + 4 * g4);
    } else {
        u32x2 u[NDB];
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            u[db] = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(pd.out) + ridx * D + 16 * db + 4 * g4);
        gqa_widen<T, D>(u, x);
    }
}

// ---- one collected 32-key step: kf / vf hold the step's K rows (A operand) and V^T fragments as 16-bit values ----
// a step that reaches past the segment's keys: zero the V rows of keys >= seg_len (dword w of a V^T fragment holds keys
// key0 + 4 g4 + {0,1} / {2,3} / 16 + {0,1} / 16 + {2,3}, the first in its low half)
template <int D>
__device__ __forceinline__ void gqa_sanitize(int key0, int g4, int seg_len, u32x4 (&vf)[D / 16]) {
    const int kb = key0 + 4 * g4;
    unsigned msk[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int ka = kb + (w >> 1) * 16 + (w & 1) * 2;
        msk[w] = (ka < seg_len ? 0x0000ffffu : 0u) | (ka + 1 < seg_len ? 0xffff0000u : 0u);
    }
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
#pragma unroll
        for (int w = 0; w < 4; ++w) vf[db][w] &= msk[w];
}

// S^T = K Q^T and the step's masked scores: p[i] is key key0 + 4 g4 + i, p[4 + i] key key0 + 16 + 4 g4 + i, of query row l15, in
// log2 units; returns the row's maximum over the 32 keys.  CT: the row sees the keys below seg_len - back (the launcher sends no
// shared segment with CT: seg_len = len).
template <typename T, int D, bool CT>
__device__ __forceinline__ float gqa_scores(int key0, int g4, int seg_len, int back, float sc, const u32x4 (&kf)[2][D / 32],
                                            const u32x4 (&qf)[D / 32], float (&p)[8]) {
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < D / 32; ++c) {
        mfma16_acc<T>(s0, kf[0][c], qf[c]);
        mfma16_acc<T>(s1, kf[1][c], qf[c]);
    }
    // the MFMAs above are asm: hipcc's hazard recogniser does not see that their results need the pipeline drained
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(s0), "+v"(s1));
    const int kb = key0 + 4 * g4;
    int lim = seg_len;
    if constexpr (CT) lim = seg_len - back;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        p[i] = (kb + i < lim) ? s0[i] * sc : -INFINITY;
        p[4 + i] = (kb + 16 + i < lim) ? s1[i] * sc : -INFINITY;
    }
    const float tmax = fmaxf(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])), fmaxf(fmaxf(p[4], p[5]), fmaxf(p[6], p[7])));
    return quad_max(tmax);
}

// online softmax in base 2: p -> the step's weights (packed into pf, the B operand of O^T += V^T P^T), (m_run, l_run) updated;
// returns the factor the accumulators are rescaled by.  The new maximum is finite: key0 < len guarantees one valid key per row.
// CT: not guaranteed -- a row with no visible key in this wave's tiles so far keeps m_run = -inf (suffix_gqa_kernel.h) -- and guarded.
template <typename T, bool CT>
__device__ __forceinline__ float gqa_softmax_update(float tmax, float (&p)[8], float& m_run, float& l_run, u32x4& pf) {
    using TR = Traits<T>;
    const float m_max = fmaxf(m_run, tmax);
    const float m_new = (CT && m_max == -INFINITY) ? 0.f : m_max;
    const float alpha = fast_exp2(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        p[i] = fast_exp2(p[i] - m_new);
        ps += p[i];
    }
    ps = quad_sum(ps);
    l_run = l_run * alpha + ps;
    m_run = m_max;
    pf = u32x4{TR::pack2(p[0], p[1]), TR::pack2(p[2], p[3]), TR::pack2(p[4], p[5]), TR::pack2(p[6], p[7])};
    return alpha;
}

// O^T = alpha O^T + V^T P^T
template <typename T, int D>
__device__ __forceinline__ void gqa_pv(float alpha, const u32x4& pf, const u32x4 (&vf)[D / 16], f32x4 (&o)[D / 16]) {
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
        o[db] *= alpha;
        mfma16_acc<T>(o[db], vf[db], pf);
    }
    // the accumulators are read by plain VALU code next (the rescale of the next step, a fold, the epilogue): drain the matrix pipeline
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
}

// ---- merge the WPU waves of the unit: every wave leaves (m, l, O^T) in a 16-row x D float tile of its own (`mine`; tile_of(w) finds
// wave w's), wave 0 folds them.  (m_s, l_s): the wave's keys-only state, merged into (ms_run, ls_run) for the LSE output.
// False for the waves that are done.
template <int D, int WPU, typename TileOf>
__device__ __forceinline__ bool gqa_merge_waves(int wave, int l15, int g4, float* mine, TileOf tile_of, float (*mlx)[4][16], float m_s,
                                                float l_s, f32x4 (&o)[D / 16], float& m_run, float& l_run, float& ms_run, float& ls_run) {
    // lane (row l15, key group g4) holds O^T[d = 16 db + 4 g4 + i][row l15] in o[db][i]; m / l are equal over g4
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
        *reinterpret_cast<f32x4*>(mine + l15 * D + 16 * db + 4 * g4) = o[db];
    if (g4 == 0) {
        mlx[wave][0][l15] = m_run;
        mlx[wave][1][l15] = l_run;
        mlx[wave][2][l15] = m_s;
        mlx[wave][3][l15] = l_s;
    }
    __syncthreads();
    if (wave != 0) return false;
#pragma unroll
    for (int w = 1; w < WPU; ++w) {
        const float* oth = tile_of(w);
        const float m2 = mlx[w][0][l15], l2 = mlx[w][1][l15];
        const float mf = fmaxf(m_run, m2);
        const float ms = (mf == -INFINITY) ? 0.f : mf;
        const float a1 = fast_exp2(m_run - ms), a2 = fast_exp2(m2 - ms);
        // (the two sums of two products are contracted by hand, the way hipcc contracted them while each kernel had its own copy of
        // this text: the other wave's product rounded, this wave's fused in.  Left to hipcc the keys-only sum came out unfused here.)
        l_run = __builtin_fmaf(l_run, a1, l2 * a2);
        m_run = mf;
        const float m3 = mlx[w][2][l15], l3 = mlx[w][3][l15];
        const float mg = fmaxf(ms_run, m3);
        const float mgs = (mg == -INFINITY) ? 0.f : mg;
        ls_run = __builtin_fmaf(ls_run, fast_exp2(ms_run - mgs), l3 * fast_exp2(m3 - mgs));
        ms_run = mg;
#pragma unroll
        for (int db = 0; db < D / 16; ++db) o[db] = o[db] * a1 + *reinterpret_cast<const f32x4*>(oth + l15 * D + 16 * db + 4 * g4) * a2;
        asm volatile("" ::: "memory");  // one wave's tile at a time: hoisting all three costs 96 registers
    }
    return true;
}

// ---- epilogue: the keys-only LSE, then normalise and store (the prefix partials are already in) ----
template <typename T, int D>
__device__ __forceinline__ void gqa_epilogue(const SuffixArgs& a, bool rvalid, int64_t ridx, int g4, const f32x4 (&o)[D / 16], float l_run,
                                             float ms_run, float ls_run) {
    using TR = Traits<T>;
    if (!rvalid) return;
    if (a.lse && g4 == 0) a.lse[ridx] = ls_run > 0.f ? ms_run * kLn2 + __logf(ls_run) : -INFINITY;
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
        const f32x4 x = o[db] * inv;
        const u32x2 pk = {TR::pack2(x[0], x[1]), TR::pack2(x[2], x[3])};
        *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(a.out) + ridx * D + 16 * db + 4 * g4) = pk;
    }
}

// ---- host: launch Kern with `lds` bytes of dynamic LDS.  raise: the launch needs more than the default dynamic-LDS limit, which is
// raised to `limit` once per DEVICE and instantiation (the statics belong to this function's instantiation, one per kernel) -- the
// attribute belongs to the function as loaded on the current device, and a process may launch on several.
template <auto Kern, typename Args>
static int gqa_launch_lds(const Args& args, dim3 grid, int threads, size_t lds, bool raise, int limit, hipStream_t s) {
    if (raise) {
        static hipError_t attr_rc[16];
        static bool attr_set[16];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return (int)hipErrorInvalidDevice;
        if (!__atomic_load_n(&attr_set[dev], __ATOMIC_ACQUIRE)) {  // idempotent: two threads racing both set the same value
            attr_rc[dev] = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, limit);
            __atomic_store_n(&attr_set[dev], true, __ATOMIC_RELEASE);
        }
        if (attr_rc[dev] != hipSuccess) return (int)attr_rc[dev];
    }
    hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, s, args);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace hyd
