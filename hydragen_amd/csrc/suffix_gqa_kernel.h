// The matrix-core suffix kernel of suffix_attn_gqa.hip (the design notes are there): its body, the kernels that wrap it and their launcher,
// in a header so that suffix_attn_causal.hip can instantiate the causal-tail form without touching the instantiations of suffix_attn_gqa.hip.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "suffix_gqa_common.h"

namespace hyd {

// WPU: waves per unit.  1: a one-wave workgroup per unit (producer and consumer of the LDS tile are the same wave, no
// barriers).  4: the unit's 32-key steps are dealt round-robin to the 4 waves of a 256-thread workgroup and their
// (m, l, O) merged through LDS at the end -- for shapes with too few units to fill the chip with one wave each (C3: 1024
// units on 256 CUs, C5: 2048), where nothing but more waves hides the per-step load latency.
// NT: K/V loads carry the non-temporal hint (suffix_gqa_common.h): the unique phase, where every key is read once.
// HPW: kv heads per workgroup (WPU = 1 only).  The HPW one-wave units of a workgroup are the kv heads hk0 .. hk0 + HPW - 1 of ONE
// sequence: they start together, have the same length and walk the same tokens, so the 2 D-byte pieces they read of every
// token's [Hkv, D] row are requested together (the one-wave workgroups of a sequence's heads are B workgroups apart in
// dispatch order).  No wave talks to another.  Chosen from shapes in launch_gqa_t (measurements there).
// CT: causal tail (hyd_suffix_attn_causal_fwd, hyd_decode_params.causal_tail): the nq query tokens of a sequence are its LAST nq
// tokens and their keys are already in the cache, so token iq sees the keys below len - (nq - 1 - iq) -- a per-ROW key limit in
// the score mask, nothing else.  With len >= nq every row's limit is at least 1: key 0 stays visible to every row, so the wave
// that walks the tile with key 0 -- the only wave of a one-wave unit -- has a finite running maximum from its first tile on, as
// in the plain form.  That does NOT hold for every wave: with four waves per unit wave w starts at key 32 w, and a tile that
// begins below len can lie wholly beyond a row's limit (len = 33, nq = 8: row 0 sees keys < 26, wave 1 starts at key 32), so a
// row's maximum in that wave is -inf until the merge; so is every row's whose sequence is shorter than nq.  The rescale in
// compute() therefore guards the -inf maximum in every CT instantiation, unconditionally -- it must stay; such a state merges as
// (m = -inf, l = 0), and a row without any key ends as zeros with lse = -inf.
// The including source picks the form with HYD_SUFFIX_CAUSAL_TAIL (one form per translation unit): the plain kernel keeps the name,
// the template arguments and the text it has always had, so the instantiations of suffix_attn_gqa.hip compile as before.
#ifndef HYD_SUFFIX_CAUSAL_TAIL
#define HYD_SUFFIX_CAUSAL_TAIL 0
#endif
#if HYD_SUFFIX_CAUSAL_TAIL
#define HYD_GQA_KERNEL suffix_attn_gqa_causal_kernel
#else
#define HYD_GQA_KERNEL suffix_attn_gqa_kernel
#endif
template <typename T, int D, int WPU, bool NT, int HPW = 1>
__global__ __launch_bounds__(64 * WPU * HPW) __attribute__((amdgpu_waves_per_eu(D == 256 ? 1 : 2, D == 256 ? 1 : 2))) void HYD_GQA_KERNEL(const SuffixArgs a) {
    constexpr bool CT = HYD_SUFFIX_CAUSAL_TAIL != 0;
    static_assert(WPU == 1 || HPW == 1, "several heads per workgroup: one-wave units only");
    constexpr int NWV = WPU * HPW;  // waves per workgroup
    // every field a wave needs (and partials[0]) sits in the first 256 bytes of SuffixArgs: one scalar-cache miss at the start of
    // a unit's dependent chain (C5 slice 7.17 -> 7.00 us at S = 16, 25.6 -> 24.9 at S = 128 in an A/B within one run; the dot-product
    // kernel, whose 32768 waves all pay the four extra loads, lost 2-7 % at S <= 4 with it and does not have it)
    warm_kernargs_256();
    using TR = Traits<T>;
    constexpr int RB = D * 2;        // bytes per K/V row
    constexpr int NCH = D / 32;      // 32-dim chunks of the QK^T contraction
    constexpr int NDB = D / 16;      // 16-wide d blocks of O^T
    constexpr int RPI = 1024 / RB;   // rows per DMA instruction
    constexpr int NVD = 32 / RPI;    // DMA instructions per 32-key tile
    constexpr int TILE = 32 * RB;    // bytes of one 32-key tile (= 16 rows * D floats: reused by the merge)
    // NSET tile sets per wave = key steps in flight.  A 32-key step is 2 x 4 KB at D = 64 -- half of what a D = 128 wave keeps in
    // flight, and the kernel is bound by exactly that (profiles/r06_head_dim_rates.txt: 4.9-5.7 TB/s at D = 64 against 5.6-6.1 at
    // 128) -- so D = 64 keeps TWO steps in flight: step j + 2 is requested into the set step j has just been read out of.
    constexpr int NSET = D == 64 ? 2 : 1;
    constexpr unsigned SETB = 2 * TILE;  // bytes of one set (K tile, V tile)
    // dynamic LDS: per wave one K and one V landing tile, then the merge's [NWV][4][16] floats
    extern __shared__ __attribute__((aligned(1024))) char gqa_smem[];
    char(*tiles)[NSET][2][TILE] = reinterpret_cast<char(*)[NSET][2][TILE]>(gqa_smem);  // [wave][set][0 = K, 1 = V]
    float(*mlx)[4][16] = reinterpret_cast<float(*)[4][16]>(gqa_smem + NWV * NSET * 2 * TILE);
    const int wv = NWV == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave of the workgroup
    const int wave = WPU == 1 ? 0 : wv;                                                      // wave of the unit
    char* ktile = tiles[wv][0][0];
    char* vtile = tiles[wv][0][1];

    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g4 = lane >> 4;
    // workgroup -> (sequence, kv-head group): blockIdx.x runs over B * (Hkv / HPW) pairs, sequences fastest
    const int hkg = (int)blockIdx.x / a.B;
    const int bslot = (int)blockIdx.x - hkg * a.B;
    const int b = a.order ? a.order[bslot] : bslot;  // dispatch slot -> sequence (hyd_suffix_params.seq_order)
    const int hk = hkg * HPW + (HPW == 1 ? 0 : wv), row0 = blockIdx.y * 16;

    // the sequence's length is requested first (a scalar load): q and the first partials are requested under its round trip, the first
    // key step goes out when it arrives
    int len_raw = a.kv_len;
    if (a.sl32) len_raw = a.sl32[b];
    else if (a.sl64) len_raw = (int)a.sl64[b];

    // ---- this lane's query row (B operand of S^T = K Q^T: column = row l15, 8 dims of every 32-dim chunk) ----
    const int row = row0 + l15;
    const bool rvalid = row < a.rows;
    const int iq = a.nq == 1 ? 0 : (rvalid ? row / a.g : 0), gq = a.nq == 1 ? (rvalid ? row : 0) : (rvalid ? row % a.g : 0);
    const int64_t ridx = ((int64_t)b * a.nq + iq) * a.Hq + hk * a.g + gq;  // [B, nq, Hq]
    [[maybe_unused]] const int back = CT && rvalid ? a.nq - 1 - iq : 0;  // CT: the newest keys this row's token does not see
    u32x4 qf[NCH];
    {
        const uint16_t* qr = static_cast<const uint16_t*>(a.q) + ridx * D + 8 * g4;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            qf[c] = rvalid ? *reinterpret_cast<const u32x4*>(qr + 32 * c) : z;
        }
    }

    // ---- prefix partials (attention.py:21-43) are dealt to the unit's waves: wave w folds partials w, w + WPU, ... into
    // its own (m, l, O) state -- a normalised partial (O_p, lse_p) IS a state (m = lse_p * log2 e, l = 1, O = O_p) -- and the
    // merge of the waves then combines everything; no partial is left for the final epilogue.  The wave's first TWO partials (16-bit,
    // fp32, or a split level's fp32 slices) are requested here, in front of the K/V stream, and folded when the first key step
    // has landed; the others are fetched behind the loop, two per round trip.  (hipcc counts only its own loads.  A plain load
    // that is still pending inside the loop makes it insert counted waits that also wait for the next step's DMAs, which it
    // does not know about -- one plain request before the stream, settled at the first wait, is what stays exact.  Round 5
    // tried one partial per key step through an asm-owned register buffer: 1 us at the paper default, nothing at C3 / C5.)
    // Not when the suffix pass's own LSE is asked for (a.lse: the unfused form), which needs the keys-only state at the end.
    const int np = a.n_partials;
    constexpr int NPRE = D == 256 ? 1 : 2;  // partials of this wave requested in front of the stream (a split level's two slices at C5; 2 of 4 at C3)
    const int npre = a.lse != nullptr ? 0 : min(NPRE, (np - wave + WPU - 1) / WPU);  // (np <= wave: 0)
    bool pre_folded = npre <= 0;
    bool pre_f32[NPRE];
    u32x4 pbuf[NPRE][NDB];  // a partial's row piece of this lane: dims [16 db + 4 g4, +4) as fp32, or as 16-bit in the low half
    float plse[NPRE];
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
        pre_f32[k] = false;
        plse[k] = -INFINITY;
#pragma unroll
        for (int db = 0; db < NDB; ++db) pbuf[k][db] = u32x4{0u, 0u, 0u, 0u};
        if (k < npre) {
            const PartialDev& pd = a.partials[wave + k * WPU];
            pre_f32[k] = pd.is_f32 != 0;
            plse[k] = pd.lse[ridx];
            if (pre_f32[k]) {
                const float* po = static_cast<const float*>(pd.out) + ridx * D + 4 * g4;
#pragma unroll
                for (int db = 0; db < NDB; ++db) pbuf[k][db] = *reinterpret_cast<const u32x4*>(po + 16 * db);
            } else {
                const uint16_t* po = static_cast<const uint16_t*>(pd.out) + ridx * D + 4 * g4;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {  // (upper half undefined: no move, hence no wait, between the load and its register)
                    const u32x2 u = *reinterpret_cast<const u32x2*>(po + 16 * db);
                    pbuf[k][db] = __builtin_shufflevector(u, u, 0, 1, -1, -1);
                }
            }
        }
    }

    // ---- K / V windows of this unit: rows [0, len) are in range, everything else reads as zero ------------------
    // The windows are BUILT over the cache's kv_len rows and cut to the sequence's length (learn_len, below) before the first step is
    // requested: no row in [len, kv_len) is fetched, a step that reaches past the length is zero-filled by the address check.  What
    // those rows hold -- NaN, or finite keys with enormous scores (tests/test_softmax_stress_gpu.py, spike_behind_length) -- cannot
    // reach the maximum or the sums; the zero-filled tail of the last step still has its scores replaced by -inf (a select, not
    // arithmetic) and its V rows zeroed in registers (sanitize, masked steps only).
    const unsigned k_ts2 = (unsigned)(a.k_ts * 2), v_ts2 = (unsigned)(a.v_ts * 2);
    const u32x4 krs = make_rsrc_g(static_cast<const uint16_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)hk * a.k_hs, (unsigned)a.kv_len * k_ts2);
    const u32x4 vrs = make_rsrc_g(static_cast<const uint16_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hk * a.v_hs, (unsigned)a.kv_len * v_ts2);
    // Tiny problems (SuffixArgs::pk): the group's shared prefix is walked first, through its own resources, then the
    // unit's own keys -- the (m, l, O) state simply carries over, and the whole operator is this one launch.
    const bool has_pre = a.pk != nullptr;
    const int gi = has_pre ? b / a.p_per : 0;
    const u32x4 krs_p = make_rsrc_g(static_cast<const uint16_t*>(has_pre ? a.pk : a.k) + (int64_t)gi * a.pk_gs + (int64_t)hk * a.pk_hs,
                                    has_pre ? (unsigned)a.p_len * k_ts2 : 0u);
    const u32x4 vrs_p = make_rsrc_g(static_cast<const uint16_t*>(has_pre ? a.pv : a.v) + (int64_t)gi * a.pv_gs + (int64_t)hk * a.pv_hs,
                                    has_pre ? (unsigned)a.p_len * v_ts2 : 0u);
    u32x4 krs_c = krs, vrs_c = vrs;  // the segment being walked
    int seg_len = 0, seg_cap = 0;  // keys of the segment being walked; rows its window addresses
    // K and V DMA: instruction i covers tile rows [i * RPI, +RPI) -- whole rows, 1 KiB contiguous when the heads of a token are
    // (Hkv = 1), RPI row pieces of 2 D bytes otherwise; the LDS image of an instruction is lane-linear, so the XOR swizzles of
    // the two tiles are applied to the per-lane SOURCE chunk (involutions inside a row).
    //   K tile: 16-byte chunk j of row r sits at position j ^ sw_k(r) -- the A-operand reads below (16 rows, one chunk
    //           column per quarter wave) then touch every bank once;  sw_k(r) = r & 15 (D >= 128), (r >> 1) & 7 (D = 64)
    //   V tile: 64-byte groups swizzled for the transposing reads (as before)
    const int drow = (lane * 16) / RB, dcp = ((lane * 16) % RB) >> 4;
    unsigned kvoff[NVD], vvoff[NVD];
#pragma unroll
    for (int i = 0; i < NVD; ++i) {
        const int r_ = i * RPI + drow;
        const int swk = D >= 128 ? (r_ & 15) : ((r_ >> 1) & 7);
        kvoff[i] = (unsigned)r_ * k_ts2 + (unsigned)(dcp ^ swk) * 16u;
        const int sw = D >= 128 ? (r_ & 3) : ((r_ >> 1) & 1);
        const int vch = (((dcp >> 2) ^ sw) << 2) | (dcp & 3);
        vvoff[i] = (unsigned)r_ * v_ts2 + (unsigned)vch * 16u;
    }
    typedef const __attribute__((address_space(3))) char* lptr_c;
    const unsigned kt0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_c)ktile);
    const unsigned vt0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_c)vtile);
    // K fragment (A operand of S^T = K Q^T): key = 16 h + l15, dims 32 c + 8 g4 .. + 8 = chunk 4 c + g4 of the row
    unsigned kaddr[2];  // byte address of chunk position 0 of this lane's row, key half h; the chunk's position is XORed in per read
    const int kswz = D >= 128 ? l15 : ((l15 >> 1) & 7);  // sw_k of rows l15 and 16 + l15 alike
#pragma unroll
    for (int h = 0; h < 2; ++h) kaddr[h] = (unsigned)(uintptr_t)(lptr_c)(ktile + (16 * h + l15) * RB);
    // V^T fragment (A operand of O^T += V^T P^T): d = 16 db + l15, keys {4 g4 + j} (half 0) / {16 + 4 g4 + j} (half 1);
    // the 16-lane group reads the 4 x 16 block, lane l15 supplies row l15 >> 2, columns 4 (l15 & 3) .. + 4
    const int trow = 4 * g4 + (l15 >> 2);
    const int tsw = D >= 128 ? (trow & 3) : ((trow >> 1) & 1);
    unsigned vaddr[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
        vaddr[db] = (unsigned)(uintptr_t)(lptr_c)(vtile + trow * RB + (((db >> 1) ^ tsw) << 6) + 32 * (db & 1) + 8 * (l15 & 3));

    f32x4 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const float sc = a.scale_log2e;

    // ---- one 32-key step --------------------------------------------------------------------------------------------------
    // issue:   2 NVD LDS-DMA instructions, K rows -> K tile, V rows -> V tile (zero fill past the segment's end)
    // collect: the landed tiles -> registers (K: 2 NCH ds_read_b128 in the A-operand layout; V^T: 2 NDB transposing reads), after
    //          which both tiles are free for the next step's DMA
    // compute: S^T = K Q^T, online softmax, O^T += V^T P^T, all from registers
    // The loop keeps ONE step in flight per wave while the previous one is computed (collect(j); issue(j + 1); compute(j); head dim 64: TWO, NSET):
    // 16 KiB per wave, 8 waves per CU.  (Round 4's form loaded K straight into MFMA operand layout -- 16 rows x 64 B per
    // instruction, every quarter wave 16 different cache lines -- and ran 10 % below this one on 8-kv-head shapes.)
    u32x4 kf[2][NCH];
    u32x4 vf[NDB];
    // (so: byte offset of the tile set, 0 when there is one)
    auto issue = [&](int key0, unsigned so) __attribute__((always_inline)) {
        const unsigned ksoff = (unsigned)key0 * k_ts2, vsoff = (unsigned)key0 * v_ts2;
#pragma unroll
        for (int i = 0; i < NVD; ++i) dma16_g<NT>(krs_c, kvoff[i], ksoff, kt0 + so + i * 1024);
#pragma unroll
        for (int i = 0; i < NVD; ++i) dma16_g<NT>(vrs_c, vvoff[i], vsoff, vt0 + so + i * 1024);
    };
    auto collect = [&](unsigned so) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                kf[h][c] = *reinterpret_cast<const __attribute__((address_space(3))) u32x4*>((uintptr_t)(kaddr[h] + so + (unsigned)(((4 * c + g4) ^ kswz) << 4)));
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const u32x2 t0 = lds_tr16_g(vaddr[db] + so);
            const u32x2 t1 = lds_tr16_g(vaddr[db] + so + 16 * RB);
            vf[db] = u32x4{t0[0], t0[1], t1[0], t1[1]};
        }
        // every read has returned before the tiles are handed to the next DMA (asm: hipcc does not order it against them otherwise)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // a step that reaches past the segment's keys: zero the V rows of keys >= seg_len (dword w of a V^T fragment holds keys
    // key0 + 4 g4 + {0,1} / {2,3} / 16 + {0,1} / 16 + {2,3}, the first in its low half)
    auto sanitize = [&](int key0) __attribute__((always_inline)) {
        const int kb = key0 + 4 * g4;
        unsigned msk[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int ka = kb + (w >> 1) * 16 + (w & 1) * 2;
            msk[w] = (ka < seg_len ? 0x0000ffffu : 0u) | (ka + 1 < seg_len ? 0xffff0000u : 0u);
        }
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int w = 0; w < 4; ++w) vf[db][w] &= msk[w];
    };
    auto compute = [&](int key0) __attribute__((always_inline)) {
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            mfma16_acc<T>(s0, kf[0][c], qf[c]);
            mfma16_acc<T>(s1, kf[1][c], qf[c]);
        }
        // the MFMAs above are asm: hipcc's hazard recogniser does not see that their results need the pipeline drained
        asm volatile("s_nop 7\n\ts_nop 7" : "+v"(s0), "+v"(s1));
        // scores of this lane: keys key0 + 4 g4 + i (s0) and key0 + 16 + 4 g4 + i (s1), query row l15
        float p[8];
        const int kb = key0 + 4 * g4;
        int lim = seg_len;  // keys of the segment this lane's row sees (CT: the launcher sends no shared segment, seg_len = len)
        if constexpr (CT) lim = seg_len - back;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = (kb + i < lim) ? s0[i] * sc : -INFINITY;
            p[4 + i] = (kb + 16 + i < lim) ? s1[i] * sc : -INFINITY;
        }
        float tmax = fmaxf(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])), fmaxf(fmaxf(p[4], p[5]), fmaxf(p[6], p[7])));
        tmax = quad_max(tmax);
        const float m_max = fmaxf(m_run, tmax);  // finite: key0 < len guarantees one valid key per row (CT: not guaranteed, guarded next)
        const float m_new = (CT && m_max == -INFINITY) ? 0.f : m_max;  // (CT: a row with no visible key in this wave's tiles so far -- see the note at the kernel)
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
        const u32x4 pf = {TR::pack2(p[0], p[1]), TR::pack2(p[2], p[3]), TR::pack2(p[4], p[5]), TR::pack2(p[6], p[7])};
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            o[db] *= alpha;
            mfma16_acc<T>(o[db], vf[db], pf);
        }
        // the accumulators are read by plain VALU code next (the rescale of the next step, a fold, the epilogue): drain the matrix pipeline
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    };

    // ---- folding a prefix partial into this wave's state -----------------------------------------------------------------
    auto fold = [&](float lse_p, const f32x4(&x)[NDB]) __attribute__((always_inline)) {
        const float m_p = lse_p * 1.4426950408889634f;
        const float mf = fmaxf(m_run, m_p);
        const float ms = (mf == -INFINITY) ? 0.f : mf;
        const float a1 = fast_exp2(m_run - ms), a2 = fast_exp2(m_p - ms);
        l_run = l_run * a1 + a2;
        m_run = mf;
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = o[db] * a1 + x[db] * a2;
    };
    auto widen = [&](const u32x2(&u)[NDB], f32x4(&x)[NDB]) __attribute__((always_inline)) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) x[db] = f32x4{TR::lo(u[db][0]), TR::hi(u[db][0]), TR::lo(u[db][1]), TR::hi(u[db][1])};
    };
    auto fetch = [&](const PartialDev& pd, f32x4(&x)[NDB]) __attribute__((always_inline)) {
        if (pd.is_f32) {
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                x[db] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(pd.out) + ridx * D + 16 * db + 4 * g4);
        } else {
            u32x2 u[NDB];
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                u[db] = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(pd.out) + ridx * D + 16 * db + 4 * g4);
            widen(u, x);
        }
    };
    // the pre-requested partials have landed (the caller waited for every outstanding load): fold them
    auto fold_pre = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < NPRE; ++k) {
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
                fold(plse[k], x);
            }
        }
        pre_folded = true;
    };
    int len = 0;
    for (int seg = has_pre ? 0 : 1; seg < 2; ++seg) {  // every segment drains its own pipeline
        constexpr int stride = 32 * WPU;
        const int k_first = wave * 32;
        if (seg == 0) { krs_c = krs_p; vrs_c = vrs_p; seg_cap = a.p_len; }
        else { krs_c = krs; vrs_c = vrs; seg_cap = a.kv_len; }
        // The first step goes out as soon as the sequence's length has arrived (a scalar load: its wait does not touch the vector
        // queue), in front of the wait for q and the first partials, and its windows END at the length: a step that reaches past
        // it is zero-filled by the address check instead of being fetched.  Until round 6 the first step was requested blind --
        // before the length, for whatever the cache's kv_len rows held -- and the windows stayed that wide: every unit read up to 31
        // rows behind its length in its last step (1.166 x the algorithmic bytes at C5's mean suffix of 128.5, FETCH_SIZE in
        // profiles/r06_v4_c5_whole_job.json) and a full 32 rows in the first 31 decode steps of every generation (C5 at S = 20:
        // 368 MB moved for 268 MB).  The round trip the blind step saved is 0.5 us per launch (profiles/r06_gqa_blind_step_ab.txt).
        bool blind = false;
#ifdef HYD_ABLATION_BUILD
        blind = a.dbg_blind != 0;  // HYD_GQA_BLIND=1: the blind first step, windows still cut at the length afterwards (A/B)
#endif
        auto learn_len = [&]() __attribute__((always_inline)) {
            if (seg == 1) {
                len = max(0, min(len_raw, a.kv_len));
                krs_c[2] = __builtin_amdgcn_readfirstlane((unsigned)len * k_ts2);
                vrs_c[2] = __builtin_amdgcn_readfirstlane((unsigned)len * v_ts2);
            }
            seg_len = seg == 0 ? a.p_len : len;
        };
        int nst = 0;  // 32-key steps of this wave
        if (blind) {
            if (seg_cap > k_first) issue(k_first, 0u);
        } else {
            learn_len();
            nst = seg_len > k_first ? (seg_len - k_first + stride - 1) / stride : 0;
            if (nst > 0) issue(k_first, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... all landed
        // hipcc counts only its own loads (q, the first partials): make it settle them HERE, where nothing is in flight -- a
        // counted wait of its own further down would also wait for the next step's DMAs, which it does not know about
#pragma unroll
        for (int c = 0; c < NCH; ++c) asm volatile("" ::"v"(qf[c]));
        if (blind) {
            if (seg == 1) asm volatile("" : "+v"(len_raw));
            learn_len();
            nst = seg_len > k_first ? (seg_len - k_first + stride - 1) / stride : 0;
        }
        if (!pre_folded) fold_pre();
        // the second set's first step goes out BEHIND the drain: hipcc's own wait for q and the partials (it lands at the settle point
        // above) is a full one and must not find a key step it does not know about in the queue
        if (NSET == 2 && nst > 1) issue(k_first + stride, SETB);
        for (int j = 0; j < nst; ++j) {
            const int key0 = k_first + j * stride;
            const unsigned so = NSET == 2 ? (unsigned)(j & 1) * SETB : 0u;
            if (j > 0) {  // step j's tiles have landed (requests return in order: with two sets, step j + 1's 2 NVD may stay out)
                if (NSET == 2 && j + 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NVD) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            collect(so);
            if (key0 + 32 > seg_len) sanitize(key0);
            if (j + NSET < nst) issue(key0 + NSET * stride, so);  // in flight while steps j (and j + 1) are computed
            compute(key0);
        }
    }
    // the keys-only state (the LSE output is the suffix pass's own; when it is asked for, no partial was folded above)
    const float m_s = m_run, l_s = l_run;

    // ---- this wave's other partials (all of them when the LSE output is asked for) ---------------------------------------
    for (int i = wave + max(npre, 0) * WPU; i < np; i += 2 * WPU) {
        // two partials per round trip: their lse values and 2 * D/16 row pieces are all requested before the first use
        const bool two = i + WPU < np;
        const int i1 = two ? i + WPU : i;
        const float lse0 = a.partials[i].lse[ridx];
        const float lse1 = two ? a.partials[i1].lse[ridx] : -INFINITY;
        f32x4 x0[NDB], x1[NDB];
        fetch(a.partials[i], x0);
        fetch(a.partials[i1], x1);
        fold(lse0, x0);
        fold(lse1, x1);
    }

    // ---- merge the WPU waves of the unit: every wave leaves (m, l, O^T) in its own V tile, wave 0 folds them -------
    float ms_run = m_s, ls_run = l_s;
    if constexpr (WPU > 1) {
        float* mine = reinterpret_cast<float*>(vtile);  // [16 rows][D]: O (unnormalised)
        // lane (row l15, key group g4) holds O^T[d = 16 db + 4 g4 + i][row l15] in o[db][i]; m / l are equal over g4
#pragma unroll
        for (int db = 0; db < NDB; ++db)
            *reinterpret_cast<f32x4*>(mine + l15 * D + 16 * db + 4 * g4) = o[db];
        if (g4 == 0) {
            mlx[wave][0][l15] = m_run;
            mlx[wave][1][l15] = l_run;
            mlx[wave][2][l15] = m_s;
            mlx[wave][3][l15] = l_s;
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int w = 1; w < WPU; ++w) {
            const float* oth = reinterpret_cast<const float*>(tiles[w][0][1]);
            const float m2 = mlx[w][0][l15], l2 = mlx[w][1][l15];
            const float mf = fmaxf(m_run, m2);
            const float ms = (mf == -INFINITY) ? 0.f : mf;
            const float a1 = fast_exp2(m_run - ms), a2 = fast_exp2(m2 - ms);
            l_run = l_run * a1 + l2 * a2;
            m_run = mf;
            const float m3 = mlx[w][2][l15], l3 = mlx[w][3][l15];
            const float mg = fmaxf(ms_run, m3);
            const float mgs = (mg == -INFINITY) ? 0.f : mg;
            ls_run = ls_run * fast_exp2(ms_run - mgs) + l3 * fast_exp2(m3 - mgs);
            ms_run = mg;
#pragma unroll
            for (int db = 0; db < NDB; ++db) o[db] = o[db] * a1 + *reinterpret_cast<const f32x4*>(oth + l15 * D + 16 * db + 4 * g4) * a2;
            asm volatile("" ::: "memory");  // one wave's tile at a time: hoisting all three costs 96 registers
        }
    }

    // ---- epilogue: normalise and store (the prefix partials are already in) -----------------------------------------
    if (!rvalid) return;
    if (a.lse && g4 == 0) a.lse[ridx] = ls_run > 0.f ? ms_run * kLn2 + __logf(ls_run) : -INFINITY;
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
        const f32x4 x = o[db] * inv;
        const u32x2 pk = {TR::pack2(x[0], x[1]), TR::pack2(x[2], x[3])};
        *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(a.out) + ridx * D + 16 * db + 4 * g4) = pk;
    }
}

template <typename T, int D, int WPU, bool NT, int HPW>
static int launch_gqa_k(const SuffixArgs& a, dim3 grid, size_t pad, hipStream_t s) {
    constexpr int NWV = WPU * HPW;
    // the K/V landing tiles, plus the (m, l) exchange area that only the cross-wave merge of WPU > 1 touches: one-wave units ask
    // for the tiles alone, which is at most 64 KB for every shape picked from shapes (HPW = 4 at D = 128, HPW = 2 at D = 256)
    constexpr size_t lds = (size_t)NWV * (D == 64 ? 2 : 1) * 2 * 32 * D * 2 + (WPU > 1 ? (size_t)NWV * 4 * 16 * sizeof(float) : 0);
    auto kern = HYD_GQA_KERNEL<T, D, WPU, NT, HPW>;
    if (lds + pad > 64 * 1024) {
        // more than the default dynamic-LDS limit (four-wave units; development pads): raise it, once per DEVICE and instantiation --
        // the attribute belongs to the function as loaded on the current device, and a process may launch on several
        static hipError_t attr_rc[16];
        static bool attr_set[16];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return (int)hipErrorInvalidDevice;
        if (!__atomic_load_n(&attr_set[dev], __ATOMIC_ACQUIRE)) {  // idempotent: two threads racing both set the same value
            attr_rc[dev] = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
            __atomic_store_n(&attr_set[dev], true, __ATOMIC_RELEASE);
        }
        if (attr_rc[dev] != hipSuccess) return (int)attr_rc[dev];
    }
    hipLaunchKernelGGL(kern, grid, dim3(64 * NWV), lds + pad, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
