// The matrix-core suffix kernel of suffix_attn_gqa.hip (the design notes are there) and its launcher, in a header so that
// suffix_attn_causal.hip can instantiate the causal-tail form without touching the instantiations of suffix_attn_gqa.hip.  What is
// written out here is the 16-bit K/V stream: the LDS layout, the DMA geometry and swizzles, issue / collect, the steps in flight with
// their counted waits, and the two-segment walk.  The lane's query row, the prefix partials, the softmax step on a collected tile, the
// four-wave merge, the epilogue and the raise-the-LDS-limit launch are suffix_gqa_unit.h's, shared with the fp8 kernel.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "suffix_gqa_unit.h"

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
// gqa_softmax_update() (suffix_gqa_unit.h) therefore guards the -inf maximum in every CT instantiation, unconditionally -- it must
// stay; such a state merges as (m = -inf, l = 0), and a row without any key ends as zeros with lse = -inf.
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

    bool rvalid;
    int64_t ridx;
    [[maybe_unused]] int back;
    u32x4 qf[NCH];
    gqa_load_query<D, CT>(a, b, hk, row0, l15, g4, rvalid, ridx, back, qf);

    // ---- prefix partials: dealt to the unit's waves, the wave's first NPRE requested in front of the K/V stream (suffix_gqa_unit.h) ----
    // (this loop and the one behind the stream are written out: as functions of the header they moved hipcc's own waits and grew
    // the D = 64 kernels by more than 1 %, profiles/gqa_unit_frame.md)
    const int np = a.n_partials;
    constexpr int NPRE = gqa_npre<D>();
    const int npre = a.lse != nullptr ? 0 : min(NPRE, (np - wave + WPU - 1) / WPU);  // (np <= wave: 0)
    bool pre_folded = npre <= 0;
    bool pre_f32[NPRE];
    u32x4 pbuf[NPRE][NDB];
    float plse[NPRE];
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
        pre_f32[k] = false;
        plse[k] = -INFINITY;
#pragma unroll
        for (int db = 0; db < NDB; ++db) pbuf[k][db] = u32x4{0u, 0u, 0u, 0u};
        if (k < npre) gqa_request_partial<D>(a.partials[wave + k * WPU], ridx, g4, pre_f32[k], pbuf[k], plse[k]);
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
    // compute: S^T = K Q^T, online softmax, O^T += V^T P^T, all from registers (gqa_sanitize / gqa_compute, suffix_gqa_unit.h)
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
    // (a lambda around the three pieces: called straight from the loop, hipcc grows the bf16 kernels by more than 1 %)
    auto compute = [&](int key0) __attribute__((always_inline)) {
        float p[8];
        u32x4 pf;
        const float tmax = gqa_scores<T, D, CT>(key0, g4, seg_len, back, sc, kf, qf, p);
        const float alpha = gqa_softmax_update<T, CT>(tmax, p, m_run, l_run, pf);
        gqa_pv<T, D>(alpha, pf, vf, o);
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
        if (!pre_folded) {  // the pre-requested partials have landed
            gqa_fold_pre<T, D>(npre, pre_f32, pbuf, plse, o, m_run, l_run);
            pre_folded = true;
        }
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
            if (key0 + 32 > seg_len) gqa_sanitize<D>(key0, g4, seg_len, vf);
            if (j + NSET < nst) issue(key0 + NSET * stride, so);  // in flight while steps j (and j + 1) are computed
            compute(key0);
        }
    }
    // the keys-only state (the LSE output is the suffix pass's own; when it is asked for, no partial was folded above)
    const float m_s = m_run, l_s = l_run;

    // ---- this wave's other partials (all of them when the LSE output is asked for) ----
    for (int i = wave + max(npre, 0) * WPU; i < np; i += 2 * WPU) {
        // two partials per round trip: their lse values and 2 * D/16 row pieces are all requested before the first use
        const bool two = i + WPU < np;
        const int i1 = two ? i + WPU : i;
        const float lse0 = a.partials[i].lse[ridx];
        const float lse1 = two ? a.partials[i1].lse[ridx] : -INFINITY;
        f32x4 x0[NDB], x1[NDB];
        gqa_fetch<T, D>(a.partials[i], ridx, g4, x0);
        gqa_fetch<T, D>(a.partials[i1], ridx, g4, x1);
        gqa_fold<D>(lse0, x0, o, m_run, l_run);
        gqa_fold<D>(lse1, x1, o, m_run, l_run);
    }

    // ---- merge the WPU waves of the unit through their V tiles ----
    float ms_run = m_s, ls_run = l_s;
    if constexpr (WPU > 1) {
        auto tile_of = [&](int w) { return reinterpret_cast<const float*>(tiles[w][0][1]); };
        if (!gqa_merge_waves<D, WPU>(wave, l15, g4, reinterpret_cast<float*>(vtile), tile_of, mlx, m_s, l_s, o, m_run, l_run, ms_run, ls_run)) return;
    }
    gqa_epilogue<T, D>(a, rvalid, ridx, g4, o, l_run, ms_run, ls_run);
}

template <typename T, int D, int WPU, bool NT, int HPW>
static int launch_gqa_k(const SuffixArgs& a, dim3 grid, size_t pad, hipStream_t s) {
    constexpr int NWV = WPU * HPW;
    // the K/V landing tiles, plus the (m, l) exchange area that only the cross-wave merge of WPU > 1 touches: one-wave units ask
    // for the tiles alone, which is at most 64 KB for every shape picked from shapes (HPW = 4 at D = 128, HPW = 2 at D = 256)
    constexpr size_t lds = (size_t)NWV * (D == 64 ? 2 : 1) * 2 * 32 * D * 2 + (WPU > 1 ? (size_t)NWV * 4 * 16 * sizeof(float) : 0);
    // more than the default dynamic-LDS limit (four-wave units; development pads): raised to 150 KiB
    return gqa_launch_lds<HYD_GQA_KERNEL<T, D, WPU, NT, HPW>>(a, grid, 64 * NWV, lds + pad, lds + pad > 64 * 1024, 150 * 1024, s);
}

}  // namespace hyd
