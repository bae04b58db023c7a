// The fp8 matrix-core suffix kernel of suffix_attn_gqa_fp8.hip (the design notes and the contract are there), in a header so that
// suffix_attn_gqa_fp8_causal.hip can instantiate the causal-tail form without touching the instantiations of suffix_attn_gqa_fp8.hip:
// what suffix_gqa_kernel.h is for the 16-bit kernel.  The including source picks the form with HYD_SUFFIX_CAUSAL_TAIL (one form per
// translation unit): the plain kernel keeps the name, the template arguments and the text it has always had.
// The causal tail (CT; the rule and its -inf cases: suffix_gqa_kernel.h) is a per-ROW key limit in the score mask: the row of token iq
// sees the keys below len - (nq - 1 - iq).  What differs from the plain form is `back` at the query load, gqa_scores<T, D, true>, and the
// guard of a row's -inf maximum in gqa_softmax_update<T, true> that every CT instantiation needs (four waves per unit: a wave's tile
// can lie wholly beyond a row's limit; a sequence shorter than nq: a row without any key).  The stream -- DMA geometry, landing sets,
// widening, waits, the windows cut at the sequence's length, gqa_sanitize -- and everything behind it are the same text.
#pragma once
#include <type_traits>

#include "suffix_gqa_unit.h"

#ifndef HYD_SUFFIX_CAUSAL_TAIL
#define HYD_SUFFIX_CAUSAL_TAIL 0
#endif
#if HYD_SUFFIX_CAUSAL_TAIL
#define HYD_GQA_FP8_KERNEL suffix_attn_gqa_fp8_causal_kernel
#else
#define HYD_GQA_FP8_KERNEL suffix_attn_gqa_fp8_kernel
#endif

namespace hyd {

namespace {

// 8 e4m3fn bytes -> 8 values of T (dims 2i, 2i + 1 in dword i), each float(fp8) * s rounded to fp32, then to T: dequantize_kv
template <typename T>
__device__ __forceinline__ u32x4 fp8x8_dequant(const u32x2& v, float s) {
    using TR = Traits<T>;
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], true);
        r[2 * i] = TR::pack2(lo[0] * s, lo[1] * s);
        r[2 * i + 1] = TR::pack2(hi[0] * s, hi[1] * s);
    }
    return r;
}

}  // namespace

// WPU, HPW: as in suffix_attn_gqa.hip.  Always the unique phase: the loads carry the non-temporal hint.
template <typename T, int D, int WPU, int HPW = 1>
__global__ __launch_bounds__(64 * WPU * HPW) __attribute__((amdgpu_waves_per_eu(D == 256 ? 1 : 2, D == 256 ? 1 : 2))) void HYD_GQA_FP8_KERNEL(const SuffixKvqArgs ka) {
    constexpr bool CT = HYD_SUFFIX_CAUSAL_TAIL != 0;
    static_assert(WPU == 1 || HPW == 1, "several heads per workgroup: one-wave units only");
    constexpr int NWV = WPU * HPW;  // waves per workgroup
    warm_kernargs_256();
    const SuffixArgs& a = ka.a;
    constexpr int RB8 = D;           // bytes per fp8 K/V row
    constexpr int RB = D * 2;        // bytes per row of the widened V tile
    constexpr int NCH = D / 32;      // 32-dim chunks of the QK^T contraction
    constexpr int NDB = D / 16;      // 16-wide d blocks of O^T
    constexpr int RPI = 1024 / RB8;  // rows per DMA instruction
    constexpr int NVD = 32 / RPI;    // DMA instructions per 32-key tile
    constexpr int TILE8 = 32 * RB8;  // bytes of one 32-key landing tile
    constexpr int TILE = 32 * RB;    // bytes of the widened V tile (= 16 rows * D floats: reused by the merge)
    constexpr int NSET = D <= 128 ? 2 : 1;  // landing-tile sets per wave = key steps in flight
    constexpr unsigned SETB = 2 * TILE8;    // bytes of one set (K tile, V tile)
    constexpr int WB = NSET * (int)SETB + TILE;  // LDS bytes of one wave
    constexpr int NWD = D / 16;      // 8-byte pieces of the V landing tile each lane widens
    // dynamic LDS: per wave NSET landing sets and the widened V tile, then the merge's [NWV][4][16] floats
    extern __shared__ __attribute__((aligned(1024))) char gqa8_smem[];
    float(*mlx)[4][16] = reinterpret_cast<float(*)[4][16]>(gqa8_smem + NWV * WB);
    const int wv = NWV == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave of the workgroup
    const int wave = WPU == 1 ? 0 : wv;                                                      // wave of the unit
    char* ktile = gqa8_smem + wv * WB;      // set 0: K landing tile, then V landing tile
    char* vland = ktile + TILE8;
    char* vtile = ktile + NSET * SETB;      // widened V

    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, g4 = lane >> 4;
    // workgroup -> (sequence, kv-head group): blockIdx.x runs over B * (Hkv / HPW) pairs, sequences fastest
    const int hkg = (int)blockIdx.x / a.B;
    const int bslot = (int)blockIdx.x - hkg * a.B;
    const int b = a.order ? a.order[bslot] : bslot;  // dispatch slot -> sequence (hyd_suffix_params.seq_order)
    const int hk = __builtin_amdgcn_readfirstlane(hkg * HPW + (HPW == 1 ? 0 : wv)), row0 = blockIdx.y * 16;

    int len_raw = a.kv_len;
    if (a.sl32) len_raw = a.sl32[b];
    else if (a.sl64) len_raw = (int)a.sl64[b];
    // the kv head's scales (null = 1), read at run time: a graph replay sees the values of its own moment
    float ksc = ka.k_scale ? ka.k_scale[hk] : 1.0f;
    float vsc = ka.v_scale ? ka.v_scale[hk] : 1.0f;

    // ---- this lane's query row (B operand of S^T = K Q^T: column = row l15, 8 dims of every 32-dim chunk) ----
    // (written out: through gqa_load_query, as in the 16-bit kernel, the one-wave instantiations lost 1.6 % at the C5 whole job)
    const int row = row0 + l15;
    const bool rvalid = row < a.rows;
    const int iq = a.nq == 1 ? 0 : (rvalid ? row / a.g : 0), gq = a.nq == 1 ? (rvalid ? row : 0) : (rvalid ? row % a.g : 0);
    const int64_t ridx = ((int64_t)b * a.nq + iq) * a.Hq + hk * a.g + gq;  // [B, nq, Hq]
    const int back = CT && rvalid ? a.nq - 1 - iq : 0;  // (CT: the newest keys this row's token does not see)
    u32x4 qf[NCH];
    {
        const uint16_t* qr = static_cast<const uint16_t*>(a.q) + ridx * D + 8 * g4;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            qf[c] = rvalid ? *reinterpret_cast<const u32x4*>(qr + 32 * c) : z;
        }
    }

    // ---- prefix partials: dealt to the unit's waves, the wave's first NPRE requested in front of the K/V stream (suffix_gqa_unit.h) ----
    // (this loop and the one behind the stream are written out, as in the 16-bit kernel)
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

    // ---- K / V windows of this unit (strides count bytes): rows [0, len) are in range, everything else reads as zero bytes = +0 ----
    // Built over the cache's kv_len rows here and cut to the sequence's length before the first step is requested (below): no row in
    // [len, kv_len) is fetched, whatever it holds (tests/test_softmax_stress_gpu.py, spike_behind_length).
    const unsigned k_ts = (unsigned)a.k_ts, v_ts = (unsigned)a.v_ts;
    u32x4 krs = make_rsrc_g(static_cast<const uint8_t*>(a.k) + (int64_t)b * a.k_bs + (int64_t)hk * a.k_hs, (unsigned)a.kv_len * k_ts);
    u32x4 vrs = make_rsrc_g(static_cast<const uint8_t*>(a.v) + (int64_t)b * a.v_bs + (int64_t)hk * a.v_hs, (unsigned)a.kv_len * v_ts);
    int seg_len = 0;
    // DMA: instruction i covers tile rows [i * RPI, +RPI), whole D-byte rows; the LDS image of an instruction is lane-linear.
    //   K tile: 16-byte chunk j of row r sits at position j ^ sw_k(r) (applied to the per-lane SOURCE chunk: an involution inside a
    //           row) so that the 16 rows one quarter wave reads of a chunk column are spread over the banks
    //   V tile: plain rows (it is only read lane-linearly, by the widening pass)
    const int drow = (lane * 16) / RB8, dcp = ((lane * 16) % RB8) >> 4;
    unsigned kvoff[NVD], vvoff[NVD];
#pragma unroll
    for (int i = 0; i < NVD; ++i) {
        const int r_ = i * RPI + drow;
        const int swk = D == 64 ? ((r_ >> 1) & 3) : (r_ & (D / 16 - 1));
        kvoff[i] = (unsigned)r_ * k_ts + (unsigned)(dcp ^ swk) * 16u;
        vvoff[i] = (unsigned)r_ * v_ts + (unsigned)dcp * 16u;
    }
    typedef const __attribute__((address_space(3))) char* lptr_c;
    const unsigned kt0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_c)ktile);
    const unsigned vt0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_c)vland);
    // K fragment (A operand of S^T = K Q^T): key = 16 h + l15, dims 32 c + 8 g4 .. + 8 = 8 bytes: half g4 & 1 of chunk 2 c + (g4 >> 1)
    unsigned kaddr[2];
    const int kswz = D == 64 ? ((l15 >> 1) & 3) : (l15 & (D / 16 - 1));  // sw_k of rows l15 and 16 + l15 alike
#pragma unroll
    for (int h = 0; h < 2; ++h) kaddr[h] = (unsigned)(uintptr_t)(lptr_c)(ktile + (16 * h + l15) * RB8) + 8u * (g4 & 1);
    // widening pass over the V landing tile: piece u = i * 64 + lane is row u / (D / 8), dims 8 (u % (D / 8)) .. + 8; it goes to the
    // 16-byte chunk of the same row in the widened tile, at the 16-bit kernel's swizzled position
    const unsigned vsrc = (unsigned)(uintptr_t)(lptr_c)vland + 8u * lane;
    unsigned vdst[NWD];
#pragma unroll
    for (int i = 0; i < NWD; ++i) {
        const int u = i * 64 + lane;
        const int r_ = u / (D / 8), c8 = u % (D / 8);
        const int sw = D >= 128 ? (r_ & 3) : ((r_ >> 1) & 1);
        const int vch = (((c8 >> 2) ^ sw) << 2) | (c8 & 3);
        vdst[i] = (unsigned)(uintptr_t)(lptr_c)(vtile + r_ * RB + vch * 16);
    }
    // V^T fragment out of the widened tile: exactly the 16-bit kernel's reads
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

    u32x4 kf[2][NCH];
    u32x4 vf[NDB];
    // (so: byte offset of the landing set)
    auto issue = [&](int key0, unsigned so) __attribute__((always_inline)) {
        const unsigned ksoff = (unsigned)key0 * k_ts, vsoff = (unsigned)key0 * v_ts;
#pragma unroll
        for (int i = 0; i < NVD; ++i) dma16_g<true>(krs, kvoff[i], ksoff, kt0 + so + i * 1024);
#pragma unroll
        for (int i = 0; i < NVD; ++i) dma16_g<true>(vrs, vvoff[i], vsoff, vt0 + so + i * 1024);
    };
    auto collect = [&](unsigned so) __attribute__((always_inline)) {
        typedef const __attribute__((address_space(3))) u32x2* lds_u32x2_c;
        typedef __attribute__((address_space(3))) u32x4* lds_u32x4_p;
        // V: landing tile -> widened tile (the previous step's transposing reads have returned: its collect waited for them)
#pragma unroll
        for (int i = 0; i < NWD; ++i) {
            const u32x2 raw = *reinterpret_cast<lds_u32x2_c>((uintptr_t)(vsrc + so + (unsigned)i * 512u));
            *reinterpret_cast<lds_u32x4_p>((uintptr_t)vdst[i]) = fp8x8_dequant<T>(raw, vsc);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const u32x2 raw = *reinterpret_cast<lds_u32x2_c>((uintptr_t)(kaddr[h] + so + (unsigned)(((2 * c + (g4 >> 1)) ^ kswz) << 4)));
                kf[h][c] = fp8x8_dequant<T>(raw, ksc);
            }
        // a wave's LDS instructions execute in order: the transposing reads see the widened tile
        asm volatile("" ::: "memory");
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const u32x2 t0 = lds_tr16_g(vaddr[db]);
            const u32x2 t1 = lds_tr16_g(vaddr[db] + 16 * RB);
            vf[db] = u32x4{t0[0], t0[1], t1[0], t1[1]};
        }
        // every read has returned before the landing set is handed to the next DMA (asm: hipcc does not order it against them otherwise)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    // ---- folding a prefix partial into this wave's state: the shared pieces behind lambdas of this kernel (called straight, the
    // four-wave instantiations lost 2 % at C3, profiles/gqa_unit_frame.md) ----
    auto fold = [&](float lse_p, const f32x4(&x)[NDB]) __attribute__((always_inline)) {
        gqa_fold<D>(lse_p, x, o, m_run, l_run);
    };
    auto fetch = [&](const PartialDev& pd, f32x4(&x)[NDB]) __attribute__((always_inline)) {
        gqa_fetch<T, D>(pd, ridx, g4, x);
    };
    auto fold_pre = [&]() __attribute__((always_inline)) {
        gqa_fold_pre<T, D>(npre, pre_f32, pbuf, plse, o, m_run, l_run);
        pre_folded = true;
    };
    // (a lambda around the three pieces: called straight from the loop, hipcc grows the bf16 kernels by more than 1 %)
    auto compute = [&](int key0) __attribute__((always_inline)) {
        float p[8];
        u32x4 pf;
        const float tmax = gqa_scores<T, D, CT>(key0, g4, seg_len, back, sc, kf, qf, p);
        const float alpha = gqa_softmax_update<T, CT>(tmax, p, m_run, l_run, pf);
        gqa_pv<T, D>(alpha, pf, vf, o);
    };
    {
        constexpr int stride = 32 * WPU;
        const int k_first = wave * 32;
        // The first step goes out as soon as the sequence's length has arrived, and its windows END at the length: a step that reaches
        // past it is zero-filled by the address check instead of being fetched.
        const int len = max(0, min(len_raw, a.kv_len));
        krs[2] = __builtin_amdgcn_readfirstlane((unsigned)len * k_ts);
        vrs[2] = __builtin_amdgcn_readfirstlane((unsigned)len * v_ts);
        seg_len = len;
        const int nst = seg_len > k_first ? (seg_len - k_first + stride - 1) / stride : 0;  // 32-key steps of this wave
        if (nst > 0) issue(k_first, 0u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... all landed
        // hipcc counts only its own loads (q, the first partials, the scales): make it settle them HERE, where nothing is in flight
#pragma unroll
        for (int c = 0; c < NCH; ++c) asm volatile("" ::"v"(qf[c]));
        asm volatile("" : "+v"(ksc), "+v"(vsc));
        if (!pre_folded) fold_pre();  // the pre-requested partials have landed
        // the second set's first step goes out BEHIND the drain: hipcc's own wait for q and the partials is a full one and must not
        // find a key step it does not know about in the queue
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

    // ---- this wave's other partials (all of them when the LSE output is asked for), two per round trip ----
    for (int i = wave + max(npre, 0) * WPU; i < np; i += 2 * WPU) {
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

    // ---- merge the WPU waves of the unit through their widened V tiles ----
    float ms_run = m_s, ls_run = l_s;
    if constexpr (WPU > 1) {
        auto tile_of = [&](int w) { return reinterpret_cast<const float*>(gqa8_smem + w * WB + NSET * SETB); };
        if (!gqa_merge_waves<D, WPU>(wave, l15, g4, reinterpret_cast<float*>(vtile), tile_of, mlx, m_s, l_s, o, m_run, l_run, ms_run, ls_run)) return;
    }
    gqa_epilogue<T, D>(a, rvalid, ridx, g4, o, l_run, ms_run, ls_run);
}

template <typename T, int D, int WPU, int HPW>
static int launch_gqa8_k(const SuffixKvqArgs& ka, dim3 grid, hipStream_t s) {
    constexpr int NWV = WPU * HPW;
    constexpr size_t wave_bytes = (size_t)(D <= 128 ? 2 : 1) * 2 * 32 * D + (size_t)32 * D * 2;  // landing sets + widened V tile
    constexpr size_t lds = NWV * wave_bytes + (WPU > 1 ? (size_t)NWV * 4 * 16 * sizeof(float) : 0);
    static_assert(lds <= 160 * 1024, "LDS of one workgroup");
    // more than the default dynamic-LDS limit: raised to exactly what the launch needs
    return gqa_launch_lds<HYD_GQA_FP8_KERNEL<T, D, WPU, HPW>>(ka, grid, 64 * NWV, lds, lds > 64 * 1024, (int)lds, s);
}

// the 16-bit launcher's shapes-only choices (gqa_launch_plan), for either form: the same 20 instantiations
template <typename T, int D>
static int launch_gqa8_t(const SuffixKvqArgs& ka, hipStream_t s) {
    const SuffixArgs& a = ka.a;
    const int chunks = (a.rows + 15) / 16;
    const GqaLaunchPlan pl = gqa_launch_plan(a, D);  // the 16-bit launcher's choices for these shapes
    dim3 grid((unsigned)a.B * (unsigned)(a.Hkv / pl.hpw), chunks, 1);
    if constexpr (D == 256) {
        if (pl.few_units) return (int)hipErrorInvalidValue;  // (not eligible: suffix_gqa_eligible)
    } else {
        if (pl.few_units) return launch_gqa8_k<T, D, 4, 1>(ka, grid, s);
    }
    switch (pl.hpw) {
        case 4:
            if constexpr (D < 256) return launch_gqa8_k<T, D, 1, 4>(ka, grid, s);
            else return (int)hipErrorInvalidValue;
        case 2: return launch_gqa8_k<T, D, 1, 2>(ka, grid, s);
        default: return launch_gqa8_k<T, D, 1, 1>(ka, grid, s);
    }
}

// ... by q dtype and head dim (the caller has asked its form's eligibility rule)
static int launch_gqa8(const SuffixKvqArgs& ka, int dtype, int D, hipStream_t s) {
    if (dtype == HYD_F16) {
        if (D == 128) return launch_gqa8_t<F16, 128>(ka, s);
        if (D == 64) return launch_gqa8_t<F16, 64>(ka, s);
        if (D == 256) return launch_gqa8_t<F16, 256>(ka, s);
    } else {
        if (D == 128) return launch_gqa8_t<BF16, 128>(ka, s);
        if (D == 64) return launch_gqa8_t<BF16, 64>(ka, s);
        if (D == 256) return launch_gqa8_t<BF16, 256>(ka, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace hyd
