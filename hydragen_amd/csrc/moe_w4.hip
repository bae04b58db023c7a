// Mixture-of-experts MLP on 4-bit (OCP e2m1) expert weights (hyd_moe_mlp_w4; include/hydragen_hip.h states the rules,
// hydragen_amd/moe.py is the definition): packed codes gate_up4 [E, 2 I, H / 2] and down4 [E, H, I / 2] (byte b of a row holds
// k = 2 b in its low and k = 2 b + 1 in its high nibble), a shift 0..12 per group of 32 k, gate_up_shift [E, 2 I, H / 32] and
// down_shift [E, H, I / 32], and one power-of-two fp32 scale per expert and output channel, gate_up_scale [E, 2 I] and down_scale
// [E, H]: weight_quant.quantize_weight_fp4's format on the [E N, K] view.  Routing, grouping and the combine are moe.hip's kernels
// (launch_moe_route_group, launch_moe_combine); the workspace is moe_layout's.  This file holds the two expert products:
//
//   moe_gate_up_w4_kernel   per (expert, 16 intermediate channels): act[slot] = round16(silu(sg * (x Wg4^T)) * (su * (x Wu4^T)))
//   moe_down_w4_kernel      per (expert, 32 output channels):       yslot[slot] = (s * (act[slot] Wd4^T)) * weight[slot]   (fp32)
//
// Both are bound by reading W, now half a byte per weight.  16 bytes hold 32 codes, one whole scale group of a row, so the layout of
// a step is linear_w4.hip's: a step is 256 deep, lane (r, g) loads, per 16-row W tile t and half j = 0 / 1, the 16 bytes of codes at
// k = 256 s + 128 j + 32 g .. + 31 of row r (non-temporal): the four lanes of a row and the two halves cover one whole 128-byte line
// of the row per step, every byte requested once.  Dword h of a load is the A operand of one v_mfma_f32_16x16x32: four
// v_cvt_scalef32_pk_{bf16,f16}_fp4 widen it straight into the packed 16-bit operand with 2^-shift as the instruction's scale (no
// pack, no multiply; e2m1 * 2^-shift lies in [2^-13, 6]: exact and normal in both types), against the 16 bytes of the slot's row at
// k + 8 h -- the lane reads 64 contiguous bytes of x or act over the four h.
//   THE UNIT OF WORK IS A HALF STEP (128 k): the four waves split the ceil(K / 128) halves of the product, not its steps.  Qwen3-30B-
// A3B's down product (K = I = 768) is three steps but six halves: 1, 2, 1, 2 per wave, where whole steps would leave one wave of
// four without work.  A wave walks its halves in k order, so two consecutive halves are still the step's one line; a wave that starts
// on an odd half shares that line with its neighbour (one line of each row per workgroup at most).  Per unit a lane holds one load
// per tile (8 registers) and the next unit's (8 more), half of what a whole-step frame keeps; the loop trip is 8 MT MFMAs.
//   The shift stream is K / 32 bytes per row.  With K % 256 == 0 (the row and the step are 8-byte aligned) a half's four bytes of a row
// are ONE aligned 4-byte load -- the half's half of the step's 8 bytes -- shared by the four lanes of the row; lane (r, g) takes
// byte g.  Other K read the lane's own byte, bounds-checked.  The next unit's bytes travel with the next unit's codes.
//   Tails are whole groups: a 32-deep group at or past K is zeros in both operands and never loaded (H % 64 and I % 32 keep every
// group whole).  The next unit's W loads are issued before this unit's widening and products.  The waves keep their own fp32 tiles:
// no barrier in the k loop; the tiles meet in LDS at the end (park_tiles / add_tiles) and wave 0 adds them in wave order, applies the
// channels' scales to the fp32 sums and stores.  So a call differs from moe.hip on the dequantized weights in accumulation order only.
//   MT tiles of 16 slots per pass, clamped duplicate rows past the expert's count, an immediate return for an expert nobody chose: as
// in moe.hip.  Grids depend on the shapes only and no float is added atomically: capture-safe, and two calls give the same bits.
#include "mma_tiles.h"  // kThreads, kWaves, mfma16, park_tiles, add_tiles

namespace hyd {

namespace {

constexpr int kUnitK = 128;  // k per unit of work: one 16-byte load of codes (one group of 32) per lane and tile

// 8 e2m1 codes (one dword) times the power of two `sc` -> 8 values of T, element j in half j % 2 of dword j / 2 (linear_w4.hip's
// widen_codes; that file keeps its own text so that its objects stay as they are)
template <typename T>
__device__ __forceinline__ u32x4 widen_fp4(uint32_t c, float sc);
template <>
__device__ __forceinline__ u32x4 widen_fp4<BF16>(uint32_t c, float sc) {
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3))};
}
template <>
__device__ __forceinline__ u32x4 widen_fp4<F16>(uint32_t c, float sc) {
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3))};
}

__device__ __forceinline__ float pow2_neg(uint32_t shift) { return __builtin_bit_cast(float, (127u - shift) << 23); }

// the lane's W of unit u: wv[t] = the 32 codes of row t's tile at k = 128 u + 32 g (wrow already points at + 16 g bytes), sv[t] = the
// unit's shift bytes of that row with the lane's own at byte g.  `wide`: K % 256 == 0
__device__ __forceinline__ void load_w(u32x4 (&wv)[2], uint32_t (&sv)[2], const uint8_t* const (&wrow)[2], const uint8_t* const (&srow)[2], int u,
                                       int g, int K, bool wide) {
    const bool in = u * kUnitK + 32 * g < K;  // (the lane's group 4 u + g is one of the row's K / 32)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        wv[t] = u32x4{0u, 0u, 0u, 0u};
        if (in) wv[t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[t] + u * (kUnitK / 2)));
        if (wide)
            sv[t] = *reinterpret_cast<const uint32_t*>(srow[t] + 4 * u);
        else
            sv[t] = in ? (uint32_t)srow[t][4 * u + g] << (8 * g) : 0u;
    }
}

// acc[t][i] += W tile t (code rows wrow[t], shift rows srow[t]) x the rows brow[i] (already at + 32 g), over the units u0 .. u1 - 1 of
// a K-deep product; `tiles` of the MT row tiles are live (uniform over the workgroup).  Operand h of a lane is its k = 32 g + 8 h .. + 7.
template <typename T, int MT>
__device__ __forceinline__ void expert_product_w4(f32x4 (&acc)[2][MT], const uint8_t* const (&wrow)[2], const uint8_t* const (&srow)[2],
                                                  const uint16_t* const (&brow)[MT], int K, int u0, int u1, int g, int tiles) {
    const bool wide = K % 256 == 0;
    u32x4 wv[2];
    uint32_t sv[2];
    if (u0 < u1) load_w(wv, sv, wrow, srow, u0, g, K, wide);
    for (int u = u0; u < u1; ++u) {
        u32x4 wn[2];
        uint32_t sn[2];
        if (u + 1 < u1) load_w(wn, sn, wrow, srow, u + 1, g, K, wide);  // in flight under this unit's widening and products
        const int kc = u * kUnitK;
        u32x4 xv[MT][4];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                xv[i][h] = u32x4{0u, 0u, 0u, 0u};
                if (i < tiles && kc + 32 * g < K) xv[i][h] = *reinterpret_cast<const u32x4*>(brow[i] + kc + 8 * h);
            }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float sc = pow2_neg((sv[t] >> (8 * g)) & 0xffu);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const u32x4 wide_a = widen_fp4<T>(wv[t][h], sc);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    if (i >= tiles) continue;
                    acc[t][i] = mfma16<T>(wide_a, xv[i][h], acc[t][i]);
                }
            }
        }
        if (u + 1 < u1) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                wv[t] = wn[t];
                sv[t] = sn[t];
            }
        }
    }
}

}  // namespace

// grid (I / 16, E).  The two W tiles are code rows i0 .. i0 + 15 (gate) and I + i0 .. (up) of gate_up4[e]; the four waves split H's halves.
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void moe_gate_up_w4_kernel(const MoeW4Args a4) {
    __shared__ float red[(kWaves - 1) * 2 * MT * 256];
    const MoeArgs& a = a4.c.c;
    const int e = (int)blockIdx.y, cnt = a.counts[e];
    if (cnt == 0) return;
    const int first = a.offsets[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int i0 = (int)blockIdx.x * 16;
    const int64_t rg = (int64_t)e * 2 * a.I + i0 + r16, ru = rg + a.I;  // the lane's gate and up rows of the [E 2 I, .] views
    const uint8_t* w = static_cast<const uint8_t*>(a.gate_up);
    const uint8_t* wrow[2] = {w + rg * (a.H >> 1) + 16 * g, w + ru * (a.H >> 1) + 16 * g};
    const uint8_t* srow[2] = {a4.gate_up_shift + rg * (a.H >> 5), a4.gate_up_shift + ru * (a.H >> 5)};
    const int units = (a.H + kUnitK - 1) / kUnitK, u0 = wave * units / kWaves, u1 = (wave + 1) * units / kWaves;
    // the scales of the lane's four channels i0 + 4 g .. + 3, gate and up: requested now, used by wave 0 after the products
    const float* sc = a4.c.gate_up_scale + (int64_t)e * 2 * a.I + i0 + 4 * g;
    float sg[4], su[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sg[r] = sc[r];
        su[r] = sc[a.I + r];
    }
    for (int base = 0; base < cnt; base += 16 * MT) {
        const int tiles = min(MT, (cnt - base + 15) >> 4);
        int slot[MT];
        const uint16_t* brow[MT];
        f32x4 acc[2][MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            slot[i] = a.slots[first + min(base + 16 * i + r16, cnt - 1)];
            brow[i] = static_cast<const uint16_t*>(a.x) + (int64_t)(slot[i] / a.k) * a.xs + 32 * g;
            acc[0][i] = acc[1][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        expert_product_w4<T, MT>(acc, wrow, srow, brow, a.H, u0, u1, g, tiles);
        park_tiles<MT>(red, acc, wave, lane);
        __syncthreads();
        if (wave == 0) {
            add_tiles<MT>(red, acc, lane);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if (i >= tiles || base + 16 * i + r16 >= cnt) continue;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gg = sg[r] * acc[0][i][r];
                    v[r] = gg / (1.f + expf(-gg)) * (su[r] * acc[1][i][r]);
                }
                uint16_t* dst = static_cast<uint16_t*>(a.act) + (int64_t)slot[i] * a.I + i0 + 4 * g;
                *reinterpret_cast<u32x2*>(dst) = u32x2{Traits<T>::pack2(v[0], v[1]), Traits<T>::pack2(v[2], v[3])};
            }
        }
        if (base + 16 * MT < cnt) __syncthreads();  // the next pass parks its tiles where wave 0 has just read
    }
}

// grid (H / 32, E).  The two W tiles are code rows h0 .. h0 + 31 of down4[e]; the four waves split I's halves (a wave whose share is
// empty adds zeros).
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void moe_down_w4_kernel(const MoeW4Args a4) {
    __shared__ float red[(kWaves - 1) * 2 * MT * 256];
    const MoeArgs& a = a4.c.c;
    const int e = (int)blockIdx.y, cnt = a.counts[e];
    if (cnt == 0) return;
    const int first = a.offsets[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int h0 = (int)blockIdx.x * 32;
    const int64_t r0 = (int64_t)e * a.H + h0 + r16, r1 = r0 + 16;  // the lane's rows of the [E H, .] views
    const uint8_t* w = static_cast<const uint8_t*>(a.down);
    const uint8_t* wrow[2] = {w + r0 * (a.I >> 1) + 16 * g, w + r1 * (a.I >> 1) + 16 * g};
    const uint8_t* srow[2] = {a4.down_shift + r0 * (a.I >> 5), a4.down_shift + r1 * (a.I >> 5)};
    const int units = (a.I + kUnitK - 1) / kUnitK, u0 = wave * units / kWaves, u1 = (wave + 1) * units / kWaves;
    const float* sc = a4.c.down_scale + (int64_t)e * a.H + h0 + 4 * g;  // the lane's channels h0 + 16 t + 4 g .. + 3
    float sd[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sd[t][r] = sc[16 * t + r];
    for (int base = 0; base < cnt; base += 16 * MT) {
        const int tiles = min(MT, (cnt - base + 15) >> 4);
        int slot[MT];
        const uint16_t* brow[MT];
        f32x4 acc[2][MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            slot[i] = a.slots[first + min(base + 16 * i + r16, cnt - 1)];
            brow[i] = static_cast<const uint16_t*>(a.act) + (int64_t)slot[i] * a.I + 32 * g;
            acc[0][i] = acc[1][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        expert_product_w4<T, MT>(acc, wrow, srow, brow, a.I, u0, u1, g, tiles);
        park_tiles<MT>(red, acc, wave, lane);
        __syncthreads();
        if (wave == 0) {
            add_tiles<MT>(red, acc, lane);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if (i >= tiles || base + 16 * i + r16 >= cnt) continue;
                const float wgt = a.weights[slot[i]];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = (sd[t][r] * acc[t][i][r]) * wgt;
                    *reinterpret_cast<f32x4*>(a.yslot + (int64_t)slot[i] * a.H + h0 + 16 * t + 4 * g) = v;
                }
            }
        }
        if (base + 16 * MT < cnt) __syncthreads();
    }
}

template <typename T>
static int launch_moe_mlp_w4_t(const MoeW4Args& a4, hipStream_t s) {
    const MoeArgs& a = a4.c.c;
    const dim3 block(kThreads);
    int rc = launch_moe_route_group(a, Traits<T>::kDtype, s);  // (refuses shapes outside the ranges)
    if (rc) return rc;
    const dim3 gu((unsigned)(a.I / 16), (unsigned)a.E), dn((unsigned)(a.H / 32), (unsigned)a.E);
    if (a.T * a.k <= 16) {  // no expert can hold more than one tile of slots
        hipLaunchKernelGGL((moe_gate_up_w4_kernel<T, 1>), gu, block, 0, s, a4);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((moe_down_w4_kernel<T, 1>), dn, block, 0, s, a4);
    } else {
        hipLaunchKernelGGL((moe_gate_up_w4_kernel<T, 2>), gu, block, 0, s, a4);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((moe_down_w4_kernel<T, 2>), dn, block, 0, s, a4);
    }
    if ((rc = (int)hipGetLastError())) return rc;
    return launch_moe_combine(a, Traits<T>::kDtype, s);
}

int launch_moe_mlp_w4(const MoeW4Args& a, int dtype, hipStream_t s) {
    return dtype == HYD_F16 ? launch_moe_mlp_w4_t<F16>(a, s) : launch_moe_mlp_w4_t<BF16>(a, s);
}

}  // namespace hyd
