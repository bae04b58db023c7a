// Mixture-of-experts MLP on fp8 (e4m3fn) expert weights (hyd_moe_mlp_w8; include/hydragen_hip.h states the rules,
// hydragen_amd/moe.py is the definition): codes gate_up8 [E, 2 I, H] and down8 [E, H, I] with one power-of-two fp32 scale per
// expert and output channel, gate_up_scale [E, 2 I] and down_scale [E, H].  Routing, grouping and the combine are moe.hip's
// kernels (launch_moe_route_group, launch_moe_combine); the workspace is moe_layout's.  This file holds the two expert products:
//
//   moe_gate_up_w8_kernel   per (expert, 16 intermediate channels): act[slot] = round16(silu(sg * (x Wg8^T)) * (su * (x Wu8^T)))
//   moe_down_w8_kernel      per (expert, 32 output channels):       yslot[slot] = (s * (act[slot] Wd8^T)) * weight[slot]   (fp32)
//
// Both are bound by reading W, now one byte per weight, so a step is 128 deep: lane (r, g) of a wave loads the 32 codes at
// k = 128 s + 32 g .. + 31 of row r of each of the two W tiles as two 16-byte non-temporal loads -- the four lanes of a row
// still cover one whole 128-byte line per step, as they do over 64 k of 16-bit weights -- and widens them in registers
// (v_cvt_pk_f32_fp8 and an exact pack: every e4m3fn value is a bf16 and an f16 value) into four A operands of
// v_mfma_f32_16x16x32, each against the matching 8 k of the 64 contiguous bytes of the slot's row (the k order inside an MFMA is
// free as long as both operands agree).  The next step's W loads are issued before this step's widening and products.  The four
// waves split the steps four ways and keep their own fp32 tiles: no barrier in the k loop; the tiles meet in LDS at the end and
// wave 0 adds them in wave order, applies the channels' scales to the fp32 sums and stores.  The codes are exact 16-bit values and
// the scales powers of two, so a call differs from moe.hip on the dequantized weights in accumulation order only.
//   MT tiles of 16 slots per pass, clamped duplicate rows past the expert's count, zeros for a 16-deep chunk at or past K (never
// loaded; H % 64 and I % 32 keep every chunk whole), an immediate return for an expert nobody chose: as in moe.hip.  Grids depend
// on the shapes only and no float is added atomically: capture-safe, and two calls give the same bits.
#include "mma_tiles.h"  // kThreads, kWaves, mfma16, widen_codes, park_tiles, add_tiles

namespace hyd {

namespace {

constexpr int kStepK = 128;  // k per step: two 16-byte loads of codes per lane and tile

// the lane's W of step s: [t][c] = 16 codes of row t's tile at k = 128 s + 32 g + 16 c (wrow already points at + 32 g)
__device__ __forceinline__ void load_w(u32x4 (&wv)[2][2], const uint8_t* const (&wrow)[2], int s, int g, int K) {
    const int kc = s * kStepK;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            wv[t][c] = u32x4{0u, 0u, 0u, 0u};
            if (kc + 32 * g + 16 * c < K) wv[t][c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[t] + kc + 16 * c));
        }
}

// acc[t][i] += W tile t (code rows wrow[t]) x the rows brow[i] (already at + 32 g), over the steps s0 .. s1 - 1 of a K-deep
// product; `tiles` of the MT row tiles are live (uniform over the workgroup).  Operand q of a lane is its k = 32 g + 8 q .. + 7.
template <typename T, int MT>
__device__ __forceinline__ void expert_product_w8(f32x4 (&acc)[2][MT], const uint8_t* const (&wrow)[2], const uint16_t* const (&brow)[MT],
                                                  int K, int s0, int s1, int g, int tiles) {
    u32x4 wv[2][2];
    if (s0 < s1) load_w(wv, wrow, s0, g, K);
    for (int s = s0; s < s1; ++s) {
        u32x4 wn[2][2];
        if (s + 1 < s1) load_w(wn, wrow, s + 1, g, K);  // in flight under this step's widening and products
        const int kc = s * kStepK;
        u32x4 xv[MT][4];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                xv[i][2 * c] = xv[i][2 * c + 1] = u32x4{0u, 0u, 0u, 0u};
                if (i < tiles && kc + 32 * g + 16 * c < K) {
                    xv[i][2 * c] = *reinterpret_cast<const u32x4*>(brow[i] + kc + 16 * c);
                    xv[i][2 * c + 1] = *reinterpret_cast<const u32x4*>(brow[i] + kc + 16 * c + 8);
                }
            }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            u32x4 wide[4];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                wide[2 * c] = widen_codes<T>(wv[t][c][0], wv[t][c][1]);
                wide[2 * c + 1] = widen_codes<T>(wv[t][c][2], wv[t][c][3]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if (i >= tiles) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[t][i] = mfma16<T>(wide[q], xv[i][q], acc[t][i]);
            }
        }
        if (s + 1 < s1) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int c = 0; c < 2; ++c) wv[t][c] = wn[t][c];
        }
    }
}

}  // namespace

// grid (I / 16, E).  The two W tiles are code rows i0 .. i0 + 15 (gate) and I + i0 .. (up) of gate_up8[e]; the four waves split H.
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void moe_gate_up_w8_kernel(const MoeW8Args aw) {
    __shared__ float red[(kWaves - 1) * 2 * MT * 256];
    const MoeArgs& a = aw.c;
    const int e = (int)blockIdx.y, cnt = a.counts[e];
    if (cnt == 0) return;
    const int first = a.offsets[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int i0 = (int)blockIdx.x * 16;
    const uint8_t* w = static_cast<const uint8_t*>(a.gate_up) + (int64_t)e * 2 * a.I * a.H;
    const uint8_t* wrow[2] = {w + (int64_t)(i0 + r16) * a.H + 32 * g, w + (int64_t)(a.I + i0 + r16) * a.H + 32 * g};
    const int steps = (a.H + kStepK - 1) / kStepK, s0 = wave * steps / kWaves, s1 = (wave + 1) * steps / kWaves;
    // the scales of the lane's four channels i0 + 4 g .. + 3, gate and up: requested now, used by wave 0 after the products
    const float* sc = aw.gate_up_scale + (int64_t)e * 2 * a.I + i0 + 4 * g;
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
        expert_product_w8<T, MT>(acc, wrow, brow, a.H, s0, s1, g, tiles);
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

// grid (H / 32, E).  The two W tiles are code rows h0 .. h0 + 31 of down8[e]; the four waves split I (a wave whose share is empty adds zeros).
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void moe_down_w8_kernel(const MoeW8Args aw) {
    __shared__ float red[(kWaves - 1) * 2 * MT * 256];
    const MoeArgs& a = aw.c;
    const int e = (int)blockIdx.y, cnt = a.counts[e];
    if (cnt == 0) return;
    const int first = a.offsets[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int h0 = (int)blockIdx.x * 32;
    const uint8_t* w = static_cast<const uint8_t*>(a.down) + (int64_t)e * a.H * a.I;
    const uint8_t* wrow[2] = {w + (int64_t)(h0 + r16) * a.I + 32 * g, w + (int64_t)(h0 + 16 + r16) * a.I + 32 * g};
    const int steps = (a.I + kStepK - 1) / kStepK, s0 = wave * steps / kWaves, s1 = (wave + 1) * steps / kWaves;
    const float* sc = aw.down_scale + (int64_t)e * a.H + h0 + 4 * g;  // the lane's channels h0 + 16 t + 4 g .. + 3
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
        expert_product_w8<T, MT>(acc, wrow, brow, a.I, s0, s1, g, tiles);
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
static int launch_moe_mlp_w8_t(const MoeW8Args& aw, hipStream_t s) {
    const MoeArgs& a = aw.c;
    const dim3 block(kThreads);
    int rc = launch_moe_route_group(a, Traits<T>::kDtype, s);  // (refuses shapes outside the ranges)
    if (rc) return rc;
    const dim3 gu((unsigned)(a.I / 16), (unsigned)a.E), dn((unsigned)(a.H / 32), (unsigned)a.E);
    if (a.T * a.k <= 16) {  // no expert can hold more than one tile of slots
        hipLaunchKernelGGL((moe_gate_up_w8_kernel<T, 1>), gu, block, 0, s, aw);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((moe_down_w8_kernel<T, 1>), dn, block, 0, s, aw);
    } else {
        hipLaunchKernelGGL((moe_gate_up_w8_kernel<T, 2>), gu, block, 0, s, aw);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((moe_down_w8_kernel<T, 2>), dn, block, 0, s, aw);
    }
    if ((rc = (int)hipGetLastError())) return rc;
    return launch_moe_combine(a, Traits<T>::kDtype, s);
}

int launch_moe_mlp_w8(const MoeW8Args& a, int dtype, hipStream_t s) {
    return dtype == HYD_F16 ? launch_moe_mlp_w8_t<F16>(a, s) : launch_moe_mlp_w8_t<BF16>(a, s);
}

}  // namespace hyd
