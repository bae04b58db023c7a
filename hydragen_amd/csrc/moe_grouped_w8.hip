// Mixture-of-experts MLP for large calls on fp8 (e4m3fn) expert weights (hyd_moe_mlp_grouped_w8; include/hydragen_hip.h states the
// rules, hydragen_amd/moe.py is the definition): hyd_moe_mlp_grouped's ranges, sort, tile table and workspace (moe_grouped.hip,
// reached through launch_moe_grouped_sort), on moe_w8.hip's four weight tensors -- codes gate_up8 [E, 2 I, H] and down8 [E, H, I], one
// power-of-two fp32 scale per expert and output channel.  This file holds the two tiled products:
//
//   moe_grouped_gate_up_w8_kernel  per (row tile, 64 intermediate channels): act[sorted position] = round16(silu(sg (x Wg8^T)) * (su (x Wu8^T)))
//   moe_grouped_down_w8_kernel     per (row tile, 128 output channels):      yslot[slot] = (s (act[position] Wd8^T)) * weight[slot]  (fp32)
//
// The frame is the 16-bit file's: four waves 2 x 2 over channels x slots, a W tile of 128 rows as the A operand of v_mfma_f32_16x16x32
// against BM = 64 / 128 gathered rows of x / act as the B operand, 64-deep steps, one barrier per step, clamped duplicate rows and
// channels that are never stored, zeros for a 16-byte chunk at or past K (never loaded), grids from the shapes alone.  The B tile is
// staged as there (rows of eight 16-byte chunks, chunk c of row r at c ^ ((r >> 1) & 7)).  What is this file's own:
//
// W TRAVELS AS CODES INTO LDS.  A thread loads the 16 codes k0 + 16 c .. + 15 of row r (c = tid & 3, r = tid >> 2 and r + 64: two
// 16-byte loads per step where the 16-bit file has four) and stores them to LDS as they are: a step's W tile is 128 rows of 64 bytes,
// 8 KB.  Lane (r16, g) of a wave reads, for MFMA half h and channel tile t, the 8 codes k0 + 32 h + 8 g .. + 7 of row 64 wc + 16 t +
// r16 -- one ds_read_b64 -- and widens them with four v_cvt_scalef32_pk_{bf16,f16}_fp8 (scale 1.0; every e4m3fn value is exact in
// both types) into the packed A operand; element j of the operand is k + j, as in the B operand's 16-byte chunk 4 h + g.  The
// scales multiply the fp32 sums in the epilogues, as in moe_w8.hip: the call differs from the 16-bit grouped call on the dequantized
// weights in the order of fp32 additions only (here: not at all inside a product, the k order is the same).
//
// PLACEMENT OF THE CODE TILE.  Count LDS in 8-byte units: a row of a step is 8 units, u = 4 h + g is the unit a fragment read takes,
// and a 128-byte line of 32 four-byte banks (16 units) holds the two rows 2 q, 2 q + 1.  A fragment read is sixteen rows R .. R + 15
// (R % 16 == 0) at ONE u per group of 16 lanes.  Stored plainly (unit 8 r + u) the sixteen reads fall on two of the sixteen unit
// columns, (8 (r & 1) + u): eight-way conflicts.  Store unit u of row r at
//         8 r + (u ^ x),   x = (r >> 1) & 7
// instead.  Over the sixteen rows, x takes every value 0 .. 7 twice, once with r even and once with r odd, so 8 (r & 1) + (u ^ x)
// takes all sixteen columns once: the 16 lanes of a group cover the 32 banks exactly.  Counted on 64 banks (32 units) the two groups
// g = 2 j, 2 j + 1 that share a pass read u and u ^ 1: the column is 8 (r & 3) + (u ^ x); for fixed r & 3, bit 0 of x is fixed and
// bits 1, 2 run free, so u ^ x and u ^ 1 ^ x together take all eight values: 32 lanes, 32 columns.  The 16-bit file's rule
// c ^ ((r >> 1) & 7) is for rows that fill a line with eight 16-byte chunks; a code row has four, and its reads are half a chunk.
//   The stores keep whole 16-byte writes: the thread's chunk c is the units 2 c, 2 c + 1, which land on (2 c ^ x), (2 c ^ x) ^ 1 -- the
// two halves of the 16-byte place 4 r + (c ^ (x >> 1)), swapped where x is odd.  So a store is one ds_write_b128 of the loaded
// bytes with the halves exchanged by four selects where (r >> 1) & 1.  Sixteen consecutive lanes write the four rows 4 m .. 4 m + 3,
// each row's four places permuted inside the row: 256 contiguous bytes, every bank once.
//
// THE FREED LDS IS A THIRD STAGE.  A stage is 8 KB of codes + 128 BM bytes of rows: 16 / 24 KB where the 16-bit file has 24 / 32.
// 128-deep steps in two stages would be 2 (16 + 32) = 96 KB at row tiles of 128, over the 80 KB that keep two workgroups on a CU, so
// they are not an option for both tile heights.  What the code is short of is time for a global load to land: a wave's step is 16
// (BM = 64) or 32 MFMAs, a few hundred cycles, and the 16-bit file gives a request exactly one step before its wave waits for it in
// front of the barrier.  Three stages of 16 / 24 KB are 48 / 72 KB, and the ring runs two steps ahead: in step s the tiles of step
// s + 3 are requested into one register set, the MFMAs of step s run from stage s % 3, and then the OTHER register set -- step
// s + 2's tiles, requested a step earlier -- is stored to stage (s + 2) % 3, which was last read in step s - 1.  Two steps of global
// loads are in flight under every step's MFMAs, each request has two steps to land, and stage (s + 1) % 3 is already complete when
// step s begins.  (The price is registers, 8 + 4 BM / 32 more than one set; DESIGN.md 4.23 has the figures.  Whether this beats the
// two-stage order has not been measured on its own.)
#include <type_traits>

#include "mma_tiles.h"  // kThreads, kWaves, mfma16

namespace hyd {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kStepK = 64;                  // k per step
constexpr int kWRows = 128;                 // rows of the W tile
constexpr int kWTile = kWRows * kStepK / 16;  // the code tile of a stage in 16-byte units
constexpr int kBChunks = kStepK / 8;        // 16-byte chunks per B row and step
constexpr int kStages = 3;

__device__ __forceinline__ int b_at(int row, int chunk) { return row * kBChunks + (chunk ^ ((row >> 1) & 7)); }  // 16-byte units
__device__ __forceinline__ int w_at8(int row, int u) { return row * 8 + (u ^ ((row >> 1) & 7)); }                // 8-byte units
__device__ __forceinline__ int w_at16(int row, int c) { return row * 4 + (c ^ ((row >> 2) & 3)); }               // 16-byte units: w_at8(row, 2 c) >> 1

// 8 e4m3fn codes -> 8 values of T, element j in half j % 2 of dword j / 2
template <typename T>
__device__ __forceinline__ u32x4 widen8(const u32x2 v) {
    u32x4 r;
    if constexpr (std::is_same<T, BF16>::value) {
        r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[0], 1.0f, false));
        r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[0], 1.0f, true));
        r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[1], 1.0f, false));
        r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v[1], 1.0f, true));
    } else {
        r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[0], 1.0f, false));
        r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[0], 1.0f, true));
        r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[1], 1.0f, false));
        r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v[1], 1.0f, true));
    }
    return r;
}

// the thread's share of the two tiles of the step at k0: 16 codes of the W rows wrow, wrow + 64 (wsrc carries + 16 wchunk) and 8
// values of the B rows brow + 32 i (bsrc carries + 8 bchunk); a chunk at or past K is zeros and is not loaded
template <int NB>
__device__ __forceinline__ void load_stage(u32x4 (&wr)[2], u32x4 (&br)[NB], const uint8_t* const (&wsrc)[2], const uint16_t* const (&bsrc)[NB], int k0,
                                           int wchunk, int bchunk, int K) {
    const bool win = k0 + 16 * wchunk < K, bin = k0 + 8 * bchunk < K;
#pragma unroll
    for (int i = 0; i < 2; ++i) wr[i] = win ? *reinterpret_cast<const u32x4*>(wsrc[i] + k0) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NB; ++i) br[i] = bin ? *reinterpret_cast<const u32x4*>(bsrc[i] + k0) : u32x4{0u, 0u, 0u, 0u};
}

template <int NB>
__device__ __forceinline__ void store_stage(u32x4* stage, const u32x4 (&wr)[2], const u32x4 (&br)[NB], int wrow, int wchunk, int brow, int bchunk) {
    const bool swap = (wrow >> 1) & 1;  // (the same for wrow + 64)
#pragma unroll
    for (int i = 0; i < 2; ++i) stage[w_at16(wrow + 64 * i, wchunk)] = swap ? u32x4{wr[i][2], wr[i][3], wr[i][0], wr[i][1]} : wr[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) stage[kWTile + b_at(brow + 32 * i, bchunk)] = br[i];
}

// one step of the ring: request step s + 3 into (wq, bq), multiply step s from stage `cur`, store (wt, bt) = step s + 2 behind it
template <typename T, int BM>
__device__ __forceinline__ void ring_step(f32x4 (&acc)[4][BM / 32], u32x4* lds, int cur, int s, int steps, u32x4 (&wq)[2], u32x4 (&bq)[BM / 32],
                                          const u32x4 (&wt)[2], const u32x4 (&bt)[BM / 32], const uint8_t* const (&wsrc)[2],
                                          const uint16_t* const (&bsrc)[BM / 32], int K, bool live) {
    constexpr int NB = BM / 32, kStage = kWTile + BM * kBChunks;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4, wc = wave & 1, ws = wave >> 1;
    if (s + 3 < steps) load_stage<NB>(wq, bq, wsrc, bsrc, (s + 3) * kStepK, tid & 3, tid & 7, K);
    if (live) {
        const u32x4* stage = lds + cur * kStage;
        const u32x2* codes = reinterpret_cast<const u32x2*>(stage);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32x2 cv[4];
            u32x4 bv[NB];
#pragma unroll
            for (int t = 0; t < 4; ++t) cv[t] = codes[w_at8(64 * wc + 16 * t + r16, 4 * h + g)];
#pragma unroll
            for (int i = 0; i < NB; ++i) bv[i] = stage[kWTile + b_at(ws * (BM / 2) + 16 * i + r16, 4 * h + g)];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const u32x4 av = widen8<T>(cv[t]);
#pragma unroll
                for (int i = 0; i < NB; ++i) acc[t][i] = mfma16<T>(av, bv[i], acc[t][i]);
            }
        }
    }
    // stage (cur + 2) % 3 was last read in step s - 1, and every wave has passed that step's barrier
    if (s + 2 < steps) store_stage<NB>(lds + (cur == 0 ? 2 : cur - 1) * kStage, wt, bt, tid >> 2, tid & 3, tid >> 3, tid & 7);
    __syncthreads();
}

// acc[t][i] += W code rows 64 wc + 16 t .. + 15 of the tile x B rows ws BM / 2 + 16 i .. + 15 over K, for the wave (wc, ws); `live`:
// the wave has channels to compute (it loads, stores and meets the barriers either way)
template <typename T, int BM>
__device__ __forceinline__ void grouped_product_w8(f32x4 (&acc)[4][BM / 32], u32x4* lds, const uint8_t* const (&wsrc)[2],
                                                   const uint16_t* const (&bsrc)[BM / 32], int K, bool live) {
    constexpr int NB = BM / 32, kStage = kWTile + BM * kBChunks;
    const int tid = (int)threadIdx.x, wrow = tid >> 2, wchunk = tid & 3, brow = tid >> 3, bchunk = tid & 7;
    const int steps = (K + kStepK - 1) / kStepK;
    u32x4 w0[2], b0[NB], w1[2], b1[NB];
    load_stage<NB>(w0, b0, wsrc, bsrc, 0, wchunk, bchunk, K);
    load_stage<NB>(w1, b1, wsrc, bsrc, kStepK, wchunk, bchunk, K);  // (past K: zeros, no loads)
    store_stage<NB>(lds, w0, b0, wrow, wchunk, brow, bchunk);
    if (steps > 1) store_stage<NB>(lds + kStage, w1, b1, wrow, wchunk, brow, bchunk);
    load_stage<NB>(w0, b0, wsrc, bsrc, 2 * kStepK, wchunk, bchunk, K);
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < steps; s += 2) {  // the two register sets change roles from step to step
        ring_step<T, BM>(acc, lds, cur, s, steps, w1, b1, w0, b0, wsrc, bsrc, K, live);
        cur = cur == kStages - 1 ? 0 : cur + 1;
        if (s + 1 < steps) {
            ring_step<T, BM>(acc, lds, cur, s + 1, steps, w0, b0, w1, b1, wsrc, bsrc, K, live);
            cur = cur == kStages - 1 ? 0 : cur + 1;
        }
    }
}

}  // namespace

// grid (row tiles, ceil(I / 64)).  The W tile of channel half h holds the gate code rows i0 + 32 h .. + 31 in LDS rows 64 h .. + 31 and
// the up rows of the same channels in rows 64 h + 32 ..: the wave of that half ends with g and u of one (slot, channel) in one lane.
template <typename T, int BM>
__global__ __launch_bounds__(kThreads) void moe_grouped_gate_up_w8_kernel(const MoeGroupedW8Args aw) {
    constexpr int NB = BM / 32;
    __shared__ u32x4 lds[kStages * (kWTile + BM * kBChunks)];
    const MoeGroupedArgs& a = aw.g;
    const i32x4 tile = reinterpret_cast<const i32x4*>(a.tiles)[blockIdx.x];
    const int e = tile[0], first = tile[1], rows = tile[2];
    if (rows == 0) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4, wc = wave & 1, ws = wave >> 1;
    const int wrow = tid >> 2, brow = tid >> 3, i0 = (int)blockIdx.y * 64, I = a.c.I, H = a.c.H;
    const uint8_t* w = static_cast<const uint8_t*>(a.c.gate_up) + (int64_t)e * 2 * I * H;
    const uint8_t* wsrc[2];
    const uint16_t* bsrc[NB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // LDS row wrow + 64 i: channel half i, gate (wrow < 32) or up row of channel i0 + 32 i + (wrow & 31)
        const int ch = min(i0 + 32 * i + (wrow & 31), I - 1);
        wsrc[i] = w + (int64_t)((wrow >> 5) * I + ch) * H + 16 * (tid & 3);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int slot = a.c.slots[first + min(brow + 32 * i, rows - 1)];
        bsrc[i] = static_cast<const uint16_t*>(a.c.x) + (int64_t)(slot / a.c.k) * a.c.xs + 8 * (tid & 7);
    }
    const bool live = i0 + 32 * wc < I;
    // the scales of the lane's channels i0 + 32 wc + 16 t + 4 g .. + 3, gate and up: requested now, used after the product
    float sg[2][4], su[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* sc = aw.gate_up_scale + (int64_t)e * 2 * I + min(i0 + 32 * wc + 16 * t + 4 * g + r, I - 1);
            sg[t][r] = sc[0];
            su[t][r] = sc[I];
        }
    f32x4 acc[4][NB];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    grouped_product_w8<T, BM>(acc, lds, wsrc, bsrc, H, live);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int row = ws * (BM / 2) + 16 * i + r16;
        if (row >= rows) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t) {  // tiles t: gate, 2 + t: up of channels i0 + 32 wc + 16 t + 4 g .. + 3
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gg = sg[t][r] * acc[t][i][r];
                v[r] = gg / (1.f + expf(-gg)) * (su[t][r] * acc[2 + t][i][r]);
            }
            uint16_t* dst = static_cast<uint16_t*>(a.c.act) + (int64_t)(first + row) * I + i0 + 32 * wc + 16 * t + 4 * g;
            *reinterpret_cast<u32x2*>(dst) = u32x2{Traits<T>::pack2(v[0], v[1]), Traits<T>::pack2(v[2], v[3])};
        }
    }
}

// grid (row tiles, ceil(H / 128)).  The W tile is the code rows h0 .. h0 + 127 of down8[e].
template <typename T, int BM>
__global__ __launch_bounds__(kThreads) void moe_grouped_down_w8_kernel(const MoeGroupedW8Args aw) {
    constexpr int NB = BM / 32;
    __shared__ u32x4 lds[kStages * (kWTile + BM * kBChunks)];
    const MoeGroupedArgs& a = aw.g;
    const i32x4 tile = reinterpret_cast<const i32x4*>(a.tiles)[blockIdx.x];
    const int e = tile[0], first = tile[1], rows = tile[2];
    if (rows == 0) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4, wc = wave & 1, ws = wave >> 1;
    const int wrow = tid >> 2, brow = tid >> 3, h0 = (int)blockIdx.y * kWRows, I = a.c.I, H = a.c.H;
    const uint8_t* w = static_cast<const uint8_t*>(a.c.down) + (int64_t)e * H * I;
    const uint8_t* wsrc[2];
    const uint16_t* bsrc[NB];
#pragma unroll
    for (int i = 0; i < 2; ++i) wsrc[i] = w + (int64_t)min(h0 + wrow + 64 * i, H - 1) * I + 16 * (tid & 3);
#pragma unroll
    for (int i = 0; i < NB; ++i) bsrc[i] = static_cast<const uint16_t*>(a.c.act) + (int64_t)(first + min(brow + 32 * i, rows - 1)) * I + 8 * (tid & 7);
    const bool live = h0 + 64 * wc < H;
    float sd[4][4];  // the scales of the lane's channels h0 + 64 wc + 16 t + 4 g .. + 3
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sd[t][r] = aw.down_scale[(int64_t)e * H + min(h0 + 64 * wc + 16 * t + 4 * g + r, H - 1)];
    f32x4 acc[4][NB];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    grouped_product_w8<T, BM>(acc, lds, wsrc, bsrc, I, live);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int row = ws * (BM / 2) + 16 * i + r16;
        if (row >= rows) continue;
        const int slot = a.c.slots[first + row];  // the scatter back from sorted order
        const float wgt = a.c.weights[slot];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (sd[t][r] * acc[t][i][r]) * wgt;
            *reinterpret_cast<f32x4*>(a.c.yslot + (int64_t)slot * H + h0 + 64 * wc + 16 * t + 4 * g) = v;
        }
    }
}

template <typename T, int BM>
static int launch_products_w8(const MoeGroupedW8Args& aw, hipStream_t s) {
    const MoeGroupedArgs& a = aw.g;
    const dim3 block(kThreads), gu((unsigned)a.ntiles, (unsigned)((a.c.I + 63) / 64)), dn((unsigned)a.ntiles, (unsigned)((a.c.H + kWRows - 1) / kWRows));
    hipLaunchKernelGGL((moe_grouped_gate_up_w8_kernel<T, BM>), gu, block, 0, s, aw);
    if (const int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL((moe_grouped_down_w8_kernel<T, BM>), dn, block, 0, s, aw);
    return (int)hipGetLastError();
}

int launch_moe_mlp_grouped_w8(const MoeGroupedW8Args& args, int dtype, hipStream_t s) {
    MoeGroupedW8Args a = args;
    int rc = launch_moe_grouped_sort(a.g, dtype, s);  // (refuses shapes outside the ranges; sets the tile height and the table's size)
    if (rc) return rc;
    if (dtype == HYD_F16)
        rc = a.g.bm == 128 ? launch_products_w8<F16, 128>(a, s) : launch_products_w8<F16, 64>(a, s);
    else
        rc = a.g.bm == 128 ? launch_products_w8<BF16, 128>(a, s) : launch_products_w8<BF16, 64>(a, s);
    if (rc) return rc;
    return launch_moe_combine(a.g.c, dtype, s);
}

}  // namespace hyd
