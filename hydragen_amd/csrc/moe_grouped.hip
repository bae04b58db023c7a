// Mixture-of-experts MLP for large calls (hyd_moe_mlp_grouped; include/hydragen_hip.h states the rules, hydragen_amd/moe.py is the
// definition): T <= 2048 rows (T k <= 16384 slots), E, k, H, I and the 16-bit weights as in moe.hip.  Where moe.hip streams W past a
// few slots per expert, this file sorts the slots by expert and runs both products as one tiled GEMM per expert and row tile, both
// operands shared through LDS: every expert is read once per call, not once per 128 rows.
//
//   moe_route_kernel (moe.hip)     one wave per row, as in hyd_moe_mlp
//   moe_grouped_count_kernel       one wave per expert: its number of slots
//   moe_grouped_place_kernel       one wave per expert: its slots in ascending order at its offset (a counting sort: the result does
//                                  not depend on arrival order), and one entry per row tile of BM sorted slots in the tile table
//   moe_grouped_gate_up_kernel     per (row tile, 64 intermediate channels): act[sorted position] = round16(silu(x Wg^T) * (x Wu^T))
//   moe_grouped_down_kernel        per (row tile, 128 output channels):      yslot[slot] = weight[slot] * (act[position] Wd^T)  (fp32)
//   moe_combine_kernel (moe.hip)   y[t] = round16(sum_j yslot[t k + j])
//
// Grids depend on the shapes only (the tile table has room for ceil(T k / BM) + min(E, T k) entries; a workgroup whose entry holds
// no rows returns at once), nothing is read back, nothing is allocated, no float is added atomically.  Row tiles run along the fast
// grid dimension: the workgroups that share a W tile are dispatched together.
//   A product workgroup (four waves, 2 x 2 over channels x slots) multiplies a W tile of 128 rows (the A operand of
// v_mfma_f32_16x16x32: a lane ends with four consecutive channels of one slot) by BM gathered rows of x / act (the B operand) in
// 64-deep steps.  Both tiles of a step live in LDS as rows of eight 16-byte chunks, chunk c of row r at place c ^ ((r >> 1) & 7): the
// sixteen rows a fragment read touches then cover all banks.  Two stages: the next step's global loads are issued into registers
// before this step's MFMAs and stored to the other stage after them; one barrier per step.  In the gate|up kernel the W tile of
// channel half h holds gate rows i0 + 32 h .. + 31 in LDS rows 64 h .. + 31 and the up rows of the same channels in rows 64 h + 32 ..:
// the wave of that half ends with g and u of the same (slot, channel) in the same lane.
//   Rows past a tile's count are clamped duplicates of its last row and are never stored; channels past I / H are clamped duplicates
// whose waves skip their MFMAs and store nothing; a 16-byte chunk at or past K is zeros in both operands and never loaded.
//   launch_moe_grouped_sort makes the route, count and place launches alone: moe_grouped_w8.hip puts its own products behind them.
#include "mma_tiles.h"  // kThreads, kWaves, mfma16

namespace hyd {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kStepK = 64;          // k per step
constexpr int kChunks = kStepK / 8;  // 16-byte chunks per tile row and step
constexpr int kWRows = 128;          // rows of the W tile

__device__ __forceinline__ int lds_at(int row, int chunk) { return row * kChunks + (chunk ^ ((row >> 1) & 7)); }

// the thread's share of a step's two tiles: chunk `chunk` of W rows lrow + 32 i and of B rows lrow + 32 i (the pointers carry + 8 chunk)
template <int NB>
__device__ __forceinline__ void load_stage(u32x4 (&wr)[4], u32x4 (&br)[NB], const uint16_t* const (&wsrc)[4], const uint16_t* const (&bsrc)[NB], int k0,
                                           int chunk, int K) {
    const bool in = k0 + 8 * chunk < K;
#pragma unroll
    for (int i = 0; i < 4; ++i) wr[i] = in ? *reinterpret_cast<const u32x4*>(wsrc[i] + k0) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NB; ++i) br[i] = in ? *reinterpret_cast<const u32x4*>(bsrc[i] + k0) : u32x4{0u, 0u, 0u, 0u};
}

template <int NB>
__device__ __forceinline__ void store_stage(u32x4* stage, const u32x4 (&wr)[4], const u32x4 (&br)[NB], int lrow, int chunk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) stage[lds_at(lrow + 32 * i, chunk)] = wr[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) stage[kWRows * kChunks + lds_at(lrow + 32 * i, chunk)] = br[i];
}

// acc[t][i] += W rows 64 wc + 16 t .. + 15 x B rows ws BM / 2 + 16 i .. + 15 over K, for the wave (wc, ws); `live`: the wave has
// channels to compute (it loads, stores and meets the barriers either way)
template <typename T, int BM>
__device__ __forceinline__ void grouped_product(f32x4 (&acc)[4][BM / 32], u32x4* lds, const uint16_t* const (&wsrc)[4],
                                                const uint16_t* const (&bsrc)[BM / 32], int K, bool live) {
    constexpr int NB = BM / 32, kStage = (kWRows + BM) * kChunks;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4, wc = wave & 1, ws = wave >> 1;
    const int lrow = tid >> 3, chunk = tid & 7;
    u32x4 wr[4], br[NB];
    load_stage<NB>(wr, br, wsrc, bsrc, 0, chunk, K);
    store_stage<NB>(lds, wr, br, lrow, chunk);
    __syncthreads();
    const int steps = (K + kStepK - 1) / kStepK;
    for (int s = 0; s < steps; ++s) {
        const u32x4* cur = lds + (s & 1) * kStage;
        if (s + 1 < steps) load_stage<NB>(wr, br, wsrc, bsrc, (s + 1) * kStepK, chunk, K);  // in flight under this step's products
        if (live) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u32x4 av[4], bv[NB];
#pragma unroll
                for (int t = 0; t < 4; ++t) av[t] = cur[lds_at(64 * wc + 16 * t + r16, 4 * h + g)];
#pragma unroll
                for (int i = 0; i < NB; ++i) bv[i] = cur[kWRows * kChunks + lds_at(ws * (BM / 2) + 16 * i + r16, 4 * h + g)];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int i = 0; i < NB; ++i) acc[t][i] = mfma16<T>(av[t], bv[i], acc[t][i]);
            }
        }
        // the other stage was last read in step s - 1, and every wave has passed that step's barrier
        if (s + 1 < steps) store_stage<NB>(lds + ((s + 1) & 1) * kStage, wr, br, lrow, chunk);
        __syncthreads();
    }
}

}  // namespace

// grid E, one wave per expert: lane l counts the slots l, l + 64, ... (the ids are 64 KB at most and come from L2)
__global__ __launch_bounds__(64) void moe_grouped_count_kernel(const MoeGroupedArgs a) {
    const int e = (int)blockIdx.x, lane = (int)threadIdx.x, n = a.c.T * a.c.k;
    int c = 0;
    for (int s = lane; s < n; s += 64) c += a.c.ids[s] == e;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) a.c.counts[e] = c;
}

// grid E, one wave per expert: offset and first row tile from the counts of the lower experts, the slots by ballot rank in ascending
// order, one table entry (expert, first sorted position, rows, 0) per row tile; the last expert's wave marks the unused entries
__global__ __launch_bounds__(64) void moe_grouped_place_kernel(const MoeGroupedArgs a) {
    const int e = (int)blockIdx.x, lane = (int)threadIdx.x, n = a.c.T * a.c.k, bm = a.bm;
    int off = 0, tile0 = 0;
    for (int q = lane; q < e; q += 64) {
        const int c = a.c.counts[q];
        off += c;
        tile0 += (c + bm - 1) / bm;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        off += __shfl_xor(off, d);
        tile0 += __shfl_xor(tile0, d);
    }
    const int cnt = a.c.counts[e];
    int run = off;
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const bool hit = s < n && a.c.ids[s] == e;
        const uint64_t m = __ballot(hit);
        if (hit) a.c.slots[run + __popcll(m & ((1ull << lane) - 1ull))] = s;  // run + rank < off + cnt <= n
        run += __popcll(m);
    }
    const int tiles = (cnt + bm - 1) / bm;  // tile0 + tiles <= ceil(n / bm) + min(E, n) = a.ntiles
    i32x4* table = reinterpret_cast<i32x4*>(a.tiles);
    for (int t = lane; t < tiles; t += 64) table[tile0 + t] = i32x4{e, off + t * bm, min(bm, cnt - t * bm), 0};
    if (e == a.c.E - 1)
        for (int t = tile0 + tiles + lane; t < a.ntiles; t += 64) table[t] = i32x4{0, 0, 0, 0};
}

// grid (row tiles, ceil(I / 64))
template <typename T, int BM>
__global__ __launch_bounds__(kThreads) void moe_grouped_gate_up_kernel(const MoeGroupedArgs a) {
    constexpr int NB = BM / 32;
    __shared__ u32x4 lds[2 * (kWRows + BM) * kChunks];
    const i32x4 tile = reinterpret_cast<const i32x4*>(a.tiles)[blockIdx.x];
    const int e = tile[0], first = tile[1], rows = tile[2];
    if (rows == 0) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4, wc = wave & 1, ws = wave >> 1;
    const int lrow = tid >> 3, chunk = tid & 7, i0 = (int)blockIdx.y * 64, I = a.c.I, H = a.c.H;
    const uint16_t* w = static_cast<const uint16_t*>(a.c.gate_up) + (int64_t)e * 2 * I * H;
    const uint16_t *wsrc[4], *bsrc[NB];
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // LDS row lrow + 32 i: channel half i >> 1, gate (i & 1 == 0) or up row of channel i0 + 32 (i >> 1) + lrow
        const int ch = min(i0 + 32 * (i >> 1) + lrow, I - 1);
        wsrc[i] = w + (int64_t)((i & 1) * I + ch) * H + 8 * chunk;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int slot = a.c.slots[first + min(lrow + 32 * i, rows - 1)];
        bsrc[i] = static_cast<const uint16_t*>(a.c.x) + (int64_t)(slot / a.c.k) * a.c.xs + 8 * chunk;
    }
    f32x4 acc[4][NB];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool live = i0 + 32 * wc < I;
    grouped_product<T, BM>(acc, lds, wsrc, bsrc, H, live);
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
                const float gg = acc[t][i][r];
                v[r] = gg / (1.f + expf(-gg)) * acc[2 + t][i][r];
            }
            uint16_t* dst = static_cast<uint16_t*>(a.c.act) + (int64_t)(first + row) * I + i0 + 32 * wc + 16 * t + 4 * g;
            *reinterpret_cast<u32x2*>(dst) = u32x2{Traits<T>::pack2(v[0], v[1]), Traits<T>::pack2(v[2], v[3])};
        }
    }
}

// grid (row tiles, ceil(H / 128))
template <typename T, int BM>
__global__ __launch_bounds__(kThreads) void moe_grouped_down_kernel(const MoeGroupedArgs a) {
    constexpr int NB = BM / 32;
    __shared__ u32x4 lds[2 * (kWRows + BM) * kChunks];
    const i32x4 tile = reinterpret_cast<const i32x4*>(a.tiles)[blockIdx.x];
    const int e = tile[0], first = tile[1], rows = tile[2];
    if (rows == 0) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4, wc = wave & 1, ws = wave >> 1;
    const int lrow = tid >> 3, chunk = tid & 7, h0 = (int)blockIdx.y * kWRows, I = a.c.I, H = a.c.H;
    const uint16_t* w = static_cast<const uint16_t*>(a.c.down) + (int64_t)e * H * I;
    const uint16_t *wsrc[4], *bsrc[NB];
#pragma unroll
    for (int i = 0; i < 4; ++i) wsrc[i] = w + (int64_t)min(h0 + lrow + 32 * i, H - 1) * I + 8 * chunk;
#pragma unroll
    for (int i = 0; i < NB; ++i) bsrc[i] = static_cast<const uint16_t*>(a.c.act) + (int64_t)(first + min(lrow + 32 * i, rows - 1)) * I + 8 * chunk;
    f32x4 acc[4][NB];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool live = h0 + 64 * wc < H;
    grouped_product<T, BM>(acc, lds, wsrc, bsrc, I, live);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int row = ws * (BM / 2) + 16 * i + r16;
        if (row >= rows) continue;
        const int slot = a.c.slots[first + row];  // the scatter back from sorted order
        const float wgt = a.c.weights[slot];
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(a.c.yslot + (int64_t)slot * H + h0 + 64 * wc + 16 * t + 4 * g) = acc[t][i] * wgt;
    }
}

static bool grouped_shapes_ok(int T, int E, int k, int H, int I) {
    return T >= 1 && T <= kMoeGroupedMaxRows && E >= 1 && E <= kMoeMaxExperts && k >= 1 && k <= kMoeMaxTopK && k <= E && H % 64 == 0 && I % 32 == 0 &&
           H >= 64 && I >= 32;
}

// rows per row tile, from the shapes alone: 128 where an expert holds 128 slots and more on average
static int grouped_bm(int T, int E, int k) { return T * k >= 128 * E ? 128 : 64; }

MoeGroupedLayout moe_grouped_layout(int T, int E, int k, int H, int I) {
    const auto r16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t n = (size_t)T * (size_t)k;
    MoeGroupedLayout l;
    l.ids = 0;
    l.weights = l.ids + r16(4 * n);
    l.counts = l.weights + r16(4 * n);
    l.slots = l.counts + r16(4 * (size_t)E);
    l.tiles = l.slots + r16(4 * n);
    l.act = l.tiles + 16 * ((n + 63) / 64 + (n < (size_t)E ? n : (size_t)E));  // room for either tile height
    l.yslot = l.act + r16(2 * n * (size_t)I);
    l.bytes = l.yslot + r16(4 * n * (size_t)H);
    return l;
}

template <typename T, int BM>
static int launch_products(const MoeGroupedArgs& a, hipStream_t s) {
    const dim3 block(kThreads), gu((unsigned)a.ntiles, (unsigned)((a.c.I + 63) / 64)), dn((unsigned)a.ntiles, (unsigned)((a.c.H + kWRows - 1) / kWRows));
    hipLaunchKernelGGL((moe_grouped_gate_up_kernel<T, BM>), gu, block, 0, s, a);
    if (const int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL((moe_grouped_down_kernel<T, BM>), dn, block, 0, s, a);
    return (int)hipGetLastError();
}

// route, count and place: the launches in front of the products, shared with moe_grouped_w8.hip; sets the tile height and the table's size
int launch_moe_grouped_sort(MoeGroupedArgs& a, int dtype, hipStream_t s) {
    if (!grouped_shapes_ok(a.c.T, a.c.E, a.c.k, a.c.H, a.c.I)) return (int)hipErrorInvalidValue;
    const int n = a.c.T * a.c.k;
    a.bm = grouped_bm(a.c.T, a.c.E, a.c.k);
    a.ntiles = (n + a.bm - 1) / a.bm + (n < a.c.E ? n : a.c.E);
    int rc = launch_moe_route(a.c, dtype, s);
    if (rc) return rc;
    hipLaunchKernelGGL(moe_grouped_count_kernel, dim3((unsigned)a.c.E), dim3(64), 0, s, a);
    if ((rc = (int)hipGetLastError())) return rc;
    hipLaunchKernelGGL(moe_grouped_place_kernel, dim3((unsigned)a.c.E), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int launch_moe_mlp_grouped(const MoeGroupedArgs& args, int dtype, hipStream_t s) {
    MoeGroupedArgs a = args;
    int rc = launch_moe_grouped_sort(a, dtype, s);
    if (rc) return rc;
    if (dtype == HYD_F16)
        rc = a.bm == 128 ? launch_products<F16, 128>(a, s) : launch_products<F16, 64>(a, s);
    else
        rc = a.bm == 128 ? launch_products<BF16, 128>(a, s) : launch_products<BF16, 64>(a, s);
    if (rc) return rc;
    return launch_moe_combine(a.c, dtype, s);
}

}  // namespace hyd
