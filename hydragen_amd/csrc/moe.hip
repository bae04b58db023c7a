// Mixture-of-experts MLP for decode-sized calls (hyd_moe_mlp; include/hydragen_hip.h states the rules, hydragen_amd/moe.py is the
// definition): T <= 128 rows, E <= 256 experts, k <= 8 experts per row, 16-bit weights gate_up [E, 2 I, H] and down [E, H, I].
//
//   moe_route_kernel     one wave per row: the k largest logits (descending, ties to the lower expert) and their softmax weights
//   moe_group_kernel     one workgroup: counts / offsets per expert and the slot numbers t k + j grouped by expert, ascending
//   moe_gate_up_kernel   per (expert, 16 intermediate channels): act[slot] = round16(silu(x Wg^T) * (x Wu^T))
//   moe_down_kernel      per (expert, 32 output channels):       yslot[slot] = weight[slot] * (act[slot] Wd^T)      (fp32)
//   moe_combine_kernel   y[t] = round16(sum_j yslot[t k + j])    in j order, one rounding
//
// Grids depend on the shapes only, nothing is read back by the host, nothing is allocated and no float is added atomically: the
// call can be captured, and two calls give the same bits.  A workgroup of an expert nobody chose returns at once, so the weights
// that are read are those of the chosen experts.
//   The two products are bound by reading W and share linear_w8_kernel's arrangement: W is the A operand of
// v_mfma_f32_16x16x32 (rows = channels), the gathered rows of x / act are the B operand (columns = slots of this expert, 16 per
// tile).  A step is 64 deep: lane (r, g) loads k = 64 s + 16 g .. + 15 of row r of each of the two W tiles as two 16-byte
// non-temporal loads (the four lanes of a row cover a 128-byte line) and each load feeds one MFMA without a shuffle, against the
// same 16 k of the slot's row (the k order inside an MFMA is free as long as both operands agree).  The next step's W loads are
// issued before this step's products.  The four waves split the k range four ways and keep their own fp32 tiles: no barrier in
// the k loop; the tiles meet in LDS at the end and wave 0 adds them in wave order.  With W as A, lane (r, g) ends up with four
// consecutive channels 4 g .. 4 g + 3 of slot r: one 8-byte (act) or 16-byte (yslot) store.
//   MT tiles of 16 slots are carried per pass; an expert with more slots takes further passes over the same W (then in L2).  Rows
// past the expert's count are clamped duplicates of its last slot and are never stored; a 16-deep chunk at or past K is zeros in
// both operands and never loaded.  A column of B only meets its own column of the accumulator: a slot depends on its own row only.
#include "mma_tiles.h"  // kThreads, kWaves, mfma16, park_tiles, add_tiles

namespace hyd {

namespace {

constexpr int kStepK = 64;        // k per step: one 16-byte load of W per lane, tile and half
constexpr int kGroupThreads = 1024;  // one thread per slot: T k <= 128 * 8

// ---- routing -------------------------------------------------------------------------------------------------------------------
// (logit, expert) as one integer whose order is "larger logit first, then lower expert": the float's bits made monotonic (-0 is
// +0, as in a comparison of values) above the complement of the index.  Never 0 for a real candidate: 0 marks "taken / absent".
__device__ __forceinline__ uint64_t route_key(float v, int e) {
    uint32_t u = v == 0.f ? 0u : __builtin_bit_cast(uint32_t, v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - (uint32_t)e);
}
__device__ __forceinline__ float route_value(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

}  // namespace

// grid ceil(T / 4), one wave per row; lane l holds the logits of experts l, l + 64, l + 128, l + 192
template <typename T>
__global__ __launch_bounds__(kThreads) void moe_route_kernel(const MoeArgs a) {
    const int lane = threadIdx.x & 63, t = (int)blockIdx.x * kWaves + ((int)threadIdx.x >> 6);
    if (t >= a.T) return;
    const uint16_t* row = static_cast<const uint16_t*>(a.logits) + (int64_t)t * a.E;
    float v[4];
    uint64_t key[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int e = lane + 64 * c;
        v[c] = 0.f;
        key[c] = 0;
        if (e < a.E) {
            v[c] = Traits<T>::lo((uint32_t)row[e]);
            key[c] = route_key(v[c], e);
        }
    }
    // k rounds of "the best of what is left": k <= E, so every round finds a real candidate and every id is inside [0, E)
    float top = 0.f, mine = 0.f;
    int mine_e = 0;
    for (int j = 0; j < a.k; ++j) {
        uint64_t best = key[0];
#pragma unroll
        for (int c = 1; c < 4; ++c) best = key[c] > best ? key[c] : best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor((unsigned long long)best, off);
            best = o > best ? o : best;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (key[c] == best) key[c] = 0;  // (keys are distinct: the owner alone strikes it out)
        const float val = route_value(best);
        if (j == 0) top = val;
        if (lane == j) {
            mine = val;
            mine_e = (int)(0xffffffffu - (uint32_t)best);
        }
    }
    // expf, not the fast intrinsic: the bound grants the weight 4 2^-23 relative.  The denominator over all E logits is added in
    // float64 (its terms are fp32 exponentials), so that its own roundings do not count; renormalised weights need no denominator
    // over E at all: softmax[id] / sum_j softmax[id_j] = exp(l_j - top) / sum_j exp(l_j - top), the k terms added in j order.
    const float p = lane < a.k ? expf(mine - top) : 0.f;
    float w;
    if (a.renorm) {
        float s = 0.f;
        for (int j = 0; j < a.k; ++j) s += __shfl(p, j);
        w = p / s;
    } else {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (lane + 64 * c < a.E) s += (double)expf(v[c] - top);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        w = (float)((double)p / s);
    }
    if (lane < a.k) {
        const int o = t * a.k + lane;
        a.ids[o] = mine_e;
        a.weights[o] = w;
        if (a.ids_out) a.ids_out[o] = mine_e;
        if (a.weights_out) a.weights_out[o] = w;
    }
}

// One workgroup, one thread per slot.  Integer LDS counters size the groups; a slot's place inside its group is the number of
// earlier slots of the same expert, whatever order the threads arrive in.
__global__ __launch_bounds__(kGroupThreads) void moe_group_kernel(const MoeArgs a) {
    __shared__ int cnt[kMoeMaxExperts], off[kMoeMaxExperts + 4], sid[kGroupThreads];
    const int s = (int)threadIdx.x, n = a.T * a.k;
    if (s < kMoeMaxExperts) cnt[s] = 0;
    __syncthreads();
    const int e = s < n ? a.ids[s] : -1;
    sid[s] = e;
    if (e >= 0) atomicAdd(&cnt[e], 1);
    __syncthreads();
    if (s < 64) {  // exclusive scan over the experts: four per lane, then across the wave
        int c[4], tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) tot += c[i] = cnt[4 * s + i];
        int incl = tot;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (s >= d) incl += o;
        }
        int run = incl - tot;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            off[4 * s + i] = run;
            run += c[i];
        }
        if (s == 63) off[kMoeMaxExperts] = run;  // = n
    }
    __syncthreads();
    if (s < a.E) a.counts[s] = cnt[s];
    if (s <= a.E) a.offsets[s] = off[s];
    if (e < 0) return;
    int rank = 0;
    for (int q = 0; q < s; ++q) rank += sid[q] == e;
    a.slots[off[e] + rank] = s;
}

namespace {

// the lane's W of step s: [t][h] = 8 elements of row t's tile at k = 64 s + 16 g + 8 h (wrow already points at + 16 g)
__device__ __forceinline__ void load_w(u32x4 (&wv)[2][2], const uint16_t* const (&wrow)[2], int s, int g, int K) {
    const int kc = s * kStepK;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            wv[t][h] = u32x4{0u, 0u, 0u, 0u};
            if (kc + 16 * g < K) wv[t][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[t] + kc + 8 * h));
        }
}

// acc[t][i] += W tile t (rows wrow[t]) x the rows brow[i], over the steps s0 .. s1 - 1 of a K-deep product; `tiles` of the MT row
// tiles are live (uniform over the workgroup)
template <typename T, int MT>
__device__ __forceinline__ void expert_product(f32x4 (&acc)[2][MT], const uint16_t* const (&wrow)[2], const uint16_t* const (&brow)[MT],
                                               int K, int s0, int s1, int g, int tiles) {
    u32x4 wv[2][2];
    if (s0 < s1) load_w(wv, wrow, s0, g, K);
    for (int s = s0; s < s1; ++s) {
        u32x4 wn[2][2];
        if (s + 1 < s1) load_w(wn, wrow, s + 1, g, K);  // in flight under this step's products
        const int kc = s * kStepK;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if (i >= tiles) continue;
            u32x4 xv[2];
            xv[0] = xv[1] = u32x4{0u, 0u, 0u, 0u};
            if (kc + 16 * g < K) {
                xv[0] = *reinterpret_cast<const u32x4*>(brow[i] + kc);
                xv[1] = *reinterpret_cast<const u32x4*>(brow[i] + kc + 8);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h) acc[t][i] = mfma16<T>(wv[t][h], xv[h], acc[t][i]);
        }
        if (s + 1 < s1) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h) wv[t][h] = wn[t][h];
        }
    }
}

}  // namespace

// grid (I / 16, E).  The two W tiles are rows i0 .. i0 + 15 (gate) and I + i0 .. (up) of gate_up[e]; the four waves split H.
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void moe_gate_up_kernel(const MoeArgs a) {
    __shared__ float red[(kWaves - 1) * 2 * MT * 256];
    const int e = (int)blockIdx.y, cnt = a.counts[e];
    if (cnt == 0) return;
    const int first = a.offsets[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int i0 = (int)blockIdx.x * 16;
    const uint16_t* w = static_cast<const uint16_t*>(a.gate_up) + (int64_t)e * 2 * a.I * a.H;
    const uint16_t* wrow[2] = {w + (int64_t)(i0 + r16) * a.H + 16 * g, w + (int64_t)(a.I + i0 + r16) * a.H + 16 * g};
    const int steps = a.H / kStepK, s0 = wave * steps / kWaves, s1 = (wave + 1) * steps / kWaves;
    for (int base = 0; base < cnt; base += 16 * MT) {
        const int tiles = min(MT, (cnt - base + 15) >> 4);
        int slot[MT];
        const uint16_t* brow[MT];
        f32x4 acc[2][MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            slot[i] = a.slots[first + min(base + 16 * i + r16, cnt - 1)];
            brow[i] = static_cast<const uint16_t*>(a.x) + (int64_t)(slot[i] / a.k) * a.xs + 16 * g;
            acc[0][i] = acc[1][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        expert_product<T, MT>(acc, wrow, brow, a.H, s0, s1, g, tiles);
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
                    const float gg = acc[0][i][r];
                    v[r] = gg / (1.f + expf(-gg)) * acc[1][i][r];
                }
                uint16_t* dst = static_cast<uint16_t*>(a.act) + (int64_t)slot[i] * a.I + i0 + 4 * g;
                *reinterpret_cast<u32x2*>(dst) = u32x2{Traits<T>::pack2(v[0], v[1]), Traits<T>::pack2(v[2], v[3])};
            }
        }
        if (base + 16 * MT < cnt) __syncthreads();  // the next pass parks its tiles where wave 0 has just read
    }
}

// grid (H / 32, E).  The two W tiles are rows h0 .. h0 + 31 of down[e]; the four waves split I (a wave whose share is empty adds zeros).
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void moe_down_kernel(const MoeArgs a) {
    __shared__ float red[(kWaves - 1) * 2 * MT * 256];
    const int e = (int)blockIdx.y, cnt = a.counts[e];
    if (cnt == 0) return;
    const int first = a.offsets[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int h0 = (int)blockIdx.x * 32;
    const uint16_t* w = static_cast<const uint16_t*>(a.down) + (int64_t)e * a.H * a.I;
    const uint16_t* wrow[2] = {w + (int64_t)(h0 + r16) * a.I + 16 * g, w + (int64_t)(h0 + 16 + r16) * a.I + 16 * g};
    const int steps = (a.I + kStepK - 1) / kStepK, s0 = wave * steps / kWaves, s1 = (wave + 1) * steps / kWaves;
    for (int base = 0; base < cnt; base += 16 * MT) {
        const int tiles = min(MT, (cnt - base + 15) >> 4);
        int slot[MT];
        const uint16_t* brow[MT];
        f32x4 acc[2][MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            slot[i] = a.slots[first + min(base + 16 * i + r16, cnt - 1)];
            brow[i] = static_cast<const uint16_t*>(a.act) + (int64_t)slot[i] * a.I + 16 * g;
            acc[0][i] = acc[1][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        expert_product<T, MT>(acc, wrow, brow, a.I, s0, s1, g, tiles);
        park_tiles<MT>(red, acc, wave, lane);
        __syncthreads();
        if (wave == 0) {
            add_tiles<MT>(red, acc, lane);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if (i >= tiles || base + 16 * i + r16 >= cnt) continue;
                const float wgt = a.weights[slot[i]];
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    *reinterpret_cast<f32x4*>(a.yslot + (int64_t)slot[i] * a.H + h0 + 16 * t + 4 * g) = acc[t][i] * wgt;
            }
        }
        if (base + 16 * MT < cnt) __syncthreads();
    }
}

// one thread per four channels of a row: the k slot rows in j order, one rounding
template <typename T>
__global__ __launch_bounds__(kThreads) void moe_combine_kernel(const MoeArgs a) {
    const int qpr = a.H >> 2;
    const int q = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (q >= a.T * qpr) return;
    const int t = q / qpr, h = (q - t * qpr) * 4;
    const float* p = a.yslot + (int64_t)t * a.k * a.H + h;
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    for (int j = 1; j < a.k; ++j) v += *reinterpret_cast<const f32x4*>(p + (int64_t)j * a.H);
    uint16_t* y = static_cast<uint16_t*>(a.y) + (int64_t)t * a.ys + h;
    *reinterpret_cast<u32x2*>(y) = u32x2{Traits<T>::pack2(v[0], v[1]), Traits<T>::pack2(v[2], v[3])};
}

MoeLayout moe_layout(int T, int E, int k, int H, int I) {
    const auto r16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t n = (size_t)T * (size_t)k;
    MoeLayout l;
    l.ids = 0;
    l.weights = l.ids + r16(4 * n);
    l.counts = l.weights + r16(4 * n);
    l.offsets = l.counts + r16(4 * (size_t)E);
    l.slots = l.offsets + r16(4 * ((size_t)E + 1));
    l.act = l.slots + r16(4 * n);
    l.yslot = l.act + r16(2 * n * (size_t)I);
    l.bytes = l.yslot + r16(4 * n * (size_t)H);
    return l;
}

static bool moe_shapes_ok(const MoeArgs& a) {
    return a.T >= 1 && a.T <= kMoeMaxRows && a.E >= 1 && a.E <= kMoeMaxExperts && a.k >= 1 && a.k <= kMoeMaxTopK && a.k <= a.E && a.H % 64 == 0 &&
           a.I % 32 == 0 && a.H >= 64 && a.I >= 32;
}

// the launches around the two expert products, for every weight format (moe_w8.hip): route and group ...
int launch_moe_route(const MoeArgs& a, int dtype, hipStream_t s) {  // (no limit on T of its own: moe_grouped.hip routes up to 2048 rows)
    const dim3 grid((unsigned)((a.T + kWaves - 1) / kWaves)), block(kThreads);
    if (dtype == HYD_F16)
        hipLaunchKernelGGL(moe_route_kernel<F16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(moe_route_kernel<BF16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_moe_route_group(const MoeArgs& a, int dtype, hipStream_t s) {
    if (!moe_shapes_ok(a)) return (int)hipErrorInvalidValue;
    const int rc = launch_moe_route(a, dtype, s);
    if (rc) return rc;
    hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(kGroupThreads), 0, s, a);
    return (int)hipGetLastError();
}

// ... and combine
int launch_moe_combine(const MoeArgs& a, int dtype, hipStream_t s) {
    const dim3 grid((unsigned)((a.T * (a.H >> 2) + kThreads - 1) / kThreads)), block(kThreads);
    if (dtype == HYD_F16)
        hipLaunchKernelGGL(moe_combine_kernel<F16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(moe_combine_kernel<BF16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

template <typename T>
static int launch_moe_mlp_t(const MoeArgs& a, hipStream_t s) {
    const dim3 block(kThreads);
    int rc = launch_moe_route_group(a, Traits<T>::kDtype, s);
    if (rc) return rc;
    const dim3 gu((unsigned)(a.I / 16), (unsigned)a.E), dn((unsigned)(a.H / 32), (unsigned)a.E);
    if (a.T * a.k <= 16) {  // no expert can hold more than one tile of slots
        hipLaunchKernelGGL((moe_gate_up_kernel<T, 1>), gu, block, 0, s, a);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((moe_down_kernel<T, 1>), dn, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((moe_gate_up_kernel<T, 2>), gu, block, 0, s, a);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((moe_down_kernel<T, 2>), dn, block, 0, s, a);
    }
    if ((rc = (int)hipGetLastError())) return rc;
    return launch_moe_combine(a, Traits<T>::kDtype, s);
}

int launch_moe_mlp(const MoeArgs& a, int dtype, hipStream_t s) {
    if (!moe_shapes_ok(a)) return (int)hipErrorInvalidValue;
    return dtype == HYD_F16 ? launch_moe_mlp_t<F16>(a, s) : launch_moe_mlp_t<BF16>(a, s);
}

}  // namespace hyd
