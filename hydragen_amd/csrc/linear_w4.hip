// Linear layers on 4-bit (OCP e2m1) weights with two-level power-of-two scales (hyd_linear_w4, hyd_weight_widen_w4;
// include/hydragen_hip.h states the rules, hydragen_amd/weight_quant.py is the definition):
//     y[m, n] = round16(scale[n] * sum_k x[m, k] * e2m1(w4[n, k]) * 2^-shift[n, k / 32]).
//
// The call is bound by reading W, as on fp8 weights (linear_w8.hip), and keeps that kernel's frame: a wave owns 32 output channels
// (two 16-row MFMA tiles of W, W is the A operand), W arrives in 16-byte non-temporal loads with the next step's loads in flight
// under this step's products, the accumulator of lane (r, g) holds y[m0 + r][n0 + 16 t + 4 g + 0..3], split-K slices go to the fp32
// workspace in linear_w8.hip's layout and ITS reduce kernel finishes the call (the per-channel scale and the one rounding are the
// fp8 call's).  The layout inside a step is this kernel's own, because 16 bytes now hold 32 codes -- one whole scale group of a row:
//   - a step is 256 deep.  Lane (r, g) issues, per 16-row tile t and j = 0 / 1, one load of bytes [128 s + 64 j + 16 g, + 16) of row
//     n0 + 16 t + r: the codes of k = 256 s + 128 j + 32 g .. + 31, so the four lanes of a row and the two j cover one whole 128-byte
//     line of the row per step, every byte requested once;
//   - the load feeds FOUR v_mfma_f32_16x16x32: MFMA h takes dword h of the load, the lane's codes 8 h .. 8 h + 7.  Four
//     v_cvt_scalef32_pk_{bf16,f16}_fp4 (byte select 0..3) widen the dword straight into the packed 16-bit A operand with 2^-shift as
//     the instruction's scale: no pack, no multiply.  e2m1 * 2^-shift lies in [2^-13, 6]: exact and normal in bf16 and in f16;
//   - the k order inside an MFMA is free as long as both operands agree: the lane's B fragment for MFMA h is the 16 bytes of x at
//     k + 8 h, the 64 contiguous bytes of its group over the four h;
//   - the shift stream is K / 32 bytes per row.  With K % 256 == 0 a step's 8 bytes of a row are ONE aligned 8-byte load that the
//     four lanes of the row share (no request beyond the W loads' own lines in flight); lane (r, g) takes byte 4 j + g of it.  Other
//     K read the lane's own two bytes, bounds-checked.  The next step's bytes travel with the next step's codes;
//   - tails are whole groups: a 32-deep group at or past K is zeros in both operands and never loaded (K % 32 == 0 is required).
//   M <= 32, linear_w4_kernel: MT = 1 / 2 row tiles of x read straight from global memory / L2; the four waves of a workgroup share
// the 32 channels and split the workgroup's K range; their fp32 tiles meet in LDS and are added in wave order.
//   M > 32, linear_w4_rows_kernel: MT = 4 / 8; the four waves take four channel groups over the SAME K range and share x through
// LDS.  The x tile is [16 MT, 128]: a W step is walked as two 128-deep sub-steps (j = 0 / 1: exactly the codes of wv[t][j]), the
// tile double-buffered with one barrier per sub-step, so that LDS stays at the fp8 kernel's 68 KB (two workgroups per CU at MT = 4;
// a [128, 256] tile twice over would be 135 KB).
// Rows past M and channels past N are computed on clamped (duplicate) rows and never stored; offsets are 64-bit; no atomics.
#include "hyd_kernels.h"

namespace hyd {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kNT = 2;         // 16-channel tiles of W per wave
constexpr int kStepK = 256;    // k per step: two 128-deep halves, one 16-byte load of W (32 codes) per lane, tile and half
constexpr int kTargetWgs = 512;
constexpr int kRowsTargetWgs = 256;
constexpr int kXRow = 272;     // bytes of an x row of one sub-step in LDS: 128 k x 2 B + 16 B (16 rows' 16-byte reads cover all banks)
constexpr int kMinStepsPerWave = 2;
constexpr int kMaxSplits = 16;

// 8 e2m1 codes (one dword: byte b holds k = 2 b in its low and k = 2 b + 1 in its high nibble) times the power of two `sc`
// -> 8 values of T, element j in half j % 2 of dword j / 2
template <typename T>
__device__ __forceinline__ u32x4 widen_codes(uint32_t c, float sc);
template <>
__device__ __forceinline__ u32x4 widen_codes<BF16>(uint32_t c, float sc) {
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3))};
}
template <>
__device__ __forceinline__ u32x4 widen_codes<F16>(uint32_t c, float sc) {
    return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3))};
}

template <typename T>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 mfma16<BF16>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma16<F16>(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ float pow2_neg(uint32_t shift) { return __builtin_bit_cast(float, (127u - shift) << 23); }

// 2^-shift of the lane's group of load (t, j): byte 4 j + g of the step's 8 shift bytes
__device__ __forceinline__ float group_scale(const u32x2& sv, int j, int g) { return pow2_neg((sv[j] >> (8 * g)) & 0xffu); }

// the lane's W of step s: wv[t][j] = the 32 codes of row t's tile at k = 256 s + 128 j + 32 g (wrow already points at + 16 g bytes),
// sv[t] = the step's shift bytes of that row with the lane's own at byte 4 j + g
__device__ __forceinline__ void load_w(u32x4 (&wv)[kNT][2], u32x2 (&sv)[kNT], const uint8_t* (&wrow)[kNT], const uint8_t* (&srow)[kNT], int s,
                                       int g, const LinearW4Args& a) {
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wv[t][j] = u32x4{0u, 0u, 0u, 0u};
            if (s * kStepK + 128 * j + 32 * g < a.c.K) wv[t][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[t] + s * (kStepK / 2) + 64 * j));
        }
        if (a.wide_shift) {
            sv[t] = *reinterpret_cast<const u32x2*>(srow[t] + 8 * s);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int gi = 8 * s + 4 * j + g;
                sv[t][j] = gi < a.groups ? (uint32_t)srow[t][gi] << (8 * g) : 0u;
            }
        }
    }
}

// y[m][n .. n + 3] = round(v * scale[n .. n + 3]): one 8-byte store, or single elements at the N tail
template <typename T>
__device__ __forceinline__ void store_quad(const LinearW8Args& a, int m, int n, f32x4 v) {
    float s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = n + r < a.N ? a.scale[n + r] : 0.f;
    const uint32_t p0 = Traits<T>::pack2(v[0] * s[0], v[1] * s[1]), p1 = Traits<T>::pack2(v[2] * s[2], v[3] * s[3]);
    uint16_t* y = static_cast<uint16_t*>(a.y) + (int64_t)m * a.ys + n;
    if (n + 3 < a.N) {
        *reinterpret_cast<u32x2*>(y) = u32x2{p0, p1};
    } else {
        y[0] = (uint16_t)(p0 & 0xffffu);
        if (n + 1 < a.N) y[1] = (uint16_t)(p0 >> 16);
        if (n + 2 < a.N) y[2] = (uint16_t)(p1 & 0xffffu);
    }
}

// the workgroup's tiles leave: fp32 quads to the split's slice (rows np = N rounded up to 4 floats long: the whole quad is inside),
// or scaled and rounded to y
template <typename T, int MT>
__device__ __forceinline__ void store_tiles(const LinearW8Args& a, const f32x4 (&acc)[kNT][MT], int m0, int n0, int r16, int g, int split) {
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int m = m0 + 16 * i + r16, n = n0 + 16 * t + 4 * g;
            if (m >= a.M || n >= a.N) continue;
            if (a.splits > 1)
                *reinterpret_cast<f32x4*>(a.ws + ((int64_t)split * a.M + m) * a.np + n) = acc[t][i];
            else
                store_quad<T>(a, m, n, acc[t][i]);
        }
}

}  // namespace

// M <= 32 (MT = 1 / 2).  grid (channel group * mtiles + row tile, K split); 4 waves that split the workgroup's K range
template <typename T, int MT>
__global__ __launch_bounds__(kThreads, MT == 2 ? 4 : 5) void linear_w4_kernel(const LinearW4Args a4) {
    __shared__ float red[(kWaves - 1) * kNT * MT * 4 * 64];
    const LinearW8Args& a = a4.c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const unsigned ng = blockIdx.x / (unsigned)a.mtiles, mtile = blockIdx.x - ng * (unsigned)a.mtiles;
    const int m0 = (int)mtile * (16 * MT), n0 = (int)ng * (16 * kNT);
    const int split = (int)blockIdx.y;
    const int parts = a.splits * kWaves, part = split * kWaves + wave;
    const int s0 = (int)((int64_t)part * a.steps / parts), s1 = (int)((int64_t)(part + 1) * a.steps / parts);

    const uint8_t *wrow[kNT], *srow[kNT];
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
        const int64_t n = min(n0 + 16 * t + r16, a.N - 1);
        wrow[t] = a.w8 + n * (a.K >> 1) + 16 * g;
        srow[t] = a4.shift + n * a4.groups;
    }
    const uint16_t* xrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) xrow[i] = static_cast<const uint16_t*>(a.x) + (int64_t)min(m0 + 16 * i + r16, a.M - 1) * a.xs + 32 * g;

    f32x4 acc[kNT][MT];
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 wv[kNT][2];
    u32x2 sv[kNT];
    if (s0 < s1) load_w(wv, sv, wrow, srow, s0, g, a4);
    for (int s = s0; s < s1; ++s) {
        u32x4 wn[kNT][2];
        u32x2 sn[kNT];
        if (s + 1 < s1) load_w(wn, sn, wrow, srow, s + 1, g, a4);  // in flight under this step's products
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kc = s * kStepK + 128 * j;
            u32x4 xv[MT][4];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    xv[i][h] = u32x4{0u, 0u, 0u, 0u};
                    if (kc + 32 * g < a.K) xv[i][h] = *reinterpret_cast<const u32x4*>(xrow[i] + kc + 8 * h);
                }
#pragma unroll
            for (int t = 0; t < kNT; ++t) {
                const float sc = group_scale(sv[t], j, g);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const u32x4 wide = widen_codes<T>(wv[t][j][h], sc);
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[t][i] = mfma16<T>(wide, xv[i][h], acc[t][i]);
                }
            }
        }
        if (s + 1 < s1) {
#pragma unroll
            for (int t = 0; t < kNT; ++t) {
                sv[t] = sn[t];
#pragma unroll
                for (int j = 0; j < 2; ++j) wv[t][j] = wn[t][j];
            }
        }
    }

    // the four waves' tiles meet in LDS: wave 0 adds them in wave order (a fixed order: reproducible) and stores
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(((wave - 1) * kNT + t) * MT + i) * 256 + r * 64 + lane] = acc[t][i][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < kWaves - 1; ++w)
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][i][r] += red[((w * kNT + t) * MT + i) * 256 + r * 64 + lane];
    store_tiles<T, MT>(a, acc, m0, n0, r16, g, split);
}

// M > 32 (MT = 4 / 8): the workgroup's four waves take four 32-channel groups over the SAME K range and share x through LDS.
// grid (group of 128 channels * mtiles + row tile, K split).  Per 128-deep sub-step the 256 threads copy the [16 MT, 128] tile of x to
// LDS with one 16-byte load and store per thread and 16 rows (zeros at and past K; rows past M are clamped duplicates).  Sub-step j
// of a step computes from buffer j while the next sub-step's tile -- (s, 1) under j = 0, (s + 1, 0) under j = 1 -- is loaded to
// registers before the products and written to the other buffer after them: one barrier per sub-step.  Fragments are read back with
// 16-byte LDS loads: lane (r, g), MFMA h reads bytes [64 g + 16 h, + 16) of row 16 i + r.
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void linear_w4_rows_kernel(const LinearW4Args a4) {
    __shared__ __attribute__((aligned(16))) uint8_t xl[2][MT * 16 * kXRow];
    const LinearW8Args& a = a4.c;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const unsigned ng = blockIdx.x / (unsigned)a.mtiles, mtile = blockIdx.x - ng * (unsigned)a.mtiles;
    const int m0 = (int)mtile * (16 * MT), n0 = (int)ng * (16 * kNT * kWaves) + wave * (16 * kNT);
    const int split = (int)blockIdx.y;
    const int s0 = (int)((int64_t)split * a.steps / a.splits), s1 = (int)((int64_t)(split + 1) * a.steps / a.splits);

    const uint8_t *wrow[kNT], *srow[kNT];
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
        const int64_t n = min(n0 + 16 * t + r16, a.N - 1);
        wrow[t] = a.w8 + n * (a.K >> 1) + 16 * g;
        srow[t] = a4.shift + n * a4.groups;
    }
    const int xr = tid >> 4, xc = tid & 15;  // the thread's row of a 16-row pass and its 8-element column chunk
    const uint16_t* xsrc[MT];
#pragma unroll
    for (int p = 0; p < MT; ++p) xsrc[p] = static_cast<const uint16_t*>(a.x) + (int64_t)min(m0 + 16 * p + xr, a.M - 1) * a.xs + 8 * xc;
    const int xdst = xr * kXRow + 16 * xc;

    f32x4 acc[kNT][MT];
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 wv[kNT][2], xg[MT];
    u32x2 sv[kNT];
    if (s0 < s1) {
        load_w(wv, sv, wrow, srow, s0, g, a4);
#pragma unroll
        for (int p = 0; p < MT; ++p) {
            xg[p] = u32x4{0u, 0u, 0u, 0u};
            if (s0 * kStepK + 8 * xc < a.K) xg[p] = *reinterpret_cast<const u32x4*>(xsrc[p] + s0 * kStepK);
            *reinterpret_cast<u32x4*>(&xl[0][p * 16 * kXRow + xdst]) = xg[p];
        }
    }
    __syncthreads();
    for (int s = s0; s < s1; ++s) {
        const bool more = s + 1 < s1;
        u32x4 wn[kNT][2];
        u32x2 sn[kNT];
        if (more) load_w(wn, sn, wrow, srow, s + 1, g, a4);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool next = j == 0 || more;
            const int kn = j == 0 ? s * kStepK + 128 : (s + 1) * kStepK;  // the next sub-step's first k
            if (next) {
#pragma unroll
                for (int p = 0; p < MT; ++p) {
                    xg[p] = u32x4{0u, 0u, 0u, 0u};
                    if (kn + 8 * xc < a.K) xg[p] = *reinterpret_cast<const u32x4*>(xsrc[p] + kn);
                }
            }
            const float sc[kNT] = {group_scale(sv[0], j, g), group_scale(sv[1], j, g)};
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const u32x4 wide[kNT] = {widen_codes<T>(wv[0][j][h], sc[0]), widen_codes<T>(wv[1][j][h], sc[1])};
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const u32x4 xv = *reinterpret_cast<const u32x4*>(&xl[j][(16 * i + r16) * kXRow + 64 * g + 16 * h]);
#pragma unroll
                    for (int t = 0; t < kNT; ++t) acc[t][i] = mfma16<T>(wide[t], xv, acc[t][i]);
                }
            }
            if (next) {
#pragma unroll
                for (int p = 0; p < MT; ++p) *reinterpret_cast<u32x4*>(&xl[j ^ 1][p * 16 * kXRow + xdst]) = xg[p];
            }
            __syncthreads();
        }
        if (more) {
#pragma unroll
            for (int t = 0; t < kNT; ++t) {
                sv[t] = sn[t];
#pragma unroll
                for (int j = 0; j < 2; ++j) wv[t][j] = wn[t][j];
            }
        }
    }
    store_tiles<T, MT>(a, acc, m0, n0, r16, g, split);
}

// One value of T from the fp32 product x: round to nearest, ties to even -- bf16 by the integer rule (x is never NaN: codes and
// scales are finite), f16 by the hardware conversion.  What torch's cast of the fp32 product gives.
template <typename T>
__device__ __forceinline__ uint32_t cvt16(float x);
template <>
__device__ __forceinline__ uint32_t cvt16<BF16>(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
template <>
__device__ __forceinline__ uint32_t cvt16<F16>(float x) {
    // (the sign is taken from the fp32 product itself: hipcc may fold product and conversion into one mixed-precision fma whose zero
    // addend turns the -0 of code 8 into +0)
    return __builtin_bit_cast(uint16_t, (_Float16)x) | ((__builtin_bit_cast(uint32_t, x) >> 16) & 0x8000u);
}

// one workgroup per row of W; a thread takes whole groups: one 16-byte load (32 codes), one shift byte, four 16-byte stores
template <typename T>
__global__ __launch_bounds__(kThreads) void weight_widen_fp4_kernel(const WeightWidenW4Args a) {
    const int n = (int)blockIdx.x;
    const float s = a.scale[n];
    const int groups = a.K >> 5;
    const uint8_t* src = a.w4 + (int64_t)n * (a.K >> 1);
    const uint8_t* sh = a.shift + (int64_t)n * groups;
    uint16_t* dst = static_cast<uint16_t*>(a.out) + (int64_t)n * a.os;
    for (int c = (int)threadIdx.x; c < groups; c += kThreads) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(src + 16 * c);
        const float sc = pow2_neg(sh[c]);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const f32x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[d], sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[d], sc, 1);
            const f32x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[d], sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[d], sc, 3);
            *reinterpret_cast<u32x4*>(dst + 32 * c + 8 * d) =
                u32x4{cvt16<T>(p0[0] * s) | (cvt16<T>(p0[1] * s) << 16), cvt16<T>(p1[0] * s) | (cvt16<T>(p1[1] * s) << 16),
                      cvt16<T>(p2[0] * s) | (cvt16<T>(p2[1] * s) << 16), cvt16<T>(p3[0] * s) | (cvt16<T>(p3[1] * s) << 16)};
        }
    }
}

// linear_w8.hip's plan with 256-deep steps: the rows kernel from 33 rows on, K split while the grid is shallow and every wave
// keeps kMinStepsPerWave steps
LinearW8Plan plan_linear_w4(int M, int N, int K) {
    LinearW8Plan pl;
    pl.mt = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8;
    const bool rows = pl.mt > 2;
    const int per_wg = rows ? 16 * kNT * kWaves : 16 * kNT;
    pl.mtiles = (int32_t)(((int64_t)M + 16 * pl.mt - 1) / (16 * pl.mt));
    pl.ngroups = (int32_t)(((int64_t)N + per_wg - 1) / per_wg);
    pl.steps = (int32_t)(((int64_t)K + kStepK - 1) / kStepK);
    const int64_t wgs = (int64_t)pl.ngroups * pl.mtiles, target = rows ? kRowsTargetWgs : kTargetWgs;
    int64_t s = (target + wgs - 1) / wgs;
    const int64_t deep = pl.steps / ((rows ? 1 : kWaves) * kMinStepsPerWave);
    if (s > deep) s = deep;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s < 1) s = 1;
    pl.splits = (int32_t)s;
    pl.np = ((int64_t)N + 3) / 4 * 4;
    pl.bytes = pl.splits > 1 ? (size_t)pl.splits * (size_t)M * (size_t)pl.np * sizeof(float) : 0;
    return pl;
}

template <typename T>
static int launch_linear_w4_t(const LinearW4Args& a, const LinearW8Plan& pl, hipStream_t s) {
    const dim3 grid((unsigned)((int64_t)pl.ngroups * pl.mtiles), (unsigned)pl.splits), block(kThreads);
    if (pl.mt == 1)
        hipLaunchKernelGGL((linear_w4_kernel<T, 1>), grid, block, 0, s, a);
    else if (pl.mt == 2)
        hipLaunchKernelGGL((linear_w4_kernel<T, 2>), grid, block, 0, s, a);
    else if (pl.mt == 4)
        hipLaunchKernelGGL((linear_w4_rows_kernel<T, 4>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((linear_w4_rows_kernel<T, 8>), grid, block, 0, s, a);
    const int rc = (int)hipGetLastError();
    if (rc || pl.splits == 1) return rc;
    return launch_linear_w8_reduce(a.c, Traits<T>::kDtype, s);  // the slices in slice order, the scale, the one rounding
}

int launch_linear_w4(const LinearW4Args& a, const LinearW8Plan& pl, int dtype, hipStream_t s) {
    const int64_t wgs = (int64_t)pl.ngroups * pl.mtiles, quads = (int64_t)a.c.M * (a.c.np >> 2);
    if (wgs <= 0 || wgs > 0x7fffffffLL || (quads + kThreads - 1) / kThreads > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    return dtype == HYD_F16 ? launch_linear_w4_t<F16>(a, pl, s) : launch_linear_w4_t<BF16>(a, pl, s);
}

int launch_weight_widen_w4(const WeightWidenW4Args& a, int dtype, hipStream_t s) {
    if (a.N <= 0) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)a.N), block(kThreads);
    if (dtype == HYD_F16)
        hipLaunchKernelGGL(weight_widen_fp4_kernel<F16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(weight_widen_fp4_kernel<BF16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
