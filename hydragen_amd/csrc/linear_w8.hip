// Linear layers on fp8 (e4m3fn) weights (hyd_linear_w8, hyd_weight_widen; include/hydragen_hip.h states the rules,
// hydragen_amd/weight_quant.py is the definition): y[m, n] = round16(scale[n] * sum_k x[m, k] * w8[n, k]).
//
// The call is bound by reading W, so both kernels are laid out around that stream.  A wave owns 32 output channels (two 16-row
// MFMA tiles of W) and walks its share of K in steps of 128: per step a lane issues four 16-byte non-temporal loads of W -- lane
// (r, g) reads bytes [64 j + 16 g, + 16) of row n0 + 16 t + r, so the four lanes of a row cover one whole 128-byte line per (t, j
// pair) and every byte of W is requested once per row tile -- and the next step's loads are in flight while this step computes.
// The 16 codes of a load are widened to the activation dtype in registers (v_cvt_pk_f32_fp8 and a pack: every e4m3fn value is a
// bf16 and an f16 value, nothing is rounded) and feed two v_mfma_f32_16x16x32 each with W as the A operand (rows = channels) and x
// as the B operand (columns = rows of x): the k order inside an MFMA is free as long as both operands agree, so lane group g
// simply takes k = 16 g .. 16 g + 15 of the 64-deep half step, which is what its 16-byte load holds.  With W as A the accumulator
// of lane (r, g) holds y[m0 + r][n0 + 16 t + 4 g + 0..3]: four consecutive channels of one row, one 8-byte store.
//   M <= 32, linear_w8_kernel: MT = 1 / 2 16-row tiles of x, read straight from global memory (32 contiguous bytes per lane and
// half step; x is a few rows and lives in L2).  The four waves of a workgroup share the 32 channels and split the workgroup's K
// range four ways; their fp32 tiles meet in LDS at the end, added in wave order.
//   M > 32, linear_w8_rows_kernel: MT = 4 / 8 row tiles (M <= 64 / more; beyond 128 rows the grid adds row tiles, adjacent in launch
// order).  Read per wave, x costs M / 16 times the W bytes in L2 traffic (measured: at M = 64 the kernel above takes 1.2-1.4 x the
// time of this one), so the four waves take four 32-channel groups over the SAME K range and share each step's [16 MT, 128] tile
// of x through LDS, double-buffered, one barrier per step.  (At M = 32 the two forms are level; the one without barriers is kept.)
// Shallow grids are split along K across workgroups (plan_linear_w8, shapes only): the fp32 partial tiles go to the workspace with
// plain 16-byte stores and linear_w8_reduce_kernel adds the slices in slice order, applies the scale and rounds once -- no atomics,
// so a call is bitwise reproducible.  Rows past M and channels past N are computed on clamped (duplicate) rows and never stored; a
// 16-deep chunk at or past K is replaced by zeros in both operands and never loaded.  A column of the B operand only ever meets its
// own column of the accumulator: a row of y depends on its own row of x only.
#include "kv_widen.h"  // widen8: hyd_weight_widen is dequantize_kv's product with the row's scale

namespace hyd {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kNT = 2;         // 16-channel tiles of W per wave
constexpr int kStepK = 128;    // k per step: two 64-deep halves, one 16-byte load of W per lane, tile and half
constexpr int kTargetWgs = 512;  // two workgroups (eight waves) per CU before K stops being split further
constexpr int kRowsTargetWgs = 256;  // linear_w8_rows_kernel: one workgroup per CU; 512 measured slower on four of five shapes (more split slices to write and add)
constexpr int kXRow = 272;  // bytes of an x row of one step in LDS: 128 k x 2 B + 16 B, so that 16 rows' 16-byte reads cover all banks
constexpr int kMinStepsPerWave = 2;
constexpr int kMaxSplits = 16;

template <typename T>
__device__ __forceinline__ uint32_t pack_exact(float lo, float hi);
template <>
__device__ __forceinline__ uint32_t pack_exact<BF16>(float lo, float hi) {  // the values are bf16 values: the upper halves
    return (__builtin_bit_cast(uint32_t, lo) >> 16) | (__builtin_bit_cast(uint32_t, hi) & 0xffff0000u);
}
template <>
__device__ __forceinline__ uint32_t pack_exact<F16>(float lo, float hi) {
    return Traits<F16>::pack2(lo, hi);
}

// 8 e4m3fn codes (the bytes of lo, then of hi) -> 8 values of T, element j in half j % 2 of dword j / 2
template <typename T>
__device__ __forceinline__ u32x4 widen_codes(uint32_t lo, uint32_t hi) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    return u32x4{pack_exact<T>(a[0], a[1]), pack_exact<T>(b[0], b[1]), pack_exact<T>(c[0], c[1]), pack_exact<T>(d[0], d[1])};
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

// the lane's W of step s: [t][j] = 16 codes of row t's tile at k = 128 s + 64 j + 16 g (wrow already points at + 16 g)
__device__ __forceinline__ void load_w(u32x4 (&wv)[kNT][2], const uint8_t* (&wrow)[kNT], int s, int g, int K) {
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kc = s * kStepK + 64 * j;
            wv[t][j] = u32x4{0u, 0u, 0u, 0u};
            if (kc + 16 * g < K) wv[t][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[t] + kc));
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

}  // namespace

// M <= 32 (MT = 1 / 2).  grid (channel group * mtiles + row tile, K split); 4 waves that split the workgroup's K range
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void linear_w8_kernel(const LinearW8Args a) {
    __shared__ float red[(kWaves - 1) * kNT * MT * 4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const unsigned ng = blockIdx.x / (unsigned)a.mtiles, mtile = blockIdx.x - ng * (unsigned)a.mtiles;
    const int m0 = (int)mtile * (16 * MT), n0 = (int)ng * (16 * kNT);
    const int split = (int)blockIdx.y;
    const int parts = a.splits * kWaves, part = split * kWaves + wave;
    const int s0 = (int)((int64_t)part * a.steps / parts), s1 = (int)((int64_t)(part + 1) * a.steps / parts);

    const uint8_t* wrow[kNT];
#pragma unroll
    for (int t = 0; t < kNT; ++t) wrow[t] = a.w8 + (int64_t)min(n0 + 16 * t + r16, a.N - 1) * a.K + 16 * g;
    const uint16_t* xrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) xrow[i] = static_cast<const uint16_t*>(a.x) + (int64_t)min(m0 + 16 * i + r16, a.M - 1) * a.xs + 16 * g;

    f32x4 acc[kNT][MT];
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 wv[kNT][2];
    if (s0 < s1) load_w(wv, wrow, s0, g, a.K);
    for (int s = s0; s < s1; ++s) {
        u32x4 wn[kNT][2];
        if (s + 1 < s1) load_w(wn, wrow, s + 1, g, a.K);  // in flight under this step's products
        u32x4 wide[kNT][2][2];
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                wide[t][j][0] = widen_codes<T>(wv[t][j][0], wv[t][j][1]);
                wide[t][j][1] = widen_codes<T>(wv[t][j][2], wv[t][j][3]);
            }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            u32x4 xv[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int kc = s * kStepK + 64 * j;
                xv[j][0] = xv[j][1] = u32x4{0u, 0u, 0u, 0u};
                if (kc + 16 * g < a.K) {
                    xv[j][0] = *reinterpret_cast<const u32x4*>(xrow[i] + kc);
                    xv[j][1] = *reinterpret_cast<const u32x4*>(xrow[i] + kc + 8);
                }
            }
#pragma unroll
            for (int t = 0; t < kNT; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h) acc[t][i] = mfma16<T>(wide[t][j][h], xv[j][h], acc[t][i]);
        }
        if (s + 1 < s1) {
#pragma unroll
            for (int t = 0; t < kNT; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j) wv[t][j] = wn[t][j];
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
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int m = m0 + 16 * i + r16, n = n0 + 16 * t + 4 * g;
            if (m >= a.M || n >= a.N) continue;
            if (a.splits > 1)  // slice rows are np = N rounded up to 4 floats long: the whole quad is inside
                *reinterpret_cast<f32x4*>(a.ws + ((int64_t)split * a.M + m) * a.np + n) = acc[t][i];
            else
                store_quad<T>(a, m, n, acc[t][i]);
        }
}

// M > 32 (MT = 4 / 8): the workgroup's four waves take four 32-channel groups over the SAME K range and share x through LDS.
// grid (group of 128 channels * mtiles + row tile, K split).  Per step the 256 threads copy the [16 MT, 128] tile of x to LDS with one 16-byte
// load and store per thread and 16 rows (zeros at and past K; rows past M are clamped duplicates), double-buffered: the next
// step's tile and W are loaded to registers before this step's products and written to the other buffer after them, one barrier
// per step.  Fragments are read back with 16-byte LDS loads (row stride kXRow: conflict-free over 16 consecutive lanes).
template <typename T, int MT>
__global__ __launch_bounds__(kThreads) void linear_w8_rows_kernel(const LinearW8Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t xl[2][MT * 16 * kXRow];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const unsigned ng = blockIdx.x / (unsigned)a.mtiles, mtile = blockIdx.x - ng * (unsigned)a.mtiles;
    const int m0 = (int)mtile * (16 * MT), n0 = (int)ng * (16 * kNT * kWaves) + wave * (16 * kNT);
    const int split = (int)blockIdx.y;
    const int s0 = (int)((int64_t)split * a.steps / a.splits), s1 = (int)((int64_t)(split + 1) * a.steps / a.splits);

    const uint8_t* wrow[kNT];
#pragma unroll
    for (int t = 0; t < kNT; ++t) wrow[t] = a.w8 + (int64_t)min(n0 + 16 * t + r16, a.N - 1) * a.K + 16 * g;
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
    if (s0 < s1) {
        load_w(wv, wrow, s0, g, a.K);
#pragma unroll
        for (int p = 0; p < MT; ++p) {
            xg[p] = u32x4{0u, 0u, 0u, 0u};
            if (s0 * kStepK + 8 * xc < a.K) xg[p] = *reinterpret_cast<const u32x4*>(xsrc[p] + s0 * kStepK);
            *reinterpret_cast<u32x4*>(&xl[0][p * 16 * kXRow + xdst]) = xg[p];
        }
    }
    __syncthreads();
    for (int s = s0; s < s1; ++s) {
        const int buf = (s - s0) & 1;
        const bool more = s + 1 < s1;
        u32x4 wn[kNT][2];
        if (more) {
            load_w(wn, wrow, s + 1, g, a.K);
#pragma unroll
            for (int p = 0; p < MT; ++p) {
                xg[p] = u32x4{0u, 0u, 0u, 0u};
                if ((s + 1) * kStepK + 8 * xc < a.K) xg[p] = *reinterpret_cast<const u32x4*>(xsrc[p] + (s + 1) * kStepK);
            }
        }
        u32x4 wide[kNT][2][2];
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                wide[t][j][0] = widen_codes<T>(wv[t][j][0], wv[t][j][1]);
                wide[t][j][1] = widen_codes<T>(wv[t][j][2], wv[t][j][3]);
            }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u32x4 xv = *reinterpret_cast<const u32x4*>(&xl[buf][(16 * i + r16) * kXRow + 128 * j + 32 * g + 16 * h]);
#pragma unroll
                    for (int t = 0; t < kNT; ++t) acc[t][i] = mfma16<T>(wide[t][j][h], xv, acc[t][i]);
                }
        if (more) {
#pragma unroll
            for (int p = 0; p < MT; ++p) *reinterpret_cast<u32x4*>(&xl[buf ^ 1][p * 16 * kXRow + xdst]) = xg[p];
#pragma unroll
            for (int t = 0; t < kNT; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j) wv[t][j] = wn[t][j];
        }
        __syncthreads();
    }
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

// one thread per four channels of a row: the slices in slice order, then the scale and the one rounding
template <typename T>
__global__ __launch_bounds__(kThreads) void linear_w8_reduce_kernel(const LinearW8Args a) {
    const int64_t qpr = a.np >> 2;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= (int64_t)a.M * qpr) return;
    const int64_t m = q / qpr;
    const int n = (int)(q - m * qpr) * 4;
    const int64_t slice = (int64_t)a.M * a.np;
    const float* p = a.ws + m * a.np + n;
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    for (int s = 1; s < a.splits; ++s) v += *reinterpret_cast<const f32x4*>(p + s * slice);
    store_quad<T>(a, (int)m, n, v);
}

// one workgroup per row of W: 8-byte loads, 16-byte stores
template <int MODE>
__global__ __launch_bounds__(kThreads) void weight_widen_kernel(const WeightWidenArgs a) {
    const int n = (int)blockIdx.x;
    const float s = a.scale[n];
    const uint8_t* src = a.w8 + (int64_t)n * a.K;
    uint16_t* dst = static_cast<uint16_t*>(a.out) + (int64_t)n * a.os;
    for (int c = (int)threadIdx.x; c < (a.K >> 3); c += kThreads)
        *reinterpret_cast<u32x4*>(dst + 8 * c) = widen8<MODE>(*reinterpret_cast<const u32x2*>(src + 8 * c), s);
}

LinearW8Plan plan_linear_w8(int M, int N, int K) {
    LinearW8Plan pl;
    pl.mt = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8;  // (16-row tiles of x per workgroup)
    const bool rows = pl.mt > 2;  // linear_w8_rows_kernel: 128 channels per workgroup, the waves share the K range
    const int per_wg = rows ? 16 * kNT * kWaves : 16 * kNT;
    pl.mtiles = (int32_t)(((int64_t)M + 16 * pl.mt - 1) / (16 * pl.mt));
    pl.ngroups = (int32_t)(((int64_t)N + per_wg - 1) / per_wg);
    pl.steps = (int32_t)(((int64_t)K + kStepK - 1) / kStepK);
    const int64_t wgs = (int64_t)pl.ngroups * pl.mtiles, target = rows ? kRowsTargetWgs : kTargetWgs;
    int64_t s = (target + wgs - 1) / wgs;
    const int64_t deep = pl.steps / ((rows ? 1 : kWaves) * kMinStepsPerWave);  // every wave keeps at least kMinStepsPerWave steps
    if (s > deep) s = deep;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s < 1) s = 1;
    pl.splits = (int32_t)s;
    pl.np = ((int64_t)N + 3) / 4 * 4;
    pl.bytes = pl.splits > 1 ? (size_t)pl.splits * (size_t)M * (size_t)pl.np * sizeof(float) : 0;
    return pl;
}

template <typename T>
static int launch_linear_w8_t(const LinearW8Args& a, const LinearW8Plan& pl, hipStream_t s) {
    const dim3 grid((unsigned)((int64_t)pl.ngroups * pl.mtiles), (unsigned)pl.splits), block(kThreads);
    if (pl.mt == 1)
        hipLaunchKernelGGL((linear_w8_kernel<T, 1>), grid, block, 0, s, a);
    else if (pl.mt == 2)
        hipLaunchKernelGGL((linear_w8_kernel<T, 2>), grid, block, 0, s, a);
    else if (pl.mt == 4)
        hipLaunchKernelGGL((linear_w8_rows_kernel<T, 4>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((linear_w8_rows_kernel<T, 8>), grid, block, 0, s, a);
    int rc = (int)hipGetLastError();
    if (rc || pl.splits == 1) return rc;
    const int64_t quads = (int64_t)a.M * (a.np >> 2);
    hipLaunchKernelGGL(linear_w8_reduce_kernel<T>, dim3((unsigned)((quads + kThreads - 1) / kThreads)), block, 0, s, a);
    return (int)hipGetLastError();
}

int launch_linear_w8(const LinearW8Args& a, const LinearW8Plan& pl, int dtype, hipStream_t s) {
    const int64_t wgs = (int64_t)pl.ngroups * pl.mtiles, quads = (int64_t)a.M * (a.np >> 2);
    if (wgs <= 0 || wgs > 0x7fffffffLL || (quads + kThreads - 1) / kThreads > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    return dtype == HYD_F16 ? launch_linear_w8_t<F16>(a, pl, s) : launch_linear_w8_t<BF16>(a, pl, s);
}

int launch_weight_widen(const WeightWidenArgs& a, int dtype, hipStream_t s) {
    if (a.N <= 0) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)a.N), block(kThreads);
    if (dtype == HYD_F16)
        hipLaunchKernelGGL(weight_widen_kernel<kFp8ToF16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(weight_widen_kernel<kFp8ToBf16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
