// Promote unique K/V rows to a packed shared level (hyd_kv_promote, include/hydragen_hip.h states the rules): the first lens[i]
// tokens of unique sequence rows[i] become packed tokens [cu[i], cu[i] + lens[i]) of the destination, K and V in one launch.
// A copy, HBM bound: every lane moves 16 destination bytes per step -- a 16-byte load and store for 16-bit sources (bytes as they
// are, whatever they encode), an 8-byte load widened to eight 16-bit values for e4m3fn sources (kv_quant.dequantize_kv: float(q8)
// * scale[h] as an fp32 product, rounded once to the destination dtype, ties to even) -- and the pad columns of a wider
// destination row are stored as zeros.  Launch geometry comes from shapes and the host's length bound only; rows / lens / cu are
// read on the device and checked there: a sequence whose entries would index outside the source or the destination is skipped
// as a whole.  No LDS, no assembly, plain vector stores.
#include "kv_widen.h"  // fdiv, cvt1 / widen8: shared with kv_gather.hip

namespace hyd {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;  // destination vectors per lane: 16 KiB written per workgroup

}  // namespace

// grid (chunks of kThreads * kUnroll destination vectors, sequences, K | V)
template <int MODE>
__global__ __launch_bounds__(kThreads) void kv_promote_kernel(const KvPromoteArgs a) {
    const int i = (int)blockIdx.y;
    const int row = a.rows[i], len = a.lens[i], at = a.cu[i];
    // bad device data: the sequence is skipped, nothing is indexed with it (uniform per workgroup)
    if (row < 0 || row >= a.B || len <= 0 || len > a.max_len || at < 0 || (int64_t)at + len > (int64_t)a.capacity) return;
    const unsigned total = (unsigned)len * (unsigned)a.vec_per_tok;  // (max_len * vec_per_tok < 2^31: the host checked)
    const unsigned first = (unsigned)blockIdx.x * (kThreads * kUnroll) + threadIdx.x;
    if ((unsigned)blockIdx.x * (kThreads * kUnroll) >= total) return;

    const bool is_v = blockIdx.z != 0;
    const char* src = static_cast<const char*>(is_v ? a.v_src : a.k_src);
    char* dst = static_cast<char*>(is_v ? a.v_dst : a.k_dst);
    const float* scale = is_v ? a.v_scale : a.k_scale;
    const int64_t bs = is_v ? a.v_bs : a.k_bs, ts = is_v ? a.v_ts : a.k_ts, hs = is_v ? a.v_hs : a.k_hs;
    constexpr int kSrcEsz = MODE == kCopy16 ? 2 : 1;
    src += (int64_t)row * bs * kSrcEsz;
    dst += (int64_t)at * a.vec_per_tok * 16;  // packed rows: a token is vec_per_tok 16-byte vectors
    const unsigned src_vecs = (unsigned)a.d_src >> 3;

    u32x4 val[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const unsigned v = first + u * kThreads;
        val[u] = u32x4{0u, 0u, 0u, 0u};
        if (v < total) {
            const unsigned t = fdiv(v, a.div_vec_per_tok), r = v - t * (unsigned)a.vec_per_tok;
            const unsigned h = fdiv(r, a.div_vec_per_head), c = r - h * (unsigned)a.vec_per_head;
            if (c < src_vecs) {  // else: a pad column of a wider destination row
                const char* p = src + ((int64_t)t * ts + (int64_t)h * hs + c * 8) * kSrcEsz;
                if (MODE == kCopy16) {
                    val[u] = *reinterpret_cast<const u32x4*>(p);
                } else {
                    val[u] = widen8<MODE>(*reinterpret_cast<const u32x2*>(p), scale ? scale[h] : 1.f);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const unsigned v = first + u * kThreads;
        if (v < total) *reinterpret_cast<u32x4*>(dst + (int64_t)v * 16) = val[u];
    }
}

int launch_kv_promote(const KvPromoteArgs& a, int src_dtype, int dst_dtype, hipStream_t s) {
    const int64_t vecs = (int64_t)a.max_len * a.vec_per_tok;
    const int64_t chunks = (vecs + kThreads * kUnroll - 1) / (kThreads * kUnroll);
    if (chunks <= 0 || chunks > 0x7fffffffLL || a.n <= 0 || a.n > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)chunks, (unsigned)a.n, 2), block(kThreads);
    if (src_dtype != HYD_FP8_E4M3)
        hipLaunchKernelGGL(kv_promote_kernel<kCopy16>, grid, block, 0, s, a);
    else if (dst_dtype == HYD_F16)
        hipLaunchKernelGGL(kv_promote_kernel<kFp8ToF16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(kv_promote_kernel<kFp8ToBf16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
