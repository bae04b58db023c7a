// Gather each survivor's whole path into one packed shared level (hyd_kv_gather_paths, include/hydragen_hip.h states the rules):
// destination sequence i is, in order, the sequence of its parent rows[i] / div_j in every chain level j -- bytes of packed
// levels of the destination's dtype -- and then the first lens[i] tokens of unique sequence rows[i], written exactly as
// kv_promote.hip writes them (16-bit rows as bytes, e4m3fn rows widened, pad columns of a wider destination row zero).  K and
// V in one launch.  A copy, HBM bound: every lane moves 16 destination bytes per step.  Launch geometry comes from shapes and
// the host's bounds only; rows / lens / cu_dst and every level's offsets are read on the device and checked there, by every
// workgroup of a sequence in the same way: a sequence with one bad entry is skipped as a whole.  A workgroup owns one chunk
// of destination vectors and walks the segments (at most HYD_MAX_LEVELS + 1) that intersect it: the walk is uniform, a lane only
// compares its vector index against the segment's ends.  The destination overlaps no source.  No LDS, no assembly, plain
// vector stores.
#include "kv_widen.h"

namespace hyd {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;  // destination vectors per lane: 16 KiB written per workgroup
constexpr unsigned kChunk = kThreads * kUnroll;

// vectors [lo, hi) of the workgroup's chunk (lo < hi), read from `src` + (vector - base) * 16
__device__ __forceinline__ void copy_bytes(const char* src, char* dst, unsigned base, unsigned lo, unsigned hi, unsigned first) {
    u32x4 val[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const unsigned v = first + u * kThreads;
        const unsigned w = v < lo ? lo : (v < hi ? v : hi - 1);  // (a lane outside [lo, hi) loads a vector of the range and stores nothing)
        val[u] = *reinterpret_cast<const u32x4*>(src + (int64_t)(w - base) * 16);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const unsigned v = first + u * kThreads;
        if (v >= lo && v < hi) *reinterpret_cast<u32x4*>(dst + (int64_t)v * 16) = val[u];
    }
}

}  // namespace

// grid (chunks of kChunk destination vectors of a path of max_path tokens, sequences, K | V)
template <int MODE>
__global__ __launch_bounds__(kThreads) void kv_gather_paths_kernel(const KvGatherArgs a) {
    const KvPromoteArgs& q = a.u;
    const int i = (int)blockIdx.y;
    const int row = q.rows[i], len = q.lens[i], at = q.cu[i];
    // bad device data: the sequence is skipped, nothing is indexed with it (uniform per workgroup)
    if (row < 0 || row >= q.B || len < 0 || len > q.max_len || at < 0) return;
    int64_t path = 0;
#pragma unroll 1
    for (int j = 0; j < a.n_levels; ++j) {
        const int p = (int)fdiv((unsigned)row, a.ldiv[j]);
        if (p >= a.ls[j]) return;
        const int lo = a.lcu[j][p], hi = a.lcu[j][p + 1];
        if (lo < 0 || hi < lo || hi > a.lcap[j]) return;
        path += hi - lo;
    }
    path += len;
    if (path > (int64_t)a.max_path || (int64_t)at + path > (int64_t)q.capacity) return;
    const unsigned vpt = (unsigned)q.vec_per_tok;
    const unsigned total = (unsigned)path * vpt;  // (max_path * vec_per_tok < 2^31: the host checked)
    const unsigned c0 = (unsigned)blockIdx.x * kChunk;
    if (c0 >= total) return;
    const unsigned c1 = c0 + kChunk < total ? c0 + kChunk : total;
    const unsigned first = c0 + threadIdx.x;

    const bool is_v = blockIdx.z != 0;
    char* dst = static_cast<char*>(is_v ? q.v_dst : q.k_dst) + (int64_t)at * vpt * 16;  // packed rows: a token is vpt 16-byte vectors

    // the chain segments, outermost level first (their offsets are read again: scalar loads of lines the check just fetched)
    unsigned s0 = 0;  // first vector of the segment
#pragma unroll 1
    for (int j = 0; j < a.n_levels && s0 < c1; ++j) {
        const int p = (int)fdiv((unsigned)row, a.ldiv[j]);
        const int lo = a.lcu[j][p], hi = a.lcu[j][p + 1];
        const unsigned s1 = s0 + (unsigned)(hi - lo) * vpt;
        if (s1 > c0 && s1 > s0) {  // (not empty, and it reaches into the chunk: s0 < c1 by the loop's condition)
            const char* src = static_cast<const char*>(is_v ? a.lv[j] : a.lk[j]) + (int64_t)lo * vpt * 16;
            copy_bytes(src, dst, s0, s0 > c0 ? s0 : c0, s1 < c1 ? s1 : c1, first);
        }
        s0 = s1;
    }
    if (s0 >= c1) return;

    // the unique segment: kv_promote.hip's body on vectors [max(s0, c0), c1), token and column counted from s0
    const char* src = static_cast<const char*>(is_v ? q.v_src : q.k_src);
    const float* scale = is_v ? q.v_scale : q.k_scale;
    const int64_t bs = is_v ? q.v_bs : q.k_bs, ts = is_v ? q.v_ts : q.k_ts, hs = is_v ? q.v_hs : q.k_hs;
    constexpr int kSrcEsz = MODE == kCopy16 ? 2 : 1;
    src += (int64_t)row * bs * kSrcEsz;
    const unsigned src_vecs = (unsigned)q.d_src >> 3;

    u32x4 val[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const unsigned v = first + u * kThreads;
        val[u] = u32x4{0u, 0u, 0u, 0u};
        if (v >= s0 && v < c1) {
            const unsigned w = v - s0;
            const unsigned t = fdiv(w, q.div_vec_per_tok), r = w - t * vpt;
            const unsigned h = fdiv(r, q.div_vec_per_head), c = r - h * (unsigned)q.vec_per_head;
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
        if (v >= s0 && v < c1) *reinterpret_cast<u32x4*>(dst + (int64_t)v * 16) = val[u];
    }
}

int launch_kv_gather(const KvGatherArgs& a, int src_dtype, int dst_dtype, hipStream_t s) {
    const int64_t vecs = (int64_t)a.max_path * a.u.vec_per_tok;
    const int64_t chunks = (vecs + kChunk - 1) / kChunk;
    if (chunks <= 0 || chunks > 0x7fffffffLL || a.u.n <= 0 || a.u.n > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)chunks, (unsigned)a.u.n, 2), block(kThreads);
    if (src_dtype != HYD_FP8_E4M3)
        hipLaunchKernelGGL(kv_gather_paths_kernel<kCopy16>, grid, block, 0, s, a);
    else if (dst_dtype == HYD_F16)
        hipLaunchKernelGGL(kv_gather_paths_kernel<kFp8ToF16>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(kv_gather_paths_kernel<kFp8ToBf16>, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
