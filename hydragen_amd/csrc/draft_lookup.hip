// Draft proposal by prompt lookup (hyd_draft_lookup; include/hydragen_hip.h states the rule, hydragen_amd/speculative.py the same in
// torch): the completions of the workloads this library is for copy from their prompts, so the tokens that followed the latest
// earlier occurrence of a row's last n-gram are good drafts -- no draft model.  One wave per row.  The row's logical sequence is
// never materialised: it is a table of segments (shared levels at row b / div, the row's own prompt, its generated tokens), and a
// token is fetched by walking the table, so shared tokens are read where they are -- no [B, context] copy.  Lane l tests the
// candidate end positions L - 2 - l, L - 2 - l - 64, ...: the match length at end position e is the number of j < ngram_max with
// token e - j == token L - 1 - j (stopping at the sequence start), and a candidate counts from ngram_min on.  The winner is the
// maximum of (match length, position) -- the longest n-gram first, the latest occurrence among equals --, a wave reduction of one
// 64-bit key.  A few thousand cached 8-byte loads per row: the launch is latency, not work, and it synchronises with nothing.
#include "hyd_kernels.h"

namespace hyd {

__global__ __launch_bounds__(64) void draft_lookup_kernel(const hyd_draft_lookup_params a) {
    const int b = (int)blockIdx.x;
    const int lane = (int)threadIdx.x;
    // the row's segment table: row pointer and first logical position of every segment (wave-uniform)
    const int64_t* base[HYD_DRAFT_MAX_SEGMENTS];
    int start[HYD_DRAFT_MAX_SEGMENTS + 1];
    int L = 0;
#pragma unroll
    for (int s = 0; s < HYD_DRAFT_MAX_SEGMENTS; ++s) {
        start[s] = L;
        base[s] = nullptr;
        if (s < a.n_segments) {
            const hyd_draft_segment& g = a.segments[s];
            const int r = b / g.div;
            int64_t n = g.lens_i64 ? g.lens_i64[r] : g.lens_i32 ? (int64_t)g.lens_i32[r] : (int64_t)g.len;
            n = n < 0 ? 0 : (n > g.len ? (int64_t)g.len : n);  // never past the row's `len` columns
            base[s] = g.ids + (int64_t)r * g.row_stride;
            L += (int)n;
        }
    }
    start[HYD_DRAFT_MAX_SEGMENTS] = L;
    auto token = [&](int p) __attribute__((always_inline)) -> int64_t {  // 0 <= p < L
        int64_t t = 0;
#pragma unroll
        for (int s = 0; s < HYD_DRAFT_MAX_SEGMENTS; ++s)
            if (p >= start[s] && p < start[s + 1]) t = base[s][p - start[s]];
        return t;
    };
    int64_t tail[HYD_DRAFT_MAX_NGRAM];  // tail[j] = token L - 1 - j
#pragma unroll
    for (int j = 0; j < HYD_DRAFT_MAX_NGRAM; ++j) tail[j] = (j < a.ngram_max && L - 1 - j >= 0) ? token(L - 1 - j) : -1;

    long long best = -1;  // (match length << 32) | end position
    for (int e = L - 2 - lane; e >= 0; e -= 64) {
        int m = 0;
#pragma unroll
        for (int j = 0; j < HYD_DRAFT_MAX_NGRAM; ++j) {
            if (j < a.ngram_max && m == j && e - j >= 0 && token(e - j) == tail[j]) m = j + 1;
        }
        if (m >= a.ngram_min) {
            const long long key = ((long long)m << 32) | (long long)e;
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    const int e = best < 0 ? L : (int)(best & 0xffffffffll);
    int n = best < 0 ? 0 : L - 1 - e;
    n = n > a.K ? a.K : n;
    if (lane < a.K) a.drafts[(int64_t)b * a.drafts_stride + lane] = lane < n ? token(e + 1 + lane) : 0;
    if (lane == 0) a.n_proposed[b] = n;
}

int launch_draft_lookup(const hyd_draft_lookup_params& p, hipStream_t s) {
    if (p.B == 0) return 0;
    hipLaunchKernelGGL(draft_lookup_kernel, dim3(p.B), dim3(64), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace hyd
