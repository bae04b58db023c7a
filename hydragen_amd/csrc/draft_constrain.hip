// Speculative decoding under a token automaton (include/hydragen_hip.h; hydragen_amd/speculative.py and
// constraint.py state both rules in torch / numpy).
//
//   * dfa_forced_kernel (hyd_dfa_forced_tokens), once per automaton: forced[s] = the one token state s allows, or -1.  The next
//     table can be gigabytes, so only the bitmap is read: one wave per state walks the row's words -- 16 bytes per lane and
//     load where every row is 16-byte aligned --, sums popcounts and keeps the position of a set bit; a wave reduction (shuffles,
//     no LDS) gives the count and the largest position, which is THE position when the count is 1.  Bits at positions >= n are
//     masked off; words past ceil(n / 32) (the stride's padding) are never read.
//   * draft_constrain_kernel (hyd_draft_constrain), every step, between the drafts and the forward pass: row b walks its K
//     drafts through the automaton from state[b].  A forced state REPLACES the draft by the forced token (accepted with
//     probability 1: the masked sampler can draw nothing else); a draft the automaton rejects ends the row's proposal.  The
//     walk is a dependent chain of at most 7 table reads, so it is one row per lane; step_state[b, i] is the state from which
//     the draw behind fed[b, i] is taken (the constrained sampler's per-logits-row state).  No address is ever formed from a
//     state outside [0, n_states) or a token outside [0, n).
#include "hyd_kernels.h"

namespace hyd {

namespace {

__device__ __forceinline__ void take(uint32_t w, int word, int& count, int& pos) {
    if (w) {
        count += __popc(w);
        pos = word * 32 + (31 - __clz((int)w));  // (words ascend per lane: the lane's last set bit)
    }
}

}  // namespace

template <bool VEC>
__global__ __launch_bounds__(256) void dfa_forced_kernel(const hyd_dfa_forced_params a) {
    const int lane = (int)threadIdx.x & 63;
    const int s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (s >= a.n_states) return;  // (whole waves leave: the shuffles below run on full waves)
    const uint32_t* row = a.allowed + (int64_t)s * a.allowed_stride;
    const int words = (a.n + 31) / 32;
    const int full = a.n / 32;  // words whose 32 bits all lie below n
    int count = 0, pos = -1;
    int w0 = 0;
    if (VEC) {
        const int quads = full / 4;
        const uint4* row4 = reinterpret_cast<const uint4*>(row);
        for (int q = lane; q < quads; q += 64) {
            const uint4 v = row4[q];
            take(v.x, 4 * q, count, pos);
            take(v.y, 4 * q + 1, count, pos);
            take(v.z, 4 * q + 2, count, pos);
            take(v.w, 4 * q + 3, count, pos);
        }
        w0 = quads * 4;
    }
    for (int w = w0 + lane; w < words; w += 64) {
        uint32_t v = row[w];
        if (w >= full) v &= (1u << (a.n & 31)) - 1u;  // the partial last word: bits at positions >= n are ignored
        take(v, w, count, pos);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        count += __shfl_xor(count, d);
        const int o = __shfl_xor(pos, d);
        pos = o > pos ? o : pos;
    }
    if (lane == 0) a.forced[s] = count == 1 ? pos : -1;
}

int launch_dfa_forced(const hyd_dfa_forced_params& p, hipStream_t s) {
    const int grid = (p.n_states + 3) / 4;
    if (grid == 0) return 0;
    const bool vec = ((uintptr_t)p.allowed & 15) == 0 && (p.allowed_stride & 3) == 0;
    if (vec) hipLaunchKernelGGL(dfa_forced_kernel<true>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(dfa_forced_kernel<false>, dim3(grid), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(64) void draft_constrain_kernel(const hyd_draft_constrain_params a) {
    const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (b >= a.B) return;
    const int K = a.K;
    int64_t* fed = a.fed + (int64_t)b * a.fed_stride;
    int32_t* ss = a.step_state + (int64_t)b * (K + 1);
    int s = a.state[b];
    int np = a.n_proposed ? a.n_proposed[b] : 0;
    int nf = 0;
    bool ended = false;  // the chain has ended: the draws behind the remaining drafts are never kept
    ss[0] = s;
    for (int j = 0; j < K; ++j) {
        if (!ended) {
            const bool in = s >= 0 && s < a.n_states;
            int64_t t = in ? (int64_t)a.forced[s] : -1;
            if (t >= 0) {
                fed[j + 1] = t;
                ++nf;
                np = np > j + 1 ? np : j + 1;
            } else if (a.only_forced) {
                ended = true;
            } else {
                t = fed[j + 1];
            }
            if (!ended && in) {
                const int e = (t >= 0 && t < a.n) ? a.next[(int64_t)s * a.next_stride + t] : HYD_DFA_REJECT;
                if (e == HYD_DFA_REJECT) ended = true;  // the masked sampler can never draw this draft
                else s = e == HYD_DFA_FREE ? -2 : (e >= 0 && e < a.n_states) ? e : -1;
            }
            if (ended) np = np < j ? np : j;
        }
        ss[j + 1] = ended ? -1 : s;
    }
    if (a.n_proposed) a.n_proposed[b] = np;
    a.n_forced[b] = nf;
}

int launch_draft_constrain(const hyd_draft_constrain_params& p, hipStream_t s) {
    const int grid = (p.B + 63) / 64;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(draft_constrain_kernel, dim3(grid), dim3(64), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace hyd
