// Acceptance of a verified multi-token decode step (hyd_draft_accept; include/hydragen_hip.h states the rules, hydragen_amd/
// speculative.py the same in torch).  Row b was fed its last emitted token and K drafts, and the sampler drew one token from the
// logits behind each of them: sampled[b, i] is a draw from the target distribution given fed[b, 0 .. i], so it is a valid next token
// exactly when the drafts in front of it were the tokens actually emitted -- the row keeps sampled[b, 0 .. n], n = the number of
// leading drafts that equal the draw before them.  One thread per row, as in stop_update.hip, which this kernel replaces on the
// speculative path: it also cuts at the first EOS id and at max_new_tokens, writes the output matrix at the row's own length (rows
// advance by different amounts), and produces the next step's first token and position -- a finished row gets the position that
// retires it from the unique K/V stream.  The host never looks at a token; it polls *live.
#include "hyd_kernels.h"

namespace hyd {

// STATES (hyd_draft_accept_states): a row that emits e >= 1 tokens also takes the automaton state behind its last emitted token,
// state[b] = after[b, e - 1] -- the constrained sampler has advanced the step's states in place, one per logits row.
template <bool STATES>
__global__ __launch_bounds__(64) void draft_accept_kernel(const hyd_draft_accept_params a, const int32_t* after, int32_t* state) {
    const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
    bool running = false;
    if (b < a.rows) {
        const int T = a.T;
        int len = a.length[b];
        int r = a.reason[b];
        int emitted = 0;
        int64_t last = a.pad;
        if (r == 0 && len < a.max_new_tokens) {
            const int64_t* fed = a.fed + (int64_t)b * T;
            const int64_t* smp = a.sampled + (int64_t)b * T;
            int n = 0;
            while (n < T - 1 && fed[n + 1] == smp[n]) ++n;
            int e = n + 1;
            const int room = a.max_new_tokens - len;
            e = e < room ? e : room;
            int which = -1;
            for (int i = 0; i < e && which < 0; ++i) {
                for (int k = 0; k < a.n_eos; ++k) {
                    if (smp[i] == a.eos[k]) {
                        which = k;
                        e = i + 1;  // the EOS token is kept
                        break;
                    }
                }
            }
            int64_t* row = a.out + (int64_t)b * a.out_stride + len;
            for (int i = 0; i < e; ++i) row[i] = smp[i];
            if (a.logprobs && a.out_logprobs) {
                const float* lp = a.logprobs + (int64_t)b * T;
                float* lrow = a.out_logprobs + (int64_t)b * a.out_stride + len;
                for (int i = 0; i < e; ++i) lrow[i] = lp[i];
            }
            last = smp[e - 1];
            len += e;
            emitted = e;
            a.length[b] = len;
            if (STATES) state[b] = after[(int64_t)b * T + e - 1];
            if (which >= 0) {
                r = 1;
                a.reason[b] = 1;
                a.stop_index[b] = which;
            }
        }
        running = r == 0 && len < a.max_new_tokens;
        a.accepted[b] = emitted > 0 ? emitted - 1 : 0;
        a.feed[b] = running ? last : a.pad;
        a.next_pos[b] = (running || !a.retire) ? a.start_pos[b] + len - 1 : (a.shared_len ? a.shared_len[b] : 0) - 1;
    }
    // rows still running after this step: one vector atomic per wave that has any
    const unsigned long long m = __ballot(running);
    if (threadIdx.x == 0 && m != 0) atomicAdd(a.live, (int)__popcll(m));
}

int launch_draft_accept(const hyd_draft_accept_params& p, hipStream_t s) {
    const int grid = (p.rows + 63) / 64;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(draft_accept_kernel<false>, dim3(grid), dim3(64), 0, s, p, (const int32_t*)nullptr, (int32_t*)nullptr);
    return (int)hipGetLastError();
}

int launch_draft_accept_states(const hyd_draft_accept_params& p, const int32_t* step_state_after, int32_t* state, hipStream_t s) {
    const int grid = (p.rows + 63) / 64;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(draft_accept_kernel<true>, dim3(grid), dim3(64), 0, s, p, step_state_after, state);
    return (int)hipGetLastError();
}

}  // namespace hyd
