// hyd_draft_accept_stop: draft_accept.hip's acceptance with stop_update.hip's rules applied to EVERY token a row emits in the
// step (include/hydragen_hip.h states the rules, hydragen_amd/speculative.py accept_stop_reference the same in torch).  A
// speculative step emits up to 8 tokens per row at once; a stop sequence may complete at any of them and may have begun in an
// earlier step, so the row's tokens are judged one by one, in order, each against the row's own output so far: the result is
// what e successive one-token hyd_stop_update steps over the accepted draws give.  A draw behind the cut never reaches `out`
// and is never matched.  The kernel also keeps the penalties' per-sequence token lists (gen / gen_len): on the speculative
// route the accept owns them, because only it knows which draws became output.
// One thread per row as in draft_accept.hip; the stop / gen parts are branches that are uniform per launch.
#include "hyd_kernels.h"

namespace hyd {

template <bool STATES>
__global__ __launch_bounds__(64) void draft_accept_stop_kernel(const hyd_draft_accept_params a, const DraftStopArgs s, const int32_t* after,
                                                               int32_t* state) {
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
            int64_t* row = a.out + (int64_t)b * a.out_stride;
            const bool lps = a.logprobs && a.out_logprobs;
            int which = -1, trim = 0;
            for (int i = 0; i < e; ++i) {  // (e shrinks to i + 1 at the token that ends the row)
                const int c = len + i;
                const int64_t tk = smp[i];
                row[c] = tk;
                if (lps) a.out_logprobs[(int64_t)b * a.out_stride + c] = a.logprobs[(int64_t)b * T + i];
                for (int k = 0; k < a.n_eos; ++k) {  // the EOS token is kept
                    if (tk == a.eos[k]) {
                        r = 1;
                        which = k;
                        break;
                    }
                }
                for (int k = 0; r == 0 && k < s.n_stop; ++k) {  // list order: the lowest matching k wins
                    const int sl = s.stop_lens[k];
                    const int64_t* st = s.stop_tokens + (int64_t)k * HYD_STOP_MAX_LEN;
                    if (c + 1 < sl || st[sl - 1] != tk) continue;  // (never in front of column 0; the last token decides most cases)
                    const int64_t* w = row + (c + 1 - sl);  // may reach into columns written by earlier steps
                    bool match = true;
                    for (int j = 0; match && j < sl - 1; ++j) match = w[j] == st[j];
                    if (!match) continue;
                    r = 2;
                    which = k;
                    if (!s.include_stop) {
                        for (int j = 0; j < sl; ++j) row[c + 1 - sl + j] = a.pad;
                        trim = sl;
                    }
                }
                if (r != 0) e = i + 1;
            }
            if (s.gen) {  // the e judged tokens go behind the sequence's list: plain vector stores, positions < gen_stride only
                const int gl = s.gen_len[b];
                int32_t* g = s.gen + (int64_t)b * s.gen_stride;
                for (int i = 0; i < e; ++i)
                    if (gl + i >= 0 && gl + i < s.gen_stride) g[gl + i] = (int32_t)smp[i];
                s.gen_len[b] = gl + e;
            }
            last = smp[e - 1];
            len += e - trim;
            emitted = e;
            a.length[b] = len;
            if (STATES) state[b] = after[(int64_t)b * T + e - 1];
            if (r != 0) {
                a.reason[b] = r;
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

int launch_draft_accept_stop(const hyd_draft_accept_params& p, const DraftStopArgs& s, const int32_t* step_state_after, int32_t* state, hipStream_t st) {
    const int grid = (p.rows + 63) / 64;
    if (grid == 0) return 0;
    if (state) hipLaunchKernelGGL(draft_accept_stop_kernel<true>, dim3(grid), dim3(64), 0, st, p, s, step_state_after, state);
    else hipLaunchKernelGGL(draft_accept_stop_kernel<false>, dim3(grid), dim3(64), 0, st, p, s, (const int32_t*)nullptr, (int32_t*)nullptr);
    return (int)hipGetLastError();
}

}  // namespace hyd
