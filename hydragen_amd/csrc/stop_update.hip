// Stop conditions of a generation, decided on the device (hyd_stop_update, include/hydragen_hip.h states the rules): one thread
// per row judges the token the sampler just drew -- EOS ids, then the stop sequences against the row's own output so far --,
// writes column t of the output matrix and the row's length / finish reason, and produces what the next decode step is fed:
// the token, and a position that makes the RoPE + append kernel skip a finished row (cache index -1: no K/V written, length 0,
// so the row leaves the suffix pass).  The host never has to look at a token; it polls live[t], the running rows per step.
// A few hundred bytes per row and a handful of cached loads: the launch is latency, not work.
#include "hyd_kernels.h"

namespace hyd {

__global__ __launch_bounds__(64) void stop_update_kernel(const StopArgs a) {
    const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
    const int t = a.t;
    bool running = false;
    if (b < a.rows) {
        int64_t* row = a.out + (int64_t)b * a.out_stride;
        const int64_t tk = a.tok[b];
        int r = a.reason[b];
        if (r != 0) {
            row[t] = a.pad;  // (a) finished at an earlier step
        } else {
            row[t] = tk;
            int which = -1, kept = t + 1;
            for (int i = 0; i < a.n_eos; ++i) {  // (b) the EOS token is kept
                if (tk == a.eos[i]) {
                    r = 1;
                    which = i;
                    break;
                }
            }
            for (int k = 0; r == 0 && k < a.n_stop; ++k) {  // (c) list order: the lowest matching k wins
                const int len = a.stop_lens[k];
                const int64_t* s = a.stop_tokens + (int64_t)k * HYD_STOP_MAX_LEN;
                if (t + 1 < len || s[len - 1] != tk) continue;  // (never in front of step 0; the last token decides most cases)
                const int64_t* w = row + (t + 1 - len);
                bool match = true;
                for (int j = 0; match && j < len - 1; ++j) match = w[j] == s[j];
                if (!match) continue;
                r = 2;
                which = k;
                if (!a.include_stop) {
                    for (int j = 0; j < len; ++j) row[t + 1 - len + j] = a.pad;
                    kept = t + 1 - len;
                }
            }
            if (r == 0 && a.max_len && t + 1 >= a.max_len[b]) r = 3;  // the row's own limit (hyd_stop_update_rows): length t + 1, stop_index stays -1
            a.length[b] = kept;  // (d) a running row: t + 1
            if (r != 0) {
                a.reason[b] = r;
                a.stop_index[b] = which;
            }
        }
        running = r == 0;
        a.feed[b] = running ? tk : a.pad;
        a.next_pos[b] = (running || !a.retire) ? a.start_pos[b] + t : (a.shared_len ? a.shared_len[b] : 0) - 1;
    }
    // rows still running after this step: one vector atomic per wave that has any
    const unsigned long long m = __ballot(running);
    if (threadIdx.x == 0 && m != 0) atomicAdd(a.live + t, (int)__popcll(m));
}

int launch_stop_update(const StopArgs& a, hipStream_t s) {
    const int grid = (a.rows + 63) / 64;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(stop_update_kernel, dim3(grid), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
