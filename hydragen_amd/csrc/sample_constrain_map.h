// The token-automaton mask of sample_constrain.hip -- the Map that puts -inf behind the tokens a row's state does not allow -- and
// what its kernels do around sample_row with the row's state (MOVED here from sample_constrain.hip, not copied: that file's kernels
// compile to the same instructions as before the move), shared with sample_rows.hip.  sample_constrain.hip's header comment
// describes the mask.
#pragma once
#include "sample_penalty_map.h"

namespace hyd {

namespace {

template <int DT, int KB, typename Inner>
struct ConstrainMap {
    const Inner& inner;
    const uint8_t* allow;  // the allowed row of the workgroup's state (global memory), or null: unconstrained

    __device__ __forceinline__ void chunk(int c, float (&f)[8], uint32_t (&k)[8]) const {
        inner.chunk(c, f, k);
        if (allow) {
            const uint32_t b = allow[c];
            const uint32_t kinf = KB == 32 ? key32(0xff800000u) : key16(DT == HYD_F16 ? 0xfc00u : 0xff80u);  // (folded at compile time)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool ok = (b >> i) & 1u;
                f[i] = ok ? f[i] : -INFINITY;
                k[i] = ok ? k[i] : kinf;
            }
        }
    }
    __device__ __forceinline__ float one(int tok, float l) const {
        const float x = inner.one(tok, l);
        return (allow && !((allow[tok >> 3] >> (tok & 7)) & 1u)) ? -INFINITY : x;
    }
};

// the workgroup's state (-1 for an unconstrained row) and the allowed row of a state
__device__ __forceinline__ int row_state(const ConstrainArgs& c, int row) {
    const int s = c.state[row];
    return s >= 0 && s < c.n_states ? s : -1;
}
__device__ __forceinline__ const uint8_t* allowed_row(const ConstrainArgs& c, int st) {
    return st >= 0 ? reinterpret_cast<const uint8_t*>(c.allowed + (int64_t)st * c.allowed_stride) : nullptr;
}

// What thread 0 needs after the draw, parked in LDS before it: the address of next[st, 0] (null: nothing to store) and of
// state[row].  Kept in scalar registers across the whole row they cost the penalised kernel a stack slot (104 SGPRs in use).
struct Late {
    const int32_t* next_row;
    int32_t* state;
};
__device__ __forceinline__ void park(const ConstrainArgs& c, int row, int st, Late* late) {
    if (threadIdx.x == 0) {
        late->next_row = (c.advance && st >= 0) ? c.next + (int64_t)st * c.next_stride : nullptr;
        late->state = c.state + row;
    }
}
// After sample_row, every thread: thread 0 stores next[st, tok].  sample_row returns 0 on EVERY thread of a row without a valid
// logit and -1 on the threads other than 0 of a row that drew: thread 1's value tells the two apart.
__device__ __forceinline__ void store_next_state(const Late* late, int tok) {
    const int other = __shfl(tok, 1);
    if (threadIdx.x == 0 && other != 0) {
        const int32_t* next_row = late->next_row;
        if (next_row) *late->state = next_row[tok];
    }
}

}  // namespace

}  // namespace hyd
