// hyd_sample_tokens_constrained: the row of hyd_sample_tokens_penalized (sample_select.h sample_row) behind a token-automaton
// mask (include/hydragen_hip.h).  A row in state s of the automaton may only emit the tokens whose bit is set in
// row s of `allowed`; after the draw its state becomes next[s, token].
//
//   * The mask is one more Map around the row's map: the inner map runs (NoMap, or the penalty map of sample_penalty_map.h),
//     then the lanes whose bit is clear get -inf and the key of -inf.  That is one byte of the allowed row per 8-token chunk and
//     pass.  -inf is absorbing under every penalty rule and never kept, so the result is what the existing kernels give on
//     masked_fill'ed logits, bit for bit (tests/test_constraint_gpu.py).
//   * The allowed row (n / 8 bytes, shared by every batch row in that state) is read from global memory in both families: the
//     penalised kernel's 70.4 KB of LDS leave no room for it at two rows per CU, and it is L2-resident after the first
//     workgroup of a state has read it.
//   * Two families, chosen on the host: every penalty neutral -> NoMap inside and the keys of the row's own width (the cost of
//     sample_filter.hip plus the bitmap bytes); otherwise the penalty map inside, fp32 keys, sample_penalty.hip's prologue.
//   * A row whose state is outside [0, n_states) skips the wrap and keeps its state: no address is ever formed from such a state.
//     Thread 0 stores the new state after the draw (a plain vector store); a row without a valid logit keeps its state.
#include "sample_constrain_map.h"  // the mask and the state update: shared with sample_rows.hip

namespace hyd {

template <int DT>
__global__ __launch_bounds__(1024) void sample_constrain_kernel(const FilterArgs a, const ConstrainArgs c) {
    constexpr int KB = DT == HYD_F32 ? 32 : 16;
    const int row = blockIdx.x;
    const int st = row_state(c, row);
    const NoMap inner;
    const ConstrainMap<DT, KB, NoMap> map{inner, allowed_row(c, st)};
    __shared__ Late late;
    park(c, row, st, &late);
    const int tok = sample_row<DT, KB>(a, map);
    store_next_state(&late, tok);  // (the read of state[row] above is behind sample_row's barriers)
}

template <int DT>
__global__ __launch_bounds__(1024) void sample_constrain_penalty_kernel(const PenaltyArgs a, const ConstrainArgs c) {
    __shared__ uint32_t ctx[kCtxWords];
    __shared__ uint32_t slow[kSlowBits / 32];
    __shared__ int keys[kSlots];
    __shared__ uint32_t vals[kSlots];
    const int row = blockIdx.x, t = threadIdx.x;
    const bool ctx_lds = a.words <= kCtxWords;
    penalty_tables(a, row, t, ctx_lds, ctx, slow, keys, vals);

    const int st = row_state(c, row);
    const PenaltyMapT<DT> inner{{a, ctx_lds ? ctx : nullptr, slow, keys, vals, row}};
    const ConstrainMap<DT, 32, PenaltyMapT<DT>> map{inner, allowed_row(c, st)};
    __shared__ Late late;
    park(c, row, st, &late);
    const int tok = sample_row<DT, 32>(a.f, map);
    if (t == 0 && a.append_out) penalty_append(a, row, tok);
    store_next_state(&late, tok);
}

int launch_sample_constrain(const PenaltyArgs& a, const ConstrainArgs& c, bool neutral, int dtype, hipStream_t s) {
    if (a.f.rows == 0) return 0;
    const dim3 grid((unsigned)a.f.rows), block(kFT);
    if (neutral) {
        if (dtype == HYD_F16) hipLaunchKernelGGL((sample_constrain_kernel<HYD_F16>), grid, block, 0, s, a.f, c);
        else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_constrain_kernel<HYD_BF16>), grid, block, 0, s, a.f, c);
        else hipLaunchKernelGGL((sample_constrain_kernel<HYD_F32>), grid, block, 0, s, a.f, c);
    } else {
        if (dtype == HYD_F16) hipLaunchKernelGGL((sample_constrain_penalty_kernel<HYD_F16>), grid, block, 0, s, a, c);
        else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_constrain_penalty_kernel<HYD_BF16>), grid, block, 0, s, a, c);
        else hipLaunchKernelGGL((sample_constrain_penalty_kernel<HYD_F32>), grid, block, 0, s, a, c);
    }
    return (int)hipGetLastError();
}

}  // namespace hyd
