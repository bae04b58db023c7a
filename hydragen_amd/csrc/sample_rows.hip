// hyd_sample_tokens_rows: the rows of hyd_sample_tokens_filtered / _penalized / _constrained with PER-ROW temperature, cuts,
// penalties and seeds (include/hydragen_hip.h).  The kernels of those entry points already run one workgroup per
// row and read every parameter as a block-uniform value; here the workgroup loads its row's values once, at the top, into the
// same block-uniform locals (sample_select.h RowVals, sample_penalty_map.h PenVals) and then runs the same text: sample_row over
// the same maps.  Nothing else differs, so a row's outputs are bit for bit those of a scalar launch with the row's values.
//
//   * Instantiations of their own, in a file of their own: the scalar kernels of sample_filter.hip, sample_penalty.hip and
//     sample_constrain.hip compile to the instructions they compiled to before (their NoRowParams form folds to the argument block).
//   * Two families, chosen on the host as in sample_constrain.hip: no penalty anywhere in the call (neutral scalars, no penalty
//     array, no bias, nothing to append) -> NoMap inside, keys of the row's own width, sample_filter.hip's cost; otherwise the
//     penalty map inside, fp32 keys and sample_penalty.hip's prologue.  The automaton's mask wraps either; without an automaton
//     (c.state null) every row is unconstrained and the wrap is skipped.
//   * The values are sanitised on the device (RowVals / PenVals state the rules) and only ever compared or multiplied: none forms
//     an address.  No LDS beyond what the scalar kernels hold, no scratch, no workspace.
#include "sample_constrain_map.h"

namespace hyd {

template <int DT>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const FilterArgs a, const ConstrainArgs c, const RowParams r) {
    constexpr int KB = DT == HYD_F32 ? 32 : 16;
    const int row = blockIdx.x;
    const int st = c.state ? row_state(c, row) : -1;
    const NoMap inner;
    const ConstrainMap<DT, KB, NoMap> map{inner, allowed_row(c, st)};
    __shared__ Late late;
    park(c, row, st, &late);
    const int tok = sample_row<DT, KB>(a, map, r);
    store_next_state(&late, tok);  // (the read of state[row] above is behind sample_row's barriers)
}

template <int DT>
__global__ __launch_bounds__(1024) void sample_rows_penalty_kernel(const PenaltyArgs a, const ConstrainArgs c, const RowParams r) {
    __shared__ uint32_t ctx[kCtxWords];
    __shared__ uint32_t slow[kSlowBits / 32];
    __shared__ int keys[kSlots];
    __shared__ uint32_t vals[kSlots];
    const int row = blockIdx.x, t = threadIdx.x;
    const bool ctx_lds = a.words <= kCtxWords;
    penalty_tables(a, row, t, ctx_lds, ctx, slow, keys, vals);

    const int st = c.state ? row_state(c, row) : -1;
    const PenaltyMapT<DT, PenVals> inner{{a, ctx_lds ? ctx : nullptr, slow, keys, vals, row, pen_vals(a, r, row)}};
    const ConstrainMap<DT, 32, PenaltyMapT<DT, PenVals>> map{inner, allowed_row(c, st)};
    __shared__ Late late;
    park(c, row, st, &late);
    const int tok = sample_row<DT, 32>(a.f, map, r);
    if (t == 0 && a.append_out) penalty_append(a, row, tok);
    store_next_state(&late, tok);
}

// c null: no automaton (ConstrainArgs of zeros: state null, nothing to advance)
int launch_sample_rows(const PenaltyArgs& a, const ConstrainArgs* c, const RowParams& r, bool neutral, int dtype, hipStream_t s) {
    if (a.f.rows == 0) return 0;
    const ConstrainArgs ca = c ? *c : ConstrainArgs{};
    const dim3 grid((unsigned)a.f.rows), block(kFT);
    if (neutral) {
        if (dtype == HYD_F16) hipLaunchKernelGGL((sample_rows_kernel<HYD_F16>), grid, block, 0, s, a.f, ca, r);
        else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_rows_kernel<HYD_BF16>), grid, block, 0, s, a.f, ca, r);
        else hipLaunchKernelGGL((sample_rows_kernel<HYD_F32>), grid, block, 0, s, a.f, ca, r);
    } else {
        if (dtype == HYD_F16) hipLaunchKernelGGL((sample_rows_penalty_kernel<HYD_F16>), grid, block, 0, s, a, ca, r);
        else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_rows_penalty_kernel<HYD_BF16>), grid, block, 0, s, a, ca, r);
        else hipLaunchKernelGGL((sample_rows_penalty_kernel<HYD_F32>), grid, block, 0, s, a, ca, r);
    }
    return (int)hipGetLastError();
}

}  // namespace hyd
