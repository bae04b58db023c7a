// hyd_sample_tokens_penalized: sample_filter.hip's row (sample_select.h sample_row) over PENALISED logits -- repetition /
// presence / frequency penalties and a sparse logit bias (include/hydragen_hip.h) -- and
// hyd_token_bitmap_build, the presence bitmap of a prompt's token ids.
//
//   * Nothing of size [rows, n] exists.  What a row needs to turn (index, logit) into x lives in the workgroup's LDS, built
//     by a prologue:
//       ctx   the row's context bitmap, the OR of its row of every context bitmap (a shared prompt is ONE bitmap row for all
//             the rows below it): n / 8 bytes, 16 KB at n = 128256.  Rows wider than kCtxWords * 32 tokens keep it in global
//             memory and OR the levels' bytes at every read;
//       tab   an open-addressing table (kSlots keys, linear probing, LDS compare-and-swap) of the row's generated tokens with
//             their counts and of the bias ids with their list positions: at most HYD_SAMPLE_GEN_MAX + HYD_SAMPLE_BIAS_MAX
//             = 3072 of 4096 slots.  Counts are integer atomics: the table's CONTENT does not depend on the insertion order;
//       slow  one bit per 8-token chunk (folded modulo kSlowBits) that says "a token of this chunk may be in tab".
//   * Every pass maps a chunk before the select sees it.  A chunk with no ctx byte and no slow bit -- the bulk of the
//     vocabulary -- costs one LDS byte, one LDS bit and, for 16-bit rows, the fp32 keys.  A touched token is evaluated in
//     double from its logit and rounded once to fp32.
//   * x is an fp32 value even for 16-bit rows: the keys are the fp32 ones and the select runs 4 radix levels.
// 1024 threads per row as sample_filter.hip; LDS 70.4 KB per workgroup: two rows per CU (160 KB).
#include "sample_penalty_map.h"  // the map, its tables' prologue and the append: shared with sample_constrain.hip

namespace hyd {

template <int DT>
__global__ __launch_bounds__(1024) void sample_penalty_kernel(const PenaltyArgs a) {
    __shared__ uint32_t ctx[kCtxWords];
    __shared__ uint32_t slow[kSlowBits / 32];
    __shared__ int keys[kSlots];
    __shared__ uint32_t vals[kSlots];
    const int row = blockIdx.x, t = threadIdx.x;
    const bool ctx_lds = a.words <= kCtxWords;
    penalty_tables(a, row, t, ctx_lds, ctx, slow, keys, vals);

    PenaltyMapT<DT> map{{a, ctx_lds ? ctx : nullptr, slow, keys, vals, row}};
    const int tok = sample_row<DT, 32>(a.f, map);
    if (t == 0 && a.append_out) penalty_append(a, row, tok);  // (every read of gen / gen_len above is behind sample_row's barriers)
}

int launch_sample_penalty(const PenaltyArgs& a, int dtype, hipStream_t s) {
    if (a.f.rows == 0) return 0;
    const dim3 grid((unsigned)a.f.rows), block(kFT);
    if (dtype == HYD_F16) hipLaunchKernelGGL((sample_penalty_kernel<HYD_F16>), grid, block, 0, s, a);
    else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_penalty_kernel<HYD_BF16>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sample_penalty_kernel<HYD_F32>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

// bits[g, v / 32] |= 1 << (v % 32) for the ids of group g: 256 threads per (group, 1024-id slice), one atomic OR per id
__global__ __launch_bounds__(256) void token_bitmap_kernel(const BitmapArgs a) {
    const int g = blockIdx.y;
    const int64_t len = a.lens ? (a.lens[g] < a.L ? a.lens[g] : a.L) : a.L;
    const int64_t j0 = (int64_t)blockIdx.x * 1024;  // (64-bit: L may sit within 1024 of INT32_MAX)
    for (int64_t j = j0 + threadIdx.x; j < j0 + 1024 && j < len; j += 256) {
        const int64_t v = a.ids[(int64_t)g * a.id_stride + j];
        if (v >= 0 && v < a.n) atomicOr(&a.bits[(int64_t)g * a.words + (v >> 5)], 1u << (v & 31));
    }
}

int launch_token_bitmap(const BitmapArgs& a, hipStream_t s) {
    if (a.groups == 0 || a.L == 0) return 0;
    const dim3 grid((unsigned)((a.L + 1023) / 1024), (unsigned)a.groups), block(256);
    hipLaunchKernelGGL(token_bitmap_kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hyd
