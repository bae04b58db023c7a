// hyd_sample_tokens_penalized_drafts: sample_penalty.hip's row over the B * T logits rows of a speculative step, with ONE list of
// generated tokens per sequence (include/hydragen_hip.h).  Logits row r belongs to sequence b = r / T and fed
// position i = r % T: its draw is conditioned on the drafts fed[b, 1 .. i] in front of it, so they count as generated tokens --
// otherwise the draw is not from the target distribution given that prefix and the scheme is no longer lossless.
//   * The prologue is penalty_tables (sample_penalty_map.h, untouched) for row b -- context bitmaps at b / rows_per_group, the
//     sequence's list, the bias ids -- and then up to 7 more insertions, one thread each, of the drafts.  Counts are integer
//     atomics: the table's CONTENT is that of the explicit list gen[b] ++ fed[b, 1 .. i], whatever the insertion order, and the
//     map reads content only.  At most 2048 + 7 + 1024 of the 4096 slots are used.
//   * Everything behind the prologue is the existing row for logits row r: cuts, noise from (seed, offset, r), log-prob, kept.
//   * Nothing is appended: on this route the accept (draft_accept_stop.hip) owns the lists.
// 1024 threads per row, the LDS of sample_penalty.hip: two rows per CU.
#include "sample_penalty_map.h"

namespace hyd {

template <int DT>
__global__ __launch_bounds__(1024) void sample_penalty_drafts_kernel(const PenaltyArgs a, const int64_t* fed, const int T) {
    __shared__ uint32_t ctx[kCtxWords];
    __shared__ uint32_t slow[kSlowBits / 32];
    __shared__ int keys[kSlots];
    __shared__ uint32_t vals[kSlots];
    const int row = blockIdx.x, t = threadIdx.x;
    const int b = row / T, i = row - b * T;
    const bool ctx_lds = a.words <= kCtxWords;
    penalty_tables(a, b, t, ctx_lds, ctx, slow, keys, vals);
    if (a.gen && t < i) {  // the drafts fed in front of this row's position (fed[b, 0] is the last emitted token: already in gen)
        const int64_t v64 = fed[(int64_t)b * T + 1 + t];
        if (v64 >= 0 && v64 < a.f.n) {
            const int v = (int)v64;
            uint32_t h = slot_of(v);
            for (;; h = (h + 1) & (kSlots - 1)) {
                const int old = atomicCAS(&keys[h], kEmpty, v);
                if (old == kEmpty || old == v) break;
            }
            atomicAdd(&vals[h], 1u);
            const int c = v >> 3;
            atomicOr(&slow[(c & (kSlowBits - 1)) >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();

    PenaltyMapT<DT> map{{a, ctx_lds ? ctx : nullptr, slow, keys, vals, b}};
    sample_row<DT, 32>(a.f, map);
}

int launch_sample_penalty_drafts(const PenaltyArgs& a, const int64_t* fed, int T, int dtype, hipStream_t s) {
    if (a.f.rows == 0) return 0;
    const dim3 grid((unsigned)a.f.rows), block(kFT);
    if (dtype == HYD_F16) hipLaunchKernelGGL((sample_penalty_drafts_kernel<HYD_F16>), grid, block, 0, s, a, fed, T);
    else if (dtype == HYD_BF16) hipLaunchKernelGGL((sample_penalty_drafts_kernel<HYD_BF16>), grid, block, 0, s, a, fed, T);
    else hipLaunchKernelGGL((sample_penalty_drafts_kernel<HYD_F32>), grid, block, 0, s, a, fed, T);
    return (int)hipGetLastError();
}

}  // namespace hyd
