// Kernel argument blocks + launcher prototypes shared by the C-ABI layer (api.hip) and the kernels.
#pragma once
#include "hyd_common.h"

namespace hyd {

constexpr int kMaxCombine = 64;  // (f32_mask of CombineArgs is 64 bits wide)
constexpr int HYD_MIXED = 3;     // CombineArgs.dtype_in only: the partials are a mix of fp32 and the 16-bit output dtype  // partials one combine launch / one suffix epilogue can merge

// Division by a launch constant without a divide on the device (Granlund & Montgomery, round-up method, exact for every
// 32-bit n and d >= 1): q = (t + ((n - t) >> sh1)) >> sh2 with t = mulhi(mul, n).  The host fills it (make_fastdiv).
struct FastDiv {
    uint32_t mul;
    uint32_t sh;  // sh1 | sh2 << 8
};
inline FastDiv make_fastdiv(uint32_t d) {
    uint32_t l = 0;
    while (l < 32 && (uint64_t(1) << l) < d) ++l;  // ceil(log2 d)
    FastDiv f;
    f.mul = (uint32_t)(((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1);
    f.sh = (l < 1 ? l : 1) | ((l > 1 ? l - 1 : 0) << 8);
    return f;
}

struct PrefixArgs {
    const void* q;
    const void* k;
    const void* v;
    void* out;   // dtype [..] or fp32 when out_f32; split sp writes at out + sp*out_split_stride
    float* lse;  // may be null
    const int32_t* cu_k;
    const int32_t* cu_q;
    int64_t k_gs, k_ts, k_hs, v_gs, v_ts, v_hs;
    int64_t out_split_stride;  // elements
    int64_t lse_split_stride;  // elements
    int32_t B, nq, Hq, Hkv, g, sb, per;
    int32_t kv_len;
    int32_t lse_q_stride;  // BHQ layout: query tokens per group
    int32_t row_blocks, nsplit, split_len;
    int32_t vgrid;    // units = sb * Hkv * nsplit * row_blocks; the launch grid may be smaller (persistent workgroups)
    int32_t wg_rows;  // query rows per workgroup: 128, or 256 (pipelined kernel, D = 128, large row counts)
    int32_t waves;    // waves per workgroup: 4 (one per SIMD, 64-row waves) or 8 (two per SIMD, 32-row waves; D = 128)
    int32_t lse_layout, out_f32;
    float scale_log2e;
    FastDiv div_row_blocks, div_nsplit, div_hkv, div_g;  // the unit / row decode divides by these four
    int32_t dbg;  // 0 in product builds; HYD_ABLATION_BUILD reads HYD_DBG to pick a timing-ablation variant of a prefix kernel
};

struct PartialDev {
    const void* out;
    const float* lse;
    int32_t is_f32;
    int32_t pad;
};

struct SuffixArgs {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    float* lse;
    const int32_t* sl32;
    const int64_t* sl64;
    const int32_t* order;  // optional permutation of the sequences: the unit in dispatch slot i works on sequence order[i] (hyd_suffix_params.seq_order)
    int64_t k_bs, k_ts, k_hs, v_bs, v_ts, v_hs;
    int32_t B, nq, Hq, Hkv, g, kv_len;
    int32_t rows;  // nq * g
    int32_t units; // B * Hkv
    int32_t n_partials;
    float scale_log2e;
    int32_t packed;  // shapes allow the lane-group path for short sequences (set by launch_suffix)
    int32_t n_pre;   // leading 16-bit partials the kernels fetch under the K/V stream (0..2, set by run_suffix)
    int32_t rows_wps_log2;  // token-row kernel (suffix_attn.hip): log2 of the waves of a workgroup that share one sequence (set by its launcher)
    int32_t dbg_blind;  // 0 in product builds; HYD_ABLATION_BUILD: HYD_GQA_BLIND=1 restores the blind first key step of the grouped-query kernel (A/B)
    int32_t shared_kv;  // the keys are read by several workgroups (a small shared level on the grouped-query kernel): no non-temporal hint
    int32_t kv_dim;     // 0, or the elements per head of NARROW unique cache rows (16 <= kv_dim < D, % 16 == 0; token-row kernel only); sits in what was padding
    // grouped-query kernel only: a shared-prefix segment walked before the unit's own keys (tiny problems: the whole
    // operator in one launch).  Sequence b reads rows [0, p_len) of group b / p_per; token strides equal k_ts / v_ts.
    const void* pk;
    const void* pv;
    int64_t pk_gs, pk_hs, pv_gs, pv_hs;
    int32_t p_len, p_per;
    PartialDev partials[kMaxCombine];
};

// fp8 unique caches (hyd_kv_quant): the argument block of the existing kernel plus the per-kv-head scales ([Hkv] or null = 1).
// The scales travel in front so that the fields the kernels read first stay within the first scalar-cache lines.
struct SuffixKvqArgs {
    const float* k_scale;
    const float* v_scale;
    SuffixArgs a;
};

struct CombineArgs {
    const void* outs[kMaxCombine];
    const float* lses[kMaxCombine];
    void* out;
    float* out_lse;
    int64_t rows;
    int32_t n, D, dtype_in, dtype_out;  // dtype_in may be HYD_F32 with a 16-bit dtype_out; HYD_MIXED: per-partial, f32_mask
    uint64_t f32_mask;                  // dtype_in == HYD_MIXED: bit i set = partial i is fp32, else it has dtype_out
    // optional BHQ re-layout of out_lse: row = tok*Hq + h -> ((tok / qpg)*Hq + h)*qpg + tok % qpg
    int32_t lse_layout, Hq, qpg;
    int32_t scalar_only;  // force the element-wise kernel (unaligned tensors)
};

struct RopeArgs {  // rope_append.hip, every form of the preamble; the defaults describe the plain one-token call on 16-bit caches
    const void* q = nullptr;
    const void* k = nullptr;
    const void* v = nullptr;
    void* q_out = nullptr;
    void* k_cache = nullptr;
    void* v_cache = nullptr;
    const float* cos = nullptr;
    const float* sin = nullptr;
    const int64_t* pos = nullptr;
    const int64_t* shared_len = nullptr;  // may be null
    int32_t* seq_lens = nullptr;
    int64_t q_bs = 0, k_bs = 0, v_bs = 0;  // batch strides of q/k/v (elements); heads contiguous
    int64_t q_ts = 0, k_ts = 0, v_ts = 0;  // their token strides (T > 1)
    int64_t kc_bs = 0, kc_ts = 0, kc_hs = 0, vc_bs = 0, vc_ts = 0, vc_hs = 0;  // elements; bytes with fp8
    int64_t pos_stride = 0, cs_stride = 0;
    const float* k_scale = nullptr;  // fp8: [Hkv] or null = 1
    const float* v_scale = nullptr;
    const void* q_weight = nullptr;  // per-head q/k RMSNorm in front of the rotation: gains [D] of the q dtype, or both null = no norm
    const void* k_weight = nullptr;
    float eps = 0.f;
    int32_t B = 0, Hq = 0, Hkv = 0, cache_len = 0, max_pos = 0;
    int32_t T = 1;         // tokens per batch row; q / k / v are [B, T, H, d]
    int32_t D = 0, d = 0;  // the kernels' head dim (64 / 128 / 256) and the rows' width: d < D = narrow rows, q_out keeps the pitch D (zero pad columns)
    int32_t fp8 = 0;       // k_cache / v_cache hold e4m3fn bytes
};

struct NormArgs {  // layer_ops.hip: h = residual + x; normed = RMSNorm(h) * weight
    const void* x;
    const void* residual;  // may be null (plain RMSNorm of x)
    const void* weight;
    void* sum_out;         // may be null
    void* norm_out;
    int64_t x_rs, r_rs, s_rs, o_rs;  // row strides (elements)
    int64_t rows;
    int32_t n;
    float eps;
};

struct SwigluArgs {  // layer_ops.hip: out = silu(gate) * up
    const void* gate;
    const void* up;
    void* out;
    int64_t g_rs, u_rs, o_rs;  // row strides (elements)
    int64_t rows;
    int32_t n;
};

struct SampleArgs {  // layer_ops.hip: out[row] ~ softmax(logits[row] / T) (Gumbel-max), or argmax when inv_temperature == 0
    const void* logits;
    int64_t* out;
    int64_t row_stride;  // elements
    uint64_t seed, offset;
    int32_t rows, n;
    float inv_temperature;
    int32_t vec_ok;      // rows are 16-byte aligned
};

struct FilterArgs {  // sample_filter.hip: SampleArgs' draw over the tokens that survive top-k / top-p / min-p
    const void* logits;
    int64_t* out;
    float* logprobs;     // may be null
    int32_t* kept;       // may be null
    int64_t row_stride;  // elements
    uint64_t seed, offset;
    int32_t rows, n;
    float inv_temperature;
    int32_t top_k;       // 0 = off
    float top_p;         // >= 1 = off
    float log_min_p;     // ln(min_p); -inf = off
    int32_t vec_ok;      // rows are 16-byte aligned
};

constexpr int kMaxContext = HYD_MAX_LEVELS + 1;
struct PenaltyArgs {  // sample_penalty.hip: FilterArgs' kernel over penalised logits (hyd_sample_tokens_penalized)
    FilterArgs f;
    double rep, inv_rep, freq, pres;  // 1, 1, 0, 0 = off; inv_rep = 1 / rep (no fp64 division in the kernel)
    const uint32_t* ctx[kMaxContext];  // [groups, words] presence bitmaps
    int32_t ctx_rpg[kMaxContext];    // rows per bitmap row
    int32_t n_ctx, words;            // words = ceil(n / 32)
    int32_t* gen;                    // [rows, gen_stride] or null
    int32_t* gen_len;
    int32_t gen_stride, append_out;
    const int64_t* bias_ids;
    const float* bias_values;
    int32_t n_bias;
};

struct ConstrainArgs {  // sample_constrain.hip: the token automaton of hyd_sample_tokens_constrained (hyd_token_dfa)
    const uint32_t* allowed;  // [n_states, allowed_stride] words
    const int32_t* next;      // [n_states, next_stride]
    int32_t* state;           // [rows]
    int64_t allowed_stride, next_stride;
    int32_t n_states, advance;
};

struct RowParams {  // sample_rows.hip: per-row sampling values (hyd_sample_tokens_rows), each [rows] or null = the launch's scalar
    const float* temperature;
    const int32_t* top_k;
    const float* top_p;
    const float* min_p;
    const float* rep;
    const float* freq;
    const float* pres;
    const uint64_t* seed;
};
struct NoRowParams {};  // the scalar launches: every value is the argument block's

struct BitmapArgs {  // sample_penalty.hip: token ids -> presence bitmap (hyd_token_bitmap_build)
    const int64_t* ids;
    const int64_t* lens;  // may be null
    uint32_t* bits;
    int64_t id_stride;
    int32_t groups, L, n, words;
};

struct TokenLogprobArgs {  // token_logprob.hip: log-probs of given tokens, greedy flags, top-N alternatives
    const void* logits;
    const int64_t* targets;
    float* logprobs;
    uint8_t* greedy;
    int64_t* top_ids;       // [rows, top_n]; unused when top_n == 0
    float* top_logprobs;
    int64_t row_stride;     // elements
    int64_t rows, row0;     // row0: first row of this launch
    int32_t n, top_n;
    int32_t vec_ok;         // rows are 16-byte aligned
};

struct StopArgs {  // stop_update.hip: EOS ids / stop sequences judged per row, the next step's token and position (hyd_stop_update)
    const int64_t* tok;
    int64_t* out;
    int32_t* length;
    int32_t* reason;
    int32_t* stop_index;
    int32_t* live;
    const int64_t* stop_tokens;  // [n_stop, HYD_STOP_MAX_LEN]
    const int64_t* start_pos;
    const int64_t* shared_len;   // may be null
    int64_t* feed;
    int64_t* next_pos;
    int64_t out_stride, pad;
    int64_t eos[HYD_STOP_MAX_EOS];
    int32_t stop_lens[HYD_STOP_MAX_SEQS];
    int32_t rows, t, n_eos, n_stop, include_stop, retire;
    const int32_t* max_len;      // [rows] or null: a row's own token limit (hyd_stop_update_rows)
};

struct DraftStopArgs {  // draft_accept_stop.hip: what hyd_draft_accept_stop reads beside hyd_draft_accept_params
    const int64_t* stop_tokens;  // [n_stop, HYD_STOP_MAX_LEN] or null
    int32_t* gen;                // [rows, gen_stride] or null: the penalties' per-sequence token lists
    int32_t* gen_len;
    int32_t stop_lens[HYD_STOP_MAX_SEQS];
    int32_t n_stop, include_stop, gen_stride, reserved;
};

struct KvPromoteArgs {  // kv_promote.hip: chosen rows of the unique K/V caches -> a packed shared level (hyd_kv_promote)
    const void* k_src;
    const void* v_src;
    void* k_dst;
    void* v_dst;
    const int32_t* rows;
    const int32_t* lens;
    const int32_t* cu;
    const float* k_scale;  // fp8 sources: [Hkv] or null = 1
    const float* v_scale;
    int64_t k_bs, k_ts, k_hs, v_bs, v_ts, v_hs;  // source strides (elements)
    int32_t n, B, max_len, capacity;
    int32_t d_src;
    int32_t vec_per_head, vec_per_tok;  // 16-byte vectors of a destination head row (d_dst / 8) and token row (Hkv * d_dst / 8)
    FastDiv div_vec_per_head, div_vec_per_tok;
};

struct KvGatherArgs {  // kv_gather.hip: each survivor's path -- its parents' sequences in a chain of levels, then its unique rows -- into one packed level
    const void* lk[HYD_MAX_LEVELS];       // chain level j: packed [cap_j, Hkv, d_dst] K / V of the destination dtype
    const void* lv[HYD_MAX_LEVELS];
    const int32_t* lcu[HYD_MAX_LEVELS];   // [s_j + 1] token offsets of its sequences
    int32_t ls[HYD_MAX_LEVELS], lcap[HYD_MAX_LEVELS];
    FastDiv ldiv[HYD_MAX_LEVELS];         // parent of unique row r in level j: r / div_j
    KvPromoteArgs u;                      // the unique segment and the destination, as hyd_kv_promote has them (u.cu: cu_dst)
    int32_t n_levels, max_path;
};

struct KvAbsmaxArgs {  // kv_scale.hip: per-kv-head max |x| of a strided 16-bit view [n_outer, n_rows, Hkv, d] (hyd_kv_absmax)
    const void* k;
    const void* v;
    const int32_t* row_lens;  // [n_outer] or null = n_rows
    unsigned* amax;           // f32 [2, Hkv] as bit patterns (non-negative floats order as their bits)
    int64_t k_os, k_rs, k_hs, v_os, v_rs, v_hs;  // outer / row / head strides (elements)
    int32_t Hkv, n_outer, n_rows;
    int32_t pph, vpr;     // 16-byte pieces of a head row (d / 8) and of a token row (Hkv * d / 8)
    int32_t cols, rstep;  // piece columns a workgroup covers (min(vpr, 256)) and the rows it takes side by side (256 / cols)
    int32_t group;        // the largest power of two that divides pph: lanes that meet by shuffles
    int32_t chunks;       // workgroups along the rows of one outer: ceil(n_rows / (HYD_KV_ABSMAX_PASSES * rstep))
    int32_t only;         // 0: K and V; 1: K alone; 2: V alone
    FastDiv div_pph, div_cols, div_chunks;
};

struct KvScalesArgs {  // kv_scale.hip: amax [2, Hkv] -> k_scale / v_scale [Hkv] (hyd_kv_scales_from_absmax)
    const float* amax;
    float* k_scale;
    float* v_scale;
    int32_t Hkv, pow2;
    float c;
};

struct LinearW8Plan {  // linear_w8.hip: the launch plan of hyd_linear_w8, from M, N and K alone
    int32_t mt;       // 16-row MFMA tiles of x a workgroup carries: 1 / 2 (linear_w8_kernel), 4 / 8 (linear_w8_rows_kernel)
    int32_t mtiles;   // workgroups along M: ceil(M / (16 * mt))
    int32_t ngroups;  // workgroups along N: ceil(N / 32), or ceil(N / 128) for the rows kernel
    int32_t steps;    // 128-deep steps along K: ceil(K / 128)
    int32_t splits;   // workgroups along K; > 1: fp32 partial sums in the workspace, reduced by a second launch
    int64_t np;       // N rounded up to 4: the row length of a partial-sum slice
    size_t bytes;     // workspace: splits > 1 ? splits * M * np * 4 : 0
};

struct LinearW8Args {  // linear_w8.hip: y = round16(scale * (x . w8^T))
    const void* x;
    const uint8_t* w8;
    const float* scale;
    void* y;
    float* ws;
    int64_t xs, ys, np;  // row strides of x / y (elements) and of a partial-sum slice (floats)
    int32_t M, N, K;
    int32_t mtiles, steps, splits;
};

struct WeightWidenArgs {  // linear_w8.hip: out = dequantize_weight(w8, scale)
    const uint8_t* w8;
    const float* scale;
    void* out;
    int64_t os;
    int32_t N, K;
};

// launchers (defined next to the kernels); return hipError_t as int
LinearW8Plan plan_linear_w8(int M, int N, int K);                                        // linear_w8.hip, shapes only
int launch_linear_w8(const LinearW8Args& a, const LinearW8Plan& pl, int dtype, hipStream_t s);  // linear_w8.hip
int launch_weight_widen(const WeightWidenArgs& a, int dtype, hipStream_t s);             // linear_w8.hip
int launch_kv_absmax(const KvAbsmaxArgs& a, int dtype, hipStream_t s);  // kv_scale.hip
int launch_kv_scales(const KvScalesArgs& a, hipStream_t s);             // kv_scale.hip
int launch_kv_promote(const KvPromoteArgs& a, int src_dtype, int dst_dtype, hipStream_t s);  // kv_promote.hip
int launch_kv_gather(const KvGatherArgs& a, int src_dtype, int dst_dtype, hipStream_t s);    // kv_gather.hip
int launch_prefix_w64(const PrefixArgs& a, int dtype, int D, bool causal, int grid, hipStream_t s);
int launch_prefix_w64_f16(const PrefixArgs& a, int D, bool causal, int grid, hipStream_t s);  // prefix_attn_w64_f16.hip
int launch_rope_append(const RopeArgs& a, int dtype, hipStream_t s);  // rope_append.hip: the kernel is picked from a's fields
int launch_add_rmsnorm(const NormArgs& a, int dtype, hipStream_t s);
int launch_swiglu(const SwigluArgs& a, int dtype, hipStream_t s);
int launch_sample(const SampleArgs& a, int dtype, hipStream_t s);
int launch_sample_filter(const FilterArgs& a, int dtype, hipStream_t s);  // sample_filter.hip
int launch_sample_penalty(const PenaltyArgs& a, int dtype, hipStream_t s);     // sample_penalty.hip
int launch_sample_constrain(const PenaltyArgs& a, const ConstrainArgs& c, bool neutral, int dtype, hipStream_t s);  // sample_constrain.hip
int launch_sample_rows(const PenaltyArgs& a, const ConstrainArgs* c, const RowParams& r, bool neutral, int dtype, hipStream_t s);  // sample_rows.hip
int launch_token_bitmap(const BitmapArgs& a, hipStream_t s);                     // sample_penalty.hip
int launch_token_logprob(const TokenLogprobArgs& a, int dtype, hipStream_t s);  // token_logprob.hip
int launch_stop_update(const StopArgs& a, hipStream_t s);                          // stop_update.hip
int launch_suffix(const SuffixArgs& a, int dtype, int D, hipStream_t s);
bool suffix_narrow_eligible(const SuffixArgs& a, int D);                              // suffix_attn.hip, shapes only (a.kv_dim set)
bool suffix_gqa_eligible(const SuffixArgs& a, int D, bool any_shape);
bool suffix_fp8_eligible(const SuffixArgs& a, int D);                                 // suffix_attn_fp8.hip, shapes only
int launch_suffix_fp8(const SuffixKvqArgs& a, int dtype, int D, hipStream_t s);       // q dtype; K/V e4m3fn
bool suffix_gqa_fp8_eligible(const SuffixArgs& a, int D);                             // suffix_attn_gqa_fp8.hip, shapes only
int launch_suffix_gqa_fp8(const SuffixKvqArgs& a, int dtype, int D, hipStream_t s);   // q dtype; K/V e4m3fn, grouped-query shapes
bool suffix_gqa_fp8_causal_eligible(const SuffixArgs& a, int D);                      // suffix_attn_gqa_fp8_causal.hip, shapes only
int launch_suffix_gqa_fp8_causal(const SuffixKvqArgs& a, int dtype, int D, hipStream_t s);  // the causal tail over fp8 caches (nq = 2..8)
int launch_suffix_gqa(const SuffixArgs& a, int dtype, int D, hipStream_t s);
bool suffix_causal_eligible(const SuffixArgs& a, int D);                              // suffix_attn_causal.hip, shapes only
int launch_suffix_causal(const SuffixArgs& a, int dtype, int D, hipStream_t s);       // the causal-tail suffix pass (nq = 2..8)
// speculative decoding: these kernels take the validated public parameter blocks as they are
int launch_draft_lookup(const hyd_draft_lookup_params& p, hipStream_t s);             // draft_lookup.hip
int launch_draft_accept(const hyd_draft_accept_params& p, hipStream_t s);             // draft_accept.hip
int launch_draft_accept_states(const hyd_draft_accept_params& p, const int32_t* step_state_after, int32_t* state, hipStream_t s);
int launch_draft_accept_stop(const hyd_draft_accept_params& p, const DraftStopArgs& s, const int32_t* step_state_after, int32_t* state,
                             hipStream_t st);                                          // draft_accept_stop.hip (state null: no states)
int launch_sample_penalty_drafts(const PenaltyArgs& a, const int64_t* fed, int T, int dtype, hipStream_t s);  // sample_penalty_drafts.hip
int launch_dfa_forced(const hyd_dfa_forced_params& p, hipStream_t s);                 // draft_constrain.hip
int launch_draft_constrain(const hyd_draft_constrain_params& p, hipStream_t s);       // draft_constrain.hip
int launch_combine(const CombineArgs& a, hipStream_t s);
size_t allreduce_block_bytes(int world, size_t max_bytes);
int launch_allreduce(char* const* blocks, size_t block_bytes, const void* in, void* out, int64_t count, int dtype,
                     int rank, int world, size_t max_bytes, int timeout_log2_polls, hipStream_t s);

}  // namespace hyd
