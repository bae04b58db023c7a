/*
 * hydragen_hip.h -- C ABI of libhydragen_hip.so: Hydragen's decomposed shared-prefix attention
 * (prefix pass + suffix pass + log-sum-exp combine) as hand-written HIP kernels for gfx950
 * (MI355X / CDNA4).
 *
 * This is the drop-in boundary for the reference's hot path.  Each entry point names the
 * reference interface it replaces (file:line relative to ScalingIntelligence/hydragen):
 *
 *   hyd_prefix_attn_fwd     hydragen/flash.py:284-306  flash_attention        (K1, K2c)
 *                           hydragen/flash.py:309-351  flash_attention_varlen (K1v)
 *                           i.e. flash-attn 2.3.6 _flash_attn_forward/_flash_attn_varlen_forward
 *                           as called from hydragen/attention.py:270,313,344
 *   hyd_suffix_attn_fwd     hydragen/flash.py:163-281  flash_attention_seqlen
 *                           (= xformers_stuff.py:189-428 _fwd_kernel_splitK + flash.py:76-160
 *                           _splitK_reduce), optionally with attention.py:352 combine fused in
 *   hyd_combine_lse         hydragen/attention.py:154-174 combine_lse (N partials; replaces both
 *                           combine_lse_triton :105-151 and combine_lse_torch :21-43)
 *   hyd_decode_attn_fused   hydragen/attention.py:177-354 hydragen_attention for the decode
 *                           case (seq_lens given): all shared levels + suffix + combine
 *   hyd_workspace_bytes     replaces the per-call torch.empty scratch of flash.py:199-204
 *
 * Conventions:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *   - the library never allocates device memory, never synchronises, reads no environment
 *     variable, holds no mutable global state, and launches only on the hipStream_t passed in
 *     (as void*): every call is HIP-graph-capture safe;
 *   - launch geometry is derived from shapes only, never from device data;
 *   - every call returns HYD_OK (0) or a negative error code; hyd_last_error_string() gives the
 *     message for the calling thread's last failure;
 *   - 16-bit dtypes: HYD_F16 (IEEE half) and HYD_BF16; accumulation, softmax and LSE are fp32.
 *   - q/out are [B, nq, Hq, D] contiguous; K/V tensors are token-major with explicit element
 *     strides and a contiguous head_dim; supported head_dim: 64, 128, 256.  Other head dims run zero-padded to the next of
 *     the three with the true dim's softmax scale; the UNIQUE K/V cache alone may keep rows of the true width d (d % 16 == 0;
 *     80 / 96 / 192 ...) without a padded copy: hyd_suffix_params.kv_dim, hyd_rope_params.head_dim.
 */
#ifndef HYDRAGEN_HIP_H
#define HYDRAGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: these entry points are its whole dynamic symbol table */
#define HYD_API __attribute__((visibility("default")))

/* 0.5.0 also carries the fp8 unique-cache entry points (hyd_kv_quant, hyd_*_kvq, hyd_kv_quant_supported) and the filtered
 * sampler (hyd_sample_filter_params, hyd_sample_tokens_filtered), the scoring entry point (hyd_token_logprob_params,
 * hyd_token_logprobs) and the penalised sampler (hyd_sample_penalty_params, hyd_sample_tokens_penalized, hyd_token_bitmap_build) and the stop-condition entry point (hyd_stop_params, hyd_stop_update) and the unique-to-shared K/V copy (hyd_kv_promote_params, hyd_kv_promote) and the path gather of a fork with merged levels (hyd_kv_gather_params, hyd_kv_gather_paths) and the fp8 scale calibration (hyd_kv_absmax_params, hyd_kv_absmax, hyd_kv_scales_params, hyd_kv_scales_from_absmax) and the fp8 linear-layer weights (hyd_linear_w8_params, hyd_linear_w8, hyd_linear_w8_workspace_bytes, hyd_weight_widen_params, hyd_weight_widen): they are new symbols and new structs only -- no existing struct, entry point or result changed -- so a caller built against 0.5.0 without them is
 * unaffected and the version stays 500. */
#define HYD_VERSION 500 /* 0.5.0: hyd_suffix_params.seq_order (schedule hint for ragged lengths); 0.4.0: hyd_add_rmsnorm, hyd_swiglu, hyd_sample_tokens (model-shell glue); 0.3.0: two-stream phases + hyd_decode_params.shared_max_workgroups, hyd_decode_two_stream_ok; 0.2.2: hyd_allreduce_params.timeout_log2_polls; 0.2.1: softmax_scale; 0.2.0: hyd_decode_params.phase, hyd_rope_params.max_pos, hyd_allreduce_* */
#define HYD_MAX_LEVELS 8

enum {
    HYD_OK = 0,
    HYD_ERR_BAD_ARG = -1,     /* null pointer, non-positive size, indivisible batch ...      */
    HYD_ERR_UNSUPPORTED = -2, /* dtype / head_dim / row count the kernels do not implement    */
    HYD_ERR_WORKSPACE = -3,   /* workspace missing or smaller than hyd_*_workspace_bytes says */
    HYD_ERR_LAUNCH = -4       /* hipLaunchKernel reported an error                            */
};

enum { HYD_F16 = 0, HYD_BF16 = 1, HYD_F32 = 2 /* hyd_combine_lse only */, HYD_FP8_E4M3 = 3 /* hyd_kv_quant.kv_dtype only */ };

/* LSE layouts: BQH = [B, nq, Hq] (what attention.py:276-280 re-lays flash's output into),
 *              BHQ = [sb, Hq, (B/sb)*nq] (what flash-attn returns, flash.py:295-306). */
enum { HYD_LSE_BQH = 0, HYD_LSE_BHQ = 1 };

/* ------------------------------------------------------------------------------------------
 * Prefix pass: batched-query attention of every query of a group against that group's single
 * shared K/V, on the MFMA matrix cores.  Sequence b belongs to group b / (B/sb)
 * (attention.py:264-268).  GQA: q-head h reads kv-head h / (Hq/Hkv).
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_prefix_params {
    const void* q;               /* [B, nq, Hq, D]                                             */
    const void* k;               /* group gi, token t, head h at k + gi*k_group_stride +       */
    const void* v;               /*   t*k_tok_stride + h*k_head_stride (elements); D contiguous */
    void* out;                   /* [B, nq, Hq, D] in dtype                                    */
    float* lse;                  /* may be NULL; natural log, softmax scale included           */
    const int32_t* cu_seqlens_k; /* NULL, or [sb+1]: group gi owns packed tokens               */
                                 /*   [cu[gi], cu[gi+1]) of k/v (k_group_stride ignored)        */
    const int32_t* cu_seqlens_q; /* NULL, or [sb+1] packed query tokens per group (then B is   */
                                 /*   the total number of query tokens and nq must be 1)       */
    void* workspace;             /* >= hyd_prefix_workspace_bytes(); may be NULL if that is 0  */
    size_t workspace_bytes;
    int64_t k_group_stride, k_tok_stride, k_head_stride;
    int64_t v_group_stride, v_tok_stride, v_head_stride;
    int32_t dtype;      /* HYD_F16 | HYD_BF16                                                  */
    int32_t B, nq, Hq, Hkv, D;
    int32_t sb;         /* number of groups (shared sequences); B % sb == 0                    */
    int32_t kv_len;     /* keys per group; with cu_seqlens_k: the maximum over groups          */
    int32_t max_q_len;  /* only with cu_seqlens_q: max query tokens per group                  */
    int32_t causal;     /* 0 | 1 (bottom-right aligned: query i sees keys j <= i + kv - nq)    */
    int32_t lse_layout; /* HYD_LSE_BQH | HYD_LSE_BHQ                                           */
    int32_t num_splits; /* split-KV factor; 0 = choose from shapes                             */
    float softmax_scale; /* 0 = D^-0.5 (what the reference always uses, flash.py:295-304); > 0: that
                          * scale -- lets a caller run a zero-padded head dim with the true one's scale */
    int32_t reserved_;
} hyd_prefix_params;

HYD_API size_t hyd_prefix_workspace_bytes(const hyd_prefix_params* p);
HYD_API int hyd_prefix_attn_fwd(const hyd_prefix_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Suffix pass: every query row of sequence b against the first seq_len[b] keys of b's own
 * K/V (non-causal), one wavefront per (sequence, kv-head), HBM-bandwidth bound.  When
 * n_partials > 0 the log-sum-exp merge with already-computed partial results (the prefix
 * passes) is done in the epilogue and `out` is the final attention output.
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_partial {
    const void* out;  /* [count][B, nq, Hq, D]; dtype, or fp32 when is_f32                      */
    const float* lse; /* [count][B, nq, Hq]                                                     */
    int32_t count;    /* number of stacked partials behind these pointers (split-KV slices)    */
    int32_t is_f32;
} hyd_partial;

typedef struct hyd_suffix_params {
    const void* q;              /* [B, nq, Hq, D]                                              */
    const void* k;              /* sequence b, token t, head h at k + b*k_batch_stride +       */
    const void* v;              /*   t*k_tok_stride + h*k_head_stride (elements)               */
    void* out;                  /* [B, nq, Hq, D] in dtype                                     */
    float* lse;                 /* [B, nq, Hq] or NULL; LSE of the suffix pass alone           */
    const int32_t* seq_lens_i32; /* [B] or NULL                                                */
    const int64_t* seq_lens_i64; /* [B] or NULL (the reference's callers hold int64:           */
                                 /*   llama.py:569); both NULL = every sequence uses kv_len    */
    const int32_t* seq_order;    /* [B] or NULL: a PERMUTATION of 0..B-1, the order in which   */
                                 /*   the sequences are handed to the chip (longest first keeps */
                                 /*   the last workgroups short when lengths are ragged: C2     */
                                 /*   heads, lengths 1..128 at random: 184 -> 169 us).  Only   */
                                 /*   the schedule depends on it, never a result; the caller    */
                                 /*   vouches that it is a permutation.  During decode every    */
                                 /*   length grows by one per step, so one argsort at the start */
                                 /*   of a generation serves all of its steps.                  */
    int64_t k_batch_stride, k_tok_stride, k_head_stride;
    int64_t v_batch_stride, v_tok_stride, v_head_stride;
    int32_t dtype;
    int32_t B, nq, Hq, Hkv, D;
    int32_t kv_len;             /* allocated keys per sequence (Mk); lengths are clamped to it */
    int32_t n_partials;         /* entries used in partials[]                                  */
    float softmax_scale;        /* 0 = D^-0.5 (kv_dim^-0.5 with narrow rows); > 0: that scale           */
                                /*   (hyd_decode_attn_fused applies either to every level as well)      */
    int32_t kv_dim;             /* (was reserved_, 0) 0 or D: k / v rows hold D elements per head.      */
                                /*   16 <= kv_dim < D, kv_dim % 16 == 0: NARROW unique caches -- rows   */
                                /*   of kv_dim elements at the strides given, read as they are (no      */
                                /*   padded copy); q, partials, levels, out and the workspace keep D,   */
                                /*   with ZERO pad columns in q, the levels and the partials (the       */
                                /*   caller vouches); out's pad columns are written as exact zeros.     */
                                /*   16-bit caches and the shapes of hyd_narrow_kv_supported only.      */
    hyd_partial partials[HYD_MAX_LEVELS];
} hyd_suffix_params;

HYD_API int hyd_suffix_attn_fwd(const hyd_suffix_params* p, void* stream);
/* The suffix pass of a MULTI-TOKEN decode step (speculative decoding: hydragen_amd/speculative.py), causal tail: the nq = T query
 * tokens of sequence b (2 <= T <= 8) are its last T tokens and their K/V are already in the cache, so query token i attends the
 * keys below clamp(seq_len[b], 0, kv_len) - (T - 1 - i), clamped at 0 -- bottom-right aligned, what a causal attention over the
 * whole sequence gives its last T rows.  The struct and everything else (partials, lse, seq_order) are hyd_suffix_attn_fwd's; the
 * unique K/V is streamed once for all T tokens.  A row whose limit is 0 (seq_len < T) comes out as zeros with lse = -inf, like a
 * sequence of length 0.  Rows of D elements only: kv_dim (narrow rows) returns HYD_ERR_UNSUPPORTED; fp8 caches go through
 * hyd_suffix_attn_causal_fwd_kvq with HYD_KVQ_CAUSAL.  T outside 2..8 is HYD_ERR_BAD_ARG.  A causal call never runs on a kernel without the limit. */
HYD_API int hyd_suffix_attn_causal_fwd(const hyd_suffix_params* p, void* stream);
/* Shapes only (capture-safe, no device read): 1 exactly when the suffix pass and the whole decode operator take the call with
 * its kv_dim -- always for kv_dim 0 / D; for narrow rows: one query row (nq == 1), Hq == Hkv, Hkv a multiple of the 64 / (D / 8)
 * heads one wave instruction covers, a sequence's cache within 2 GiB (the token-row kernel; the other suffix kernels have no
 * narrow form) --, else 0: such calls return HYD_ERR_UNSUPPORTED, and so does kv_dim with fp8 caches (the _kvq entry points).
 * For finite caches out and lse are bit-identical to the D-wide call on zero-padded k / v with the same softmax scale.  A call
 * with narrow rows ignores single_launch_small: the prefix + suffix pair runs. */
HYD_API int hyd_narrow_kv_supported(const hyd_suffix_params* p);

/* ------------------------------------------------------------------------------------------
 * combine_lse for N partials (attention.py:21-43): out = sum_i out_i*exp(lse_i-m) / sum_i exp(lse_i-m).
 * rows = B*nq*Hq.  `outs`/`lses` are HOST arrays of n device pointers.  dtype may be HYD_F32.
 * out_lse (may be NULL) receives the merged LSE  m + log(sum_i exp(lse_i - m)).
 * ------------------------------------------------------------------------------------------ */
HYD_API int hyd_combine_lse(const void* const* outs, const float* const* lses, int32_t n, int64_t rows, int32_t D,
                    int32_t dtype, void* out, float* out_lse, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole decode-step operator: hydragen_attention with seq_lens given (attention.py:177-354):
 * one prefix pass per shared level into the workspace, then the suffix pass with the merge
 * fused into its epilogue.  With kv_len == 0 and one level the prefix result is written to
 * `out` directly (attention.py:273-274).
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_level {
    const void* k;
    const void* v;
    const int32_t* cu_seqlens_k; /* NULL for uniform levels                                   */
    int64_t k_group_stride, k_tok_stride, k_head_stride;
    int64_t v_group_stride, v_tok_stride, v_head_stride;
    int32_t sb;                  /* shared sequences in this level                            */
    int32_t kv_len;              /* uniform length, or max length when cu_seqlens_k != NULL   */
} hyd_level;

/* Which part of the operator a call enqueues.  ALL is the normal one-call form.  SHARED runs only the
 * per-level prefix passes (they read q and the shared caches and fill the workspace); UNIQUE runs only
 * the suffix pass + merge and expects the workspace as a SHARED call with the same parameters left it.
 * The two halves touch disjoint inputs (the unique K/V and seq_lens are read by UNIQUE only), so a
 * caller may run SHARED on one stream while this step's k/v are still being appended on another.
 *
 * Two-stream form (the reference issues the two passes one after the other, attention.py:250-352; they do not
 * depend on each other, the prefix pass is matrix-core bound and the suffix pass HBM bound):
 *   stream A: SHARED            (with shared_max_workgroups > 0 the prefix pass keeps to that many CUs)
 *   stream B: UNIQUE_PARTIAL    suffix pass alone; its normalised partial + LSE go to the workspace
 *   join, then MERGE            log-sum-exp combine of every partial into `out` (attention.py:21-43)
 * with the same parameters (and workspace) in all three calls.  The caller owns the streams and the
 * fork / join (events, or the edges of a captured graph); hyd_decode_two_stream_ok() says whether the
 * shapes have both parts.  Results equal the one-call form up to one extra rounding of the unique partial
 * to the 16-bit dtype. */
enum { HYD_PHASE_ALL = 0, HYD_PHASE_SHARED = 1, HYD_PHASE_UNIQUE = 2, HYD_PHASE_UNIQUE_PARTIAL = 3, HYD_PHASE_MERGE = 4 };

typedef struct hyd_decode_params {
    hyd_suffix_params suffix;    /* q, unique k/v, seq_lens, out; n_partials/partials ignored */
    hyd_level levels[HYD_MAX_LEVELS];
    int32_t n_levels;
    int32_t phase;               /* HYD_PHASE_*                                               */
    void* workspace;             /* >= hyd_decode_workspace_bytes()                           */
    size_t workspace_bytes;
    int32_t shared_max_workgroups; /* 0 = one workgroup per unit of a prefix pass (the whole chip); > 0: at most
                                    * that many persistent workgroups, one per CU, walk the units           */
    int32_t f32_partials;          /* 0: an unsplit level's partial is stored in the 16-bit dtype (what the reference
                                    * does: its flash-attn output is 16-bit, README.md:488-490); 1: kept fp32 (one
                                    * rounding less, + 2 bytes per output element written and read back)           */
    int32_t single_launch_small;   /* 1 (HYD_PHASE_ALL only): a problem so small that it is launch latency, not work --
                                    * one uniform shared level with few query rows per (group, kv head), short prefix,
                                    * few keys in all -- runs as ONE kernel that walks the group's shared keys and then
                                    * the sequence's own (what the no-sharing baseline does, without the replicated
                                    * prefix).  The result then differs from the phase-split forms by their roundings of
                                    * the partial.  Not taken when suffix.lse is set (that is the LSE of the unique
                                    * keys alone in every form).  0: always the prefix pass + suffix pass pair.       */
    int32_t causal_tail;           /* (was reserved, 0) 0: the operator as it always was.  1: a multi-token decode step -- the
                                    * unique part of HYD_PHASE_ALL / UNIQUE / UNIQUE_PARTIAL follows hyd_suffix_attn_causal_fwd's
                                    * rule (suffix.nq = T in 2..8; every query sees every shared key, as before); the one-launch
                                    * form is not taken.  Refused with HYD_ERR_UNSUPPORTED for narrow rows (suffix.kv_dim) and by
                                    * hyd_decode_attn_fused_kvq for fp8 caches without HYD_KVQ_CAUSAL in hyd_kv_quant.flags. */
} hyd_decode_params;

HYD_API size_t hyd_decode_workspace_bytes(const hyd_decode_params* p);
HYD_API int hyd_decode_attn_fused(const hyd_decode_params* p, void* stream);
/* 1 when the shapes have both a shared and a unique part (the two-stream phases apply), else 0. */
HYD_API int hyd_decode_two_stream_ok(const hyd_decode_params* p);

/* Upper bound helper mirroring SURVEY 8b's `hyd_workspace_bytes(shape...)`: bytes that
 * hyd_decode_attn_fused needs for n_levels uniform levels of the given shapes, in ANY form of the
 * call (every phase, f32_partials set or not: unsplit levels are sized with fp32 partials). */
HYD_API size_t hyd_workspace_bytes(int32_t B, int32_t nq, int32_t Hq, int32_t Hkv, int32_t D, int32_t n_levels,
                           const int32_t* level_sb, const int32_t* level_kv_len);

/* ------------------------------------------------------------------------------------------
 * Decode-step preamble of the attention block: RoPE of this step's q and k at
 * absolute positions (llama.py:485-501), append of k/v into the unique caches at index
 * position - shared_len (llama.py:236-262, 487-492) and seq_lens = index + 1 (llama.py:569),
 * in one kernel.  q/k/v are [B, 1, H, D] with heads contiguous; cos/sin are fp32 [max_pos, D]
 * tables in the rotate-half convention (first D/2 columns are read).
 * Contract: a position below the row's shared length (cache index < 0) writes no K/V for that row, and position
 * shared_len - 1 (-1 without shared_len) reports seq_lens[b] = 0 -- the row takes no part in the suffix pass of the step;
 * callers may rely on it (hyd_stop_update retires the finished rows of a generation this way).
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_rope_params {
    const void* q;               /* [B, 1, Hq, D], batch stride q_batch_stride                   */
    const void* k;               /* [B, 1, Hkv, D]                                               */
    const void* v;               /* [B, 1, Hkv, D]                                               */
    void* q_out;                 /* [B, 1, Hq, D] contiguous: rotated queries                    */
    void* k_cache;               /* [maxB, cache_len, Hkv, D] with the strides below            */
    void* v_cache;
    const float* cos;            /* [max_pos, D] fp32, row stride cs_stride                      */
    const float* sin;
    const int64_t* position_ids; /* [B] absolute positions, element stride pos_stride            */
    const int64_t* shared_len;   /* [B] or NULL (= 0)                                            */
    int32_t* seq_lens;           /* out [B]                                                      */
    int64_t q_batch_stride, k_batch_stride, v_batch_stride;
    int64_t kc_batch_stride, kc_tok_stride, kc_head_stride;
    int64_t vc_batch_stride, vc_tok_stride, vc_head_stride;
    int64_t pos_stride, cs_stride;
    int32_t dtype, B, Hq, Hkv, D, cache_len;
    int32_t max_pos;             /* rows of the cos/sin tables; positions are clamped to it (the  */
                                 /*   host checks the range before launching: a kernel cannot raise) */
    int32_t head_dim;            /* (was reserved, 0) 0 or D: as above.  16 <= head_dim < D, % 16 == 0: q / k / v are rows of
                                  * head_dim elements (head stride head_dim), cos / sin [max_pos, head_dim] (the first head_dim / 2
                                  * columns are read, pairs (i, i + head_dim / 2)), K / V go into the caches as rows of head_dim
                                  * elements at the cache strides, and q_out stays [B, 1, Hq, D] with exact zeros in its pad
                                  * columns.  16-bit caches only. */
} hyd_rope_params;

HYD_API int hyd_rope_append_decode(const hyd_rope_params* p, void* stream);

/* The same preamble for a MULTI-TOKEN decode step: q / k / v are [B, T, H, D] (2 <= T <= 8; heads contiguous, batch and token
 * strides given), position_ids[b] is the absolute position of the row's FIRST token and token i uses position + i.  K (rotated)
 * and V of token i go to cache index idx + i with idx = position - shared_len, q_out is [B, T, Hq, D] contiguous, and
 * seq_lens[b] = idx + T: the T new keys are part of the sequence (hyd_suffix_attn_causal_fwd reads them back).
 * Contract, as above: a cache index < 0 or >= cache_len writes nothing.  A row fed position shared_len - 1 (idx = -1, a retired
 * row) takes no part: NONE of its T tokens is written and seq_lens[b] = 0 -- seq_lens[b] is idx + T only when idx >= 0, else 0.
 * K/V rows of drafts a step rejects stay in the cache behind the row's next length; they are never read, and the next step,
 * which starts behind the last accepted token and writes T rows again, overwrites them.
 * D 64 / 128 / 256 (no narrow head dims); fp8 caches: hyd_rope_append_multi_kvq. */
typedef struct hyd_rope_multi_params {
    const void* q;               /* token i of row b at q + b*q_batch_stride + i*q_tok_stride, [Hq, D] contiguous   */
    const void* k;               /* [B, T, Hkv, D] likewise                                                         */
    const void* v;
    void* q_out;                 /* [B, T, Hq, D] contiguous                                                        */
    void* k_cache;               /* [maxB, cache_len, Hkv, D] with the strides below                                */
    void* v_cache;
    const float* cos;            /* [max_pos, D] fp32, row stride cs_stride                                         */
    const float* sin;
    const int64_t* position_ids; /* [B] position of the first token, element stride pos_stride                      */
    const int64_t* shared_len;   /* [B] or NULL (= 0)                                                               */
    int32_t* seq_lens;           /* out [B]                                                                         */
    int64_t q_batch_stride, k_batch_stride, v_batch_stride;
    int64_t q_tok_stride, k_tok_stride, v_tok_stride;
    int64_t kc_batch_stride, kc_tok_stride, kc_head_stride;
    int64_t vc_batch_stride, vc_tok_stride, vc_head_stride;
    int64_t pos_stride, cs_stride;
    int32_t dtype, B, T, Hq, Hkv, D, cache_len;
    int32_t max_pos;             /* rows of the cos/sin tables; positions are clamped to it                         */
} hyd_rope_multi_params;

HYD_API int hyd_rope_append_multi(const hyd_rope_multi_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise glue of the decoder layer around the attention block (the model shell); rows are
 * tokens, n the hidden / intermediate size, every row 16-byte aligned (n and the row strides multiples of 8).
 *
 * hyd_add_rmsnorm: sum_out = residual + x rounded to dtype (the residual stream of llama.py:615-631: `hidden_states =
 * residual + hidden_states`), norm_out = sum_out * rsqrt(mean(sum_out^2) + eps) * weight with fp32 statistics and one
 * rounding (transformers' LlamaRMSNorm, constructed at llama.py:605-608,656) in one pass.  residual == NULL: plain
 * RMSNorm of x (sum_out ignored).  sum_out may alias residual or x.  n <= 16384.
 *
 * hyd_swiglu: out = silu(gate) * up (transformers' LlamaMLP, llama.py:2,604: down_proj(act_fn(gate_proj(x)) *
 * up_proj(x))), fp32 maths, one rounding; gate / up may be the column halves of one fused GEMM output.
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_add_rmsnorm_params {
    const void* x;         /* [rows, n] block output (o_proj / down_proj), row stride x_row_stride        */
    const void* residual;  /* [rows, n] or NULL                                                          */
    const void* weight;    /* [n], dtype                                                                 */
    void* sum_out;         /* [rows, n] or NULL                                                          */
    void* norm_out;        /* [rows, n]                                                                  */
    int64_t x_row_stride, residual_row_stride, sum_row_stride, norm_row_stride; /* elements              */
    int64_t rows;
    int32_t n;
    int32_t dtype;         /* HYD_F16 | HYD_BF16                                                         */
    float eps;
    int32_t reserved;
} hyd_add_rmsnorm_params;

HYD_API int hyd_add_rmsnorm(const hyd_add_rmsnorm_params* p, void* stream);

typedef struct hyd_swiglu_params {
    const void* gate;      /* [rows, n], row stride gate_row_stride                                       */
    const void* up;        /* [rows, n]                                                                  */
    void* out;             /* [rows, n]                                                                  */
    int64_t gate_row_stride, up_row_stride, out_row_stride; /* elements                                  */
    int64_t rows;
    int32_t n;
    int32_t dtype;
} hyd_swiglu_params;

HYD_API int hyd_swiglu(const hyd_swiglu_params* p, void* stream);

/* Next token of every sequence from its last-position logits: out[row] ~ softmax(logits[row] / temperature), what
 * `sample_from_logits` (llama.py: softmax(logits / temperature) + torch.multinomial(num_samples=1)) draws, by the
 * Gumbel-max identity argmax_v(logits_v / temperature + g_v) in one pass over the logits; temperature == 0: plain
 * argmax (lowest index on ties), as the reference's temperature-0 branch.  The noise is Philox4x32-10 keyed by
 * (seed, offset, row, column): the same (seed, offset) gives the same tokens on any device / launch geometry; the
 * caller advances `offset` by one per call.  logits: [rows, n] HYD_F16 | HYD_BF16 | HYD_F32, row stride in elements. */
typedef struct hyd_sample_params {
    const void* logits;
    int64_t* out;          /* [rows]                                                                     */
    int64_t row_stride;
    uint64_t seed, offset;
    int32_t rows, n;
    int32_t dtype;
    float temperature;     /* >= 0                                                                       */
} hyd_sample_params;

HYD_API int hyd_sample_tokens(const hyd_sample_params* p, void* stream);

/* hyd_sample_tokens with the usual sampling cuts, and the sampled token's log-probability.  For one row l (length n), with
 * m = max(l) and p = softmax(l):
 *   - the cuts act on the UNSCALED distribution softmax(l), not on softmax(l / temperature) (the reference's apply_top_p;
 *     HF applies the temperature first, so results differ from HF when temperature != 1);
 *   - top_k > 0 keeps every token whose logit is >= the k-th largest logit (ties kept; k >= n: no cut);
 *   - top_p < 1 then keeps, among the top-k survivors renormalised, the tokens with l >= t*, t* the largest logit value whose
 *     top set {l >= t*} holds >= top_p of their mass: the token that crosses top_p and every token tied with it are kept;
 *   - min_p > 0 keeps p_i >= min_p * p_max, i.e. l_i - m >= ln(min_p) (the max always survives);
 *   - -inf and NaN logits are never kept; a row without a finite logit gives token 0, kept 0 and a NaN log-prob;
 *   - the draw is argmax(l / temperature + g) over the kept tokens with hyd_sample_tokens' noise g for the same
 *     (seed, offset, row, column), bit for bit: with no cut set the tokens are hyd_sample_tokens' tokens; temperature 0 is
 *     the argmax (lowest index on ties);
 *   - logprobs[row] = l_tok - m - ln sum_j exp(l_j - m) (fp32): the log-probability under the unscaled, unfiltered
 *     distribution, independent of temperature and cuts;
 *   - masses are summed as fixed-point integers: tokens, kept counts and log-probs do not depend on the run or the launch.
 * Rows longer than HYD_SAMPLE_FILTER_MAX_N give HYD_ERR_UNSUPPORTED; top_k < 0, top_p outside (0, 1] and min_p outside
 * [0, 1] (NaN included) give HYD_ERR_BAD_ARG. */
#define HYD_SAMPLE_FILTER_MAX_N (1 << 22)
typedef struct hyd_sample_filter_params {
    const void* logits;    /* [rows, n] HYD_F16 | HYD_BF16 | HYD_F32, row stride in elements        */
    int64_t* out;          /* [rows] sampled token                                                  */
    float* logprobs;       /* [rows] or NULL: log softmax(logits)[out] (unscaled, unfiltered)       */
    int32_t* kept;         /* [rows] or NULL: number of tokens that survived the filters            */
    int64_t row_stride;
    uint64_t seed, offset; /* as hyd_sample_params                                                  */
    int32_t rows, n, dtype;
    float temperature;     /* >= 0                                                                  */
    int32_t top_k;         /* 0 = off                                                               */
    float top_p;           /* (0, 1]; 1 = off                                                       */
    float min_p;           /* [0, 1]; 0 = off                                                       */
} hyd_sample_filter_params;

HYD_API int hyd_sample_tokens_filtered(const hyd_sample_filter_params* p, void* stream);

/* hyd_sample_tokens_filtered on PENALISED logits: repetition / presence / frequency penalties and a sparse logit bias, in the
 * same single launch (one workgroup per row, no [rows, n] side tensor).  For one row l (length n), with
 *   ctx  = the tokens of the row's context: the union of the row's bitmap rows, row b reading row b / rows_per_group of every
 *          context bitmap (a prompt shared by a group of rows is one bitmap row of ceil(n / 32) words, bit v of the row = bit
 *          v % 32 of word v / 32);
 *   c[v] = how often v occurs among gen[row, 0 .. min(gen_len[row], gen_stride)) (entries outside [0, n) are ignored),
 * the penalised logit x[v] is, in this order:
 *   1. v in ctx or c[v] > 0:  x = l > 0 ? l / repetition_penalty : l * repetition_penalty (the HF / vLLM rule); else x = l;
 *   2. x -= frequency_penalty * c[v] + presence_penalty * (c[v] > 0)   (the OpenAI / vLLM rule: generated tokens only);
 *   3. v == bias_ids[k]:  x += bias_values[k]   (-inf bans the token; ids distinct, ids outside [0, n) are ignored).
 *      The entry point cannot check that the ids are distinct: an id given twice gets the value at the bitwise OR of its
 *      two (1-based) list positions if that is a position of the list, else no bias -- never a read outside the list.
 * A token that no rule touches keeps its logit exactly; a touched one is evaluated in double from the fp32 / 16-bit logit
 * and rounded ONCE to fp32.  Everything hyd_sample_tokens_filtered does then acts on x instead of l, unchanged: the cuts on
 * the unscaled softmax(x), the draw argmax(x / temperature + g) with hyd_sample_tokens' noise for the same (seed, offset, row,
 * column), temperature 0 = lowest-index argmax of x, -inf and NaN never kept (a row whose every x is one: token 0, kept 0,
 * NaN log-prob), and logprobs[row] = log softmax(x)[token]: the PENALISED, unscaled, unfiltered distribution.  With every
 * penalty neutral (1, 0, 0, no bitmap, no generated token, no bias) tokens, kept counts and log-probs are
 * hyd_sample_tokens_filtered's bit for bit.  Fixed-point masses as there: a row's outputs do not depend on the run, the launch
 * geometry or the other rows.  gen_len is read on the device at launch time.  append_out != 0: after the draw the kernel
 * stores the token at gen[row, gen_len[row]] (if that is < gen_stride) and adds one to gen_len[row], so that a decode loop
 * that feeds back what it samples needs no other launch to keep the list.
 * Side memory is the bitmaps and gen; the kernel has no workspace.
 * HYD_ERR_BAD_ARG: what hyd_sample_tokens_filtered refuses, repetition_penalty <= 0 or NaN or inf, a non-finite
 * frequency_penalty / presence_penalty, n_context outside [0, HYD_SAMPLE_MAX_CONTEXT], a null context bitmap or rows_per_group
 * <= 0, gen_len without gen (or gen without gen_len), gen_stride < 0, append_out without gen, n_bias outside
 * [0, HYD_SAMPLE_BIAS_MAX] or n_bias > 0 without ids / values, misaligned pointers.  HYD_ERR_UNSUPPORTED: a bad dtype,
 * n > HYD_SAMPLE_FILTER_MAX_N, gen_stride > HYD_SAMPLE_GEN_MAX. */
#define HYD_SAMPLE_MAX_CONTEXT (HYD_MAX_LEVELS + 1) /* every shared level and the rows' own prompts */
#define HYD_SAMPLE_BIAS_MAX 1024                    /* entries of the logit-bias list               */
#define HYD_SAMPLE_GEN_MAX 2048                     /* generated tokens per row the kernel counts   */
typedef struct hyd_token_bitmap {
    const uint32_t* bits;   /* [groups, ceil(n / 32)]                                                */
    int32_t rows_per_group; /* row b reads bitmap row b / rows_per_group                             */
    int32_t reserved;
} hyd_token_bitmap;

typedef struct hyd_sample_penalty_params {
    const void* logits;    /* [rows, n] HYD_F16 | HYD_BF16 | HYD_F32, row stride in elements        */
    int64_t* out;          /* [rows] sampled token                                                  */
    float* logprobs;       /* [rows] or NULL: log softmax(x)[out] (penalised, unscaled, unfiltered) */
    int32_t* kept;         /* [rows] or NULL: number of tokens that survived the filters            */
    int64_t row_stride;
    uint64_t seed, offset; /* as hyd_sample_params                                                  */
    int32_t rows, n, dtype;
    float temperature;     /* >= 0                                                                  */
    int32_t top_k;         /* 0 = off                                                               */
    float top_p;           /* (0, 1]; 1 = off                                                       */
    float min_p;           /* [0, 1]; 0 = off                                                       */
    int32_t n_context;     /* context bitmaps in use                                                */
    double repetition_penalty; /* > 0; 1 = off                                                      */
    double frequency_penalty;  /* finite; 0 = off                                                   */
    double presence_penalty;   /* finite; 0 = off                                                   */
    hyd_token_bitmap context[HYD_MAX_LEVELS + 1];
    int32_t* gen;          /* [rows, gen_stride] generated tokens, or NULL (written only by append_out) */
    int32_t* gen_len;      /* [rows] device; NULL iff gen is NULL                                   */
    int32_t gen_stride;    /* <= HYD_SAMPLE_GEN_MAX                                                 */
    int32_t append_out;    /* != 0: append the drawn token to gen / gen_len                         */
    const int64_t* bias_ids;  /* [n_bias] distinct                                                  */
    const float* bias_values; /* [n_bias] finite or -inf                                            */
    int32_t n_bias;        /* <= HYD_SAMPLE_BIAS_MAX                                                */
    int32_t reserved;
} hyd_sample_penalty_params;

HYD_API int hyd_sample_tokens_penalized(const hyd_sample_penalty_params* p, void* stream);

/* Presence bitmap of token ids: bits[g, v / 32] |= 1 << (v % 32) for every v = ids[g, j], j < lens[g] (lens NULL: j < L), 0 <= v
 * < n.  The kernel ORs into `bits` (atomic OR): the caller zeroes it first, or accumulates several id tensors into one bitmap.
 * One launch, nothing else is allocated.  Null ids / bits, groups < 0, L < 0, n <= 0 or n > HYD_SAMPLE_FILTER_MAX_N, id_stride
 * < L and misaligned pointers give HYD_ERR_BAD_ARG. */
typedef struct hyd_token_bitmap_params {
    const int64_t* ids;    /* [groups, L], row stride id_stride (elements)                          */
    const int64_t* lens;   /* [groups] or NULL                                                      */
    uint32_t* bits;        /* [groups, ceil(n / 32)]                                                */
    int64_t id_stride;
    int32_t groups, L, n, reserved;
} hyd_token_bitmap_params;

HYD_API int hyd_token_bitmap_build(const hyd_token_bitmap_params* p, void* stream);

/* hyd_sample_tokens_penalized under a token automaton: what a row may emit depends on what it has emitted so far, decided inside
 * the same single launch.  A token automaton over n tokens with n_states states is one table next [n_states, n] of int32:
 *   next[s, v] >= 0               token v is allowed in state s and leads to that state (< n_states);
 *   next[s, v] == HYD_DFA_REJECT  v is not allowed in s;
 *   next[s, v] == HYD_DFA_FREE    v is allowed, and the row is unconstrained from then on;
 * and the bitmap allowed [n_states, ceil(n / 32)] derived from it: bit v % 32 of word v / 32 of row s is set iff next[s, v] !=
 * HYD_DFA_REJECT (hyd_token_bitmap's bit layout; one row per STATE, shared by every batch row in that state -- nothing of size
 * [rows, n] exists).  state[row] is read on the device at launch time.  A row whose state lies outside [0, n_states) is
 * unconstrained: its logits are taken as they are and its state does not change.  For a constrained row every rule of
 * hyd_sample_tokens_penalized (penalties, bias, cuts, draw, log-prob, kept) acts on the row with the logits of the tokens whose
 * bit is clear replaced by -inf; bits at positions >= n are ignored.  -inf is absorbing under every penalty rule and never kept,
 * so tokens, kept counts and log-probs are, bit for bit, those of hyd_sample_tokens_penalized (with every penalty neutral: of
 * hyd_sample_tokens_filtered) on logits filled with -inf at the tokens that are not allowed, for the same (seed, offset).
 * advance != 0: after the draw state[row] = next[state[row], token].  A row without any valid logit gives token 0, kept 0 and a
 * NaN log-prob, as there, and keeps its state.  The kernel reads `allowed` for the mask and `next` for the one entry of the
 * drawn token: a pair that does not agree is the caller's responsibility -- a token drawn into a HYD_DFA_REJECT entry leaves
 * the row unconstrained (state -1), like HYD_DFA_FREE, and so does any entry outside [0, n_states).  No indexing ever uses a
 * state outside [0, n_states).
 * c == NULL is exactly hyd_sample_tokens_penalized(p).  The call is capture-safe: no allocation, no synchronisation, no
 * workspace, no environment variable; state is the only memory written besides what hyd_sample_tokens_penalized writes.
 * HYD_ERR_BAD_ARG: everything hyd_sample_tokens_penalized refuses (HYD_ERR_UNSUPPORTED where it says so), a null allowed /
 * next / state, n_states <= 0, allowed_stride < ceil(n / 32), next_stride < n, pointers not aligned to 4 bytes. */
#define HYD_DFA_REJECT (-1)
#define HYD_DFA_FREE (-2)
typedef struct hyd_token_dfa {
    const uint32_t* allowed;   /* [n_states, allowed_stride] words                                      */
    const int32_t*  next;      /* [n_states, next_stride]                                               */
    int32_t*        state;     /* [rows] device, read at launch time                                    */
    int64_t allowed_stride;    /* words,    >= ceil(n / 32)                                             */
    int64_t next_stride;       /* elements, >= n                                                        */
    int32_t n_states;
    int32_t advance;           /* != 0: state[row] = next[state[row], token] after the draw             */
} hyd_token_dfa;

HYD_API int hyd_sample_tokens_constrained(const hyd_sample_penalty_params* p, const hyd_token_dfa* c, void* stream);

/* hyd_sample_tokens_constrained with PER-ROW sampling values and seeds: the rows of one launch may each sample with their own
 * temperature, cuts, penalties and noise key (requests of different settings batched behind one shared prompt).  Every array is a
 * device pointer to p->rows entries, or NULL = the scalar in p for every row; with every array NULL the call is exactly
 * hyd_sample_tokens_constrained(p, c) (c == NULL: hyd_sample_tokens_penalized(p)).  Row r uses entry r, and each value means what
 * the scalar of the same name in p means: a row's tokens, kept counts, log-probs, appended tokens and advanced states are, bit
 * for bit, what a scalar launch with that row's values gives that row.  The penalties arrive as fp32 and are widened to double
 * exactly: a per-row value f behaves like the scalar (double)f.
 * The arrays are read on the device at launch time, once per row, and the host cannot check them, so the kernel replaces what
 * the scalar entry points refuse, and no value ever forms an address:
 *   temperature          NaN or < 0 -> 0 (argmax);  the noise scale is temperature > 0 ? 1.0f / temperature : 0 (fp32)
 *   top_k                < 0 -> 0 (off);  >= n: no cut
 *   top_p                outside (0, 1] or NaN -> 1 (off)
 *   min_p                outside [0, 1] or NaN -> 0 (off);  the threshold is min_p > 0 ? (float)log((double)min_p) : -inf
 *   repetition_penalty   <= 0, NaN or inf -> 1 (off);  positive logits are multiplied by 1.0 / (double)repetition_penalty
 *   frequency_penalty, presence_penalty   NaN or +-inf -> 0 (off)
 * -- the expressions the host evaluates for the scalars of the other entry points.
 * seed != NULL: row r draws with the noise hyd_sample_tokens_filtered gives ROW 0 of a launch with seed = seed[r] and the same
 * p->offset -- Philox counter (chunk, 0, offset lo, offset hi), key seed[r]; p->seed is not used.  A row's draw is then a function
 * of its own logits, values, seed and offset: neither its position in the batch nor the other rows play a part.
 * One launch, one workgroup per row; no workspace, no allocation, no synchronisation: capture-safe like the call it extends.  A call
 * in which no penalty can act (neutral scalars in p, no penalty array, no bias, append_out == 0) costs what
 * hyd_sample_tokens_filtered costs; any other pays hyd_sample_tokens_penalized's prologue.
 * HYD_ERR_BAD_ARG / HYD_ERR_UNSUPPORTED: everything hyd_sample_tokens_constrained refuses (the scalars in p are checked even where
 * an array overrides them), and an array pointer that is not aligned to its element size (4 bytes; seed: 8).  rows == 0 succeeds
 * without a launch. */
HYD_API int hyd_sample_tokens_rows(const hyd_sample_penalty_params* p, const hyd_token_dfa* c, const float* temperature,
                                   const int32_t* top_k, const float* top_p, const float* min_p, const float* repetition_penalty,
                                   const float* frequency_penalty, const float* presence_penalty, const uint64_t* seed, void* stream);

/* Log-probabilities of GIVEN tokens (scoring, teacher forcing) and the top-N alternatives of every row.  For one row l (length n)
 * and its target token t, with the valid logits those that are neither NaN nor -inf and m = their max:
 *   - logprobs[row] = l_t - m - ln sum_j exp(l_j - m) over the valid logits (fp32), with hyd_sample_tokens_filtered's fixed-point
 *     masses and closing expression: for any row and token, the same bits as that entry point's log-prob of the token;
 *   - greedy[row] = 1 iff t is the LOWEST-index maximum of the valid logits (torch.argmax's tie rule; what hyd_sample_tokens
 *     picks at temperature 0), else 0;
 *   - top_ids[row, :top_n] / top_logprobs[row, :top_n]: the top_n largest valid logits ordered by (value descending, index
 *     ascending) and their log-probs (same expression); a row with fewer valid logits pads with id -1 and -inf;
 *   - t < 0 or t >= n: logprob NaN, greedy 0, and no load at t (the caller marks padding this way); l_t NaN: NaN; l_t -inf:
 *     -inf; a row without a valid logit: NaN, greedy 0, top-N all padding;
 *   - masses are summed as fixed-point integers: a row's outputs do not depend on the run, the launch geometry or the other
 *     rows of the launch.
 * Null logits / targets / logprobs / greedy, rows outside [0, 2^31], n <= 0, row_stride < n, top_n outside
 * [0, HYD_TOP_LOGPROBS_MAX], top_n > 0 without top_ids and top_logprobs, and misaligned pointers give HYD_ERR_BAD_ARG; a bad
 * dtype and n > HYD_SAMPLE_FILTER_MAX_N give HYD_ERR_UNSUPPORTED. */
#define HYD_TOP_LOGPROBS_MAX 20
typedef struct hyd_token_logprob_params {
    const void* logits;    /* [rows, n] HYD_F16 | HYD_BF16 | HYD_F32, row stride in elements           */
    int32_t dtype, n;
    int64_t rows, row_stride;
    const int64_t* targets; /* [rows] token to score; outside [0, n): padding                          */
    float* logprobs;       /* [rows]                                                                   */
    uint8_t* greedy;       /* [rows] 0 / 1                                                             */
    int32_t top_n, reserved;
    int64_t* top_ids;      /* [rows, top_n] or NULL when top_n == 0                                    */
    float* top_logprobs;   /* [rows, top_n] or NULL when top_n == 0                                    */
} hyd_token_logprob_params;

HYD_API int hyd_token_logprobs(const hyd_token_logprob_params* p, void* stream);

/* Stop conditions of a generation, decided on the device: one launch per decode step, after the sampling launch.  Row b's token
 * of step t (tok[b]; t = 0 is the token drawn from the prefill logits) is judged by these rules, in this order
 * (hydragen_amd/stopping.py states the same definition in torch):
 *   (a) reason[b] != 0 (the row finished at an earlier step): out[b, t] = pad, nothing else changes;
 *   (b) otherwise out[b, t] = tok[b]; tok[b] == eos[i] for the lowest i < n_eos: reason 1, stop_index i, length t + 1 (the EOS
 *       token is kept);
 *   (c) otherwise the stop sequences in list order: sequence k (stop_lens[k] = len tokens, stop_tokens[k, 0 .. len)) matches
 *       when t + 1 >= len and out[b, t + 1 - len .. t] equals it -- never reaching back in front of step 0, and never across
 *       columns a finished row has padded, since only running rows are tested; the lowest matching k gives reason 2,
 *       stop_index k; include_stop == 0: the len matched columns become pad and length = t + 1 - len, else they stay and
 *       length = t + 1;
 *   (d) otherwise the row keeps running: length = t + 1.
 * Then, for the next step: feed[b] = tok[b] for a running row, pad for a finished one; next_pos[b] = start_pos[b] + t for a
 * running row and shared_len[b] - 1 (-1 with shared_len NULL) for a finished one -- the position at which
 * hyd_rope_append_decode writes no K/V and reports length 0, so that the row leaves the suffix pass; retire == 0: start_pos[b]
 * + t for every row.  live[t] += the number of rows still running after the step (the caller zeroes live once per generation).
 * A row's outputs depend on that row alone, not on the launch geometry.  t is a host value: the launch is not meant for a
 * captured graph that is replayed with another t.
 * HYD_ERR_BAD_ARG: a null tok / out / length / reason / stop_index / live / start_pos / feed / next_pos, rows < 0, n_eos outside
 * [0, HYD_STOP_MAX_EOS], n_stop outside [0, HYD_STOP_MAX_SEQS], n_stop > 0 without stop_tokens, a stop length outside
 * [1, HYD_STOP_MAX_LEN], t outside [0, out_stride), misaligned pointers.  rows == 0 succeeds without a launch. */
#define HYD_STOP_MAX_EOS 16
#define HYD_STOP_MAX_SEQS 32
#define HYD_STOP_MAX_LEN 16
typedef struct hyd_stop_params {
    const int64_t* tok;         /* [rows] the tokens just drawn                                              */
    int64_t* out;               /* [rows, out_stride] the generation's output matrix; column t is written     */
    int32_t* length;            /* [rows] kept tokens                                                        */
    int32_t* reason;            /* [rows] 0 = running, 1 = EOS, 2 = stop sequence, 3 = the row's own limit   */
    int32_t* stop_index;        /* [rows] which EOS id / stop sequence matched; the caller starts it at -1   */
    int32_t* live;              /* [out_stride] rows still running after each step; zeroed by the caller     */
    const int64_t* stop_tokens; /* [n_stop, HYD_STOP_MAX_LEN] device, or NULL when n_stop == 0               */
    const int64_t* start_pos;   /* [rows] absolute position at which a row's token of step 0 is fed          */
    const int64_t* shared_len;  /* [rows] or NULL (= 0)                                                      */
    int64_t* feed;              /* [rows] out: the token to feed next                                        */
    int64_t* next_pos;          /* [rows] out: the position to feed it at                                    */
    int64_t out_stride;         /* elements                                                                  */
    int64_t pad;
    int64_t eos[HYD_STOP_MAX_EOS];         /* HOST values                                                    */
    int32_t stop_lens[HYD_STOP_MAX_SEQS];  /* HOST values, each in [1, HYD_STOP_MAX_LEN]                     */
    int32_t rows, t, n_eos, n_stop;
    int32_t include_stop;       /* != 0: a matched stop sequence stays in out and counts in length           */
    int32_t retire;             /* != 0: finished rows get the position that retires them from the K/V stream */
} hyd_stop_params;

HYD_API int hyd_stop_update(const hyd_stop_params* p, void* stream);

/* hyd_stop_update with a token limit PER ROW.  max_len: a device pointer to p->rows int32 entries, or NULL = exactly
 * hyd_stop_update(p).  With max_len, after rules (a) to (c) and before (d):
 *   (c') a row still running at step t with t + 1 >= max_len[b] finishes: reason 3 (the row's own limit), length t + 1, stop_index
 *        stays -1.
 * Rules (a) to (c) win when they apply at the same step (an EOS exactly at the limit gives reason 1; a stop sequence that would
 * complete a step after the limit is never matched).  A row finished this way is padded, fed pad and retired from the unique K/V
 * stream exactly like a row finished by EOS.  An entry <= 0 finishes the row at step 0 with length 1.  max_len is read on the
 * device; entries are only compared.  Refusals as hyd_stop_update, and a max_len that is not 4-byte aligned: HYD_ERR_BAD_ARG. */
HYD_API int hyd_stop_update_rows(const hyd_stop_params* p, const int32_t* max_len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Speculative decoding (hydragen_amd/speculative.py states both definitions in torch): drafts by prompt lookup, and the
 * acceptance of a verified step.  Neither launch synchronises with the host.
 *
 * hyd_draft_lookup: row b's LOGICAL sequence is the concatenation of n_segments segments -- the shared levels given to this
 * generation on the row's path, its own prompt, its generated tokens.  Segment s contributes the first len tokens of row
 * b / div of ids (lens_i64[b / div], else lens_i32[b / div], clamped to [0, len], the columns of a row; without either, len):
 * there is no per-row copy of shared tokens.  With L the total length: for n = ngram_max down to ngram_min, the last n tokens of the
 * sequence are looked for among its earlier positions; an occurrence must END strictly before the last position (the trivial
 * match is excluded) and the LATEST one wins; the first n with an occurrence wins.  With e the end position of the winner,
 * drafts[b, j] = token e + 1 + j for j < n_proposed[b] = min(K, L - 1 - e), the other slots hold 0 (any token is a valid draft:
 * it is only verified); no occurrence, or L < 2: n_proposed[b] = 0.  Matches and proposals may cross segment boundaries.
 * One wave per row: lanes scan candidate end positions, a wave reduction picks the maximum of (match length, position).
 * HYD_ERR_BAD_ARG: null or misaligned pointers, B < 0, K outside [1, 7], 1 <= ngram_min <= ngram_max <= HYD_DRAFT_MAX_NGRAM
 * violated, n_segments outside [1, HYD_DRAFT_MAX_SEGMENTS], a segment with div < 1 or a null ids with a non-zero length. */
#define HYD_DRAFT_MAX_SEGMENTS (HYD_MAX_LEVELS + 2)
#define HYD_DRAFT_MAX_NGRAM 8
typedef struct hyd_draft_segment {
    const int64_t* ids;      /* [rows of the segment, row_stride]                                          */
    const int64_t* lens_i64; /* [rows of the segment] or NULL                                              */
    const int32_t* lens_i32; /* [rows of the segment] or NULL; both NULL: every row holds `len` tokens     */
    int64_t row_stride;      /* elements                                                                   */
    int32_t len;             /* columns of a row: the uniform length, and the cap of the per-row lengths   */
    int32_t div;             /* row b of the batch reads row b / div of the segment (the fan-out)          */
} hyd_draft_segment;

typedef struct hyd_draft_lookup_params {
    hyd_draft_segment segments[HYD_DRAFT_MAX_SEGMENTS];
    int64_t* drafts;         /* out [B, drafts_stride]: columns 0 .. K - 1 are written                     */
    int32_t* n_proposed;     /* out [B]                                                                    */
    int64_t drafts_stride;   /* elements                                                                   */
    int32_t n_segments, B, K, ngram_min, ngram_max;
    int32_t reserved;
} hyd_draft_lookup_params;

HYD_API int hyd_draft_lookup(const hyd_draft_lookup_params* p, void* stream);

/* hyd_draft_accept: after a step that fed row b the T = K + 1 tokens fed[b, :] (its last emitted token, then K drafts) and drew
 * sampled[b, i] from the logits behind fed[b, i].  A row with reason[b] != 0 or length[b] >= max_new_tokens has finished: nothing
 * of it changes and accepted[b] = 0.  Otherwise, in this order: n = the number of leading i < K with fed[b, i + 1] ==
 * sampled[b, i]; the row emits sampled[b, 0 .. n]; the run is cut behind its first EOS id (kept: reason 1, stop_index = the
 * lowest matching i < n_eos) and at max_new_tokens - length[b] tokens (reason stays 0); the e emitted tokens (and their
 * log-probs, when both logprobs and out_logprobs are given) go to out[b, length[b] ..), length[b] += e and accepted[b] = e - 1,
 * the drafts that became output.  For the next step: a row that still runs is fed its last emitted token at position
 * start_pos[b] + length[b] - 1 (start_pos: the position of the token in column 0); a finished row is fed pad at position
 * shared_len[b] - 1 (-1 with shared_len NULL), which retires it from the K/V stream (hyd_rope_append_multi), or -- retire == 0
 * -- at start_pos[b] + length[b] - 1 like a running one.  *live += the rows still running after the step (the caller zeroes it).
 * The caller fills out with pad and zeroes length / reason before the first call; a generation's first token (drawn from the
 * prefill logits) is entered by a call with T = 1 -- the one case in which K = 0 is accepted.
 * HYD_ERR_BAD_ARG: null or misaligned pointers, rows < 0, T outside [1, 8], n_eos outside [0, HYD_STOP_MAX_EOS],
 * max_new_tokens outside [1, out_stride]. */
typedef struct hyd_draft_accept_params {
    const int64_t* fed;         /* [rows, T]                                                                 */
    const int64_t* sampled;     /* [rows, T]                                                                 */
    const float* logprobs;      /* [rows, T] or NULL                                                         */
    int64_t* out;               /* [rows, out_stride]                                                        */
    float* out_logprobs;        /* [rows, out_stride] or NULL                                                */
    int32_t* length;            /* [rows] tokens emitted so far                                              */
    int32_t* reason;            /* [rows] 0 = running or cut at max_new_tokens, 1 = EOS                      */
    int32_t* stop_index;        /* [rows] which EOS id matched; the caller starts it at -1                   */
    int32_t* accepted;          /* [rows] out: drafts of this step that became output                        */
    int32_t* live;              /* [1] rows still running after the step are ADDED; zeroed by the caller     */
    const int64_t* start_pos;   /* [rows]                                                                    */
    const int64_t* shared_len;  /* [rows] or NULL (= 0)                                                      */
    int64_t* feed;              /* [rows] out: the first token of the next step                              */
    int64_t* next_pos;          /* [rows] out: its position                                                  */
    int64_t out_stride;         /* elements                                                                  */
    int64_t pad;
    int64_t eos[HYD_STOP_MAX_EOS];  /* HOST values                                                           */
    int32_t rows, T, n_eos, max_new_tokens;
    int32_t retire;
    int32_t reserved;
} hyd_draft_accept_params;

HYD_API int hyd_draft_accept(const hyd_draft_accept_params* p, void* stream);

/* Speculative decoding under a token automaton (hyd_token_dfa's tables): drafts a state FORCES are accepted with probability 1,
 * because the masked sampler can draw nothing else.  Three launches around the step, none synchronises with the host.
 *
 * hyd_dfa_forced_tokens, once per automaton: state s is FORCED when exactly one bit at a position below n is set in row s of
 * `allowed`; forced[s] = that token, else -1 (no bit, or two and more).  Bits at positions >= n are ignored and words past
 * ceil(n / 32) of a row are not read.  Only the bitmap is read (one wave per state, 16-byte loads where allowed is 16-byte aligned
 * and allowed_stride a multiple of 4 words); no workspace.
 * HYD_ERR_BAD_ARG: null or misaligned (4 bytes) pointers, n_states <= 0, n <= 0, allowed_stride < ceil(n / 32). */
typedef struct hyd_dfa_forced_params {
    const uint32_t* allowed;   /* [n_states, allowed_stride] words                                           */
    int32_t* forced;           /* out [n_states]                                                             */
    int64_t allowed_stride;    /* words                                                                      */
    int32_t n_states, n;
} hyd_dfa_forced_params;

HYD_API int hyd_dfa_forced_tokens(const hyd_dfa_forced_params* p, void* stream);

/* hyd_draft_constrain: after the drafts of a step are in fed[b, 1 .. K] (fed[b, 0] is the row's last emitted token, whose effect
 * is already in state[b]) and before the forward pass.  Row b, with s = state[b] and step_state[b, 0] = s, for j = 0 .. K - 1:
 *   1. s in [0, n_states) and forced[s] >= 0: fed[b, j + 1] = forced[s], n_forced[b] counts it, n_proposed[b] = max(., j + 1);
 *   2. otherwise, with only_forced != 0, the chain ends: n_proposed[b] = min(., j), the remaining drafts keep what they hold and
 *      step_state[b, j + 1 ..] = -1;
 *   3. s in [0, n_states): with t = fed[b, j + 1], e = next[s, t] (HYD_DFA_REJECT for t outside [0, n)).  e == HYD_DFA_REJECT:
 *      the draft can never be drawn -- n_proposed[b] = min(., j) and step_state[b, j + 1 ..] = -1, their draws are never kept;
 *      e == HYD_DFA_FREE: s = -2; e in [0, n_states): s = e; any other value: s = -1 (as in hyd_sample_tokens_constrained);
 *   4. s outside [0, n_states): the row is unconstrained, s and the draft stay;
 *   5. step_state[b, j + 1] = s.
 * step_state, flattened to [B * T], is the state array of the step's hyd_sample_tokens_constrained call over its B * T logits
 * rows (advance != 0): logits row (b, i) predicts the token behind fed[b, i] and is masked by step_state[b, i].  A draw behind a
 * column at or past an ended chain is unconstrained: the caller must not keep it (a draft rejected in 3. can never equal the
 * draw in front of it; behind 2. the caller compares columns past n_proposed[b] with a value no token equals).
 * state is read only; n_proposed may be NULL (nothing is counted).  One row per lane; no read uses a state outside
 * [0, n_states) or a token outside [0, n).
 * HYD_ERR_BAD_ARG: null or misaligned pointers, B < 0, K outside [1, 7], n_states <= 0, n <= 0, next_stride < n,
 * fed_stride < K + 1.  B == 0 succeeds without a launch. */
typedef struct hyd_draft_constrain_params {
    const int32_t* state;      /* [B]                                                                        */
    int64_t* fed;              /* [B, fed_stride]: columns 1 .. K are read and, where a state is forced, written */
    int32_t* n_proposed;       /* [B] in / out, or NULL                                                      */
    const int32_t* forced;     /* [n_states] hyd_dfa_forced_tokens' output                                   */
    const int32_t* next;       /* [n_states, next_stride]                                                    */
    int32_t* step_state;       /* out [B, K + 1]                                                             */
    int32_t* n_forced;         /* out [B] drafts of this step a forced state wrote                           */
    int64_t fed_stride;        /* elements, >= K + 1                                                         */
    int64_t next_stride;       /* elements, >= n                                                             */
    int32_t B, K, n_states, n;
    int32_t only_forced;       /* != 0: the drafts are the forced chain alone                                */
    int32_t reserved;
} hyd_draft_constrain_params;

HYD_API int hyd_draft_constrain(const hyd_draft_constrain_params* p, void* stream);

/* hyd_draft_accept_states: hyd_draft_accept, bit for bit, and for a row that emits e >= 1 tokens also
 * state[b] = step_state_after[b, e - 1] -- step_state_after [rows, T] is the step's state array AFTER the constrained sampler
 * advanced it, so its entry (b, i) is the state behind sampled[b, i].  A finished row, or one that emits nothing, keeps its
 * state.  With step_state_after and state both NULL the call IS hyd_draft_accept; one of them NULL, or misaligned (4 bytes), is
 * HYD_ERR_BAD_ARG, as is everything hyd_draft_accept refuses. */
HYD_API int hyd_draft_accept_states(const hyd_draft_accept_params* p, const int32_t* step_state_after, int32_t* state, void* stream);

/* hyd_draft_accept_stop: hyd_draft_accept (hyd_draft_accept_states when the two state arrays are given) with hyd_stop_update's
 * rules applied to EVERY token the row emits in the step, and the penalties' per-sequence token lists kept beside it.  Of `stop`
 * only stop_tokens, stop_lens, n_stop and include_stop are read; its other fields may be null or zero.  A running row
 * (reason == 0, length < max_new_tokens) computes n and e = min(n + 1, room) as hyd_draft_accept does.  Then, for i = 0 .. e - 1
 * in order, with column c = length[b] + i:
 *   1. out[b, c] = sampled[b, i];
 *   2. it equals eos[j] for the lowest j: reason 1, stop_index j, the token is kept, the run ends with e = i + 1;
 *   3. otherwise the stop sequences in list order: sequence k (len_k tokens) matches when c + 1 >= len_k and
 *      out[b, c + 1 - len_k .. c] equals it -- never reaching in front of column 0, but possibly into columns written by earlier
 *      steps; the lowest matching k gives reason 2, stop_index k, and the run ends with e = i + 1.  include_stop == 0: the len_k
 *      matched columns become pad and length[b] = c + 1 - len_k; else they stay and length[b] = c + 1;
 *   4. otherwise the row keeps running: length[b] += e.
 * Draws behind the cut, and rejected draws, never reach out and are never matched.  accepted[b] = e - 1 with the final e, before
 * any trim; out_logprobs is written for the e judged columns; state[b] = step_state_after[b, e - 1] when the state arrays are
 * given.  gen != NULL: the e judged tokens go to gen[b, gen_len[b] ..) as int32, only at positions < gen_stride, and gen_len[b]
 * += e (plain vector stores; a finished row's list does not change).  feed, next_pos (from the length after the trim), *live and
 * finished rows behave exactly as in hyd_draft_accept.  In one sentence: for every row the result equals e successive one-token
 * hyd_stop_update steps over the accepted draws.  stop == NULL (or n_stop == 0) with gen == NULL is byte for byte
 * hyd_draft_accept / hyd_draft_accept_states.
 * HYD_ERR_BAD_ARG: everything hyd_draft_accept_states refuses, n_stop outside [0, HYD_STOP_MAX_SEQS], n_stop > 0 without
 * stop_tokens, a stop length outside [1, HYD_STOP_MAX_LEN], gen without gen_len (or gen_len without gen), gen_stride < 0 or
 * > HYD_SAMPLE_GEN_MAX, misaligned pointers.  rows == 0 succeeds without a launch. */
HYD_API int hyd_draft_accept_stop(const hyd_draft_accept_params* p, const hyd_stop_params* stop, const int32_t* step_state_after,
                                  int32_t* state, int32_t* gen, int32_t* gen_len, int32_t gen_stride, void* stream);

/* hyd_sample_tokens_penalized_drafts: hyd_sample_tokens_penalized over the p->rows = B * T logits rows of a speculative step, with
 * ONE token list per sequence.  Logits row r belongs to sequence b = r / T and fed position i = r % T.  p->gen is
 * [B, gen_stride] and p->gen_len [B].  The row's counts c[v] run over gen[b, 0 .. min(gen_len[b], gen_stride)) followed by
 * fed[b, 1 .. i] (fed int64 [B, T]: the drafts fed in front of the position that row draws; fed[b, 0] is the last emitted token
 * and is already in gen; ids outside [0, n) are ignored).  With gen NULL there are no lists and fed is not read.  The context
 * bitmaps are read at row b / rows_per_group.  Everything else is hyd_sample_tokens_penalized's for logits row r: the bias list,
 * penalties in double with one rounding, cuts, noise from (seed, offset, r), logprobs, kept.  Tokens, kept counts and log-probs
 * are, bit for bit, what hyd_sample_tokens_penalized returns for the B * T-row call in which row r carries the explicit list
 * gen[b] ++ fed[b, 1 .. i] and the context bitmaps have rows_per_group * T.  T == 1 is exactly hyd_sample_tokens_penalized(p).
 * Capture-safe like that call; the kernel has no workspace and writes nothing but out / logprobs / kept.
 * Refusals: everything hyd_sample_tokens_penalized refuses; HYD_ERR_BAD_ARG for T outside [1, 8], rows % T != 0, append_out != 0
 * (hyd_draft_accept_stop owns the lists on this route), a null fed while gen != NULL, a misaligned fed. */
HYD_API int hyd_sample_tokens_penalized_drafts(const hyd_sample_penalty_params* p, const int64_t* fed, int32_t T, void* stream);

/* ------------------------------------------------------------------------------------------
 * All-reduce(sum) of the tensor-parallel block output (hydragen/tp.py:83-87 after down_proj, :108-112 after
 * o_proj; the reference calls torch.distributed / NCCL there) as a two-shot direct exchange over
 * peer-mapped device memory: xGMI is a full mesh, so every rank reads its slice straight from every
 * peer (reduce-scatter), then every reduced slice from its owner (all-gather).  One process per GPU.
 *
 * Each rank owns one zero-initialised "shared block" of hyd_allreduce_block_bytes() bytes of UNCACHED device
 * memory -- hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached), or hipDeviceMallocFinegrained where that is
 * refused; NEVER plain hipMalloc: peers write the block's flags and read its staged payload through the fabric,
 * which does not probe the owner's L2 for coarse-grained allocations (stale reads) -- exports it with
 * hyd_ipc_get_handle, and maps every peer's block with hyd_ipc_open_handle (handles travel over any host channel,
 * e.g. torch.distributed all_gather_object).
 * `blocks` is a HOST array of `world` device pointers: blocks[r] is rank r's block as mapped in THIS
 * process (blocks[rank] is the own block).  `in` / `out` are ordinary device buffers, 16-byte aligned,
 * count * sizeof(dtype) <= max_bytes; in == out is allowed.  Every rank must issue the same sequence of
 * calls.  Capture-safe: the call's epoch lives in the block, not in the arguments.
 * Waiting is bounded by a POLL COUNT, 2^timeout_log2_polls polls of ~0.3 us each per wait (0 = the default
 * 2^27, ~40 s -- longer than any lazy module load, graph capture or shard load between two ranks' calls):
 * a peer that never shows up makes the kernel give up instead of hanging the device; `out` is then NOT the
 * sum, and the block's status word (hyd_allreduce_status) is 1 / 2.  The caller MUST read that word before
 * trusting results of a run (hydragen_amd.tp.check_collectives does, at the end of every generate()).
 * ------------------------------------------------------------------------------------------ */
#define HYD_IPC_HANDLE_BYTES 64
#define HYD_ALLREDUCE_MAX_WORLD 8
HYD_API int hyd_ipc_get_handle(const void* dev_ptr, void* handle_out);
HYD_API int hyd_ipc_open_handle(const void* handle, void** dev_ptr_out);
HYD_API int hyd_ipc_close_handle(void* dev_ptr);

typedef struct hyd_allreduce_params {
    void* const* blocks;  /* HOST array [world] of device pointers (see above)                      */
    const void* in;
    void* out;
    int64_t count;        /* elements                                                              */
    size_t max_bytes;     /* the value the blocks were sized with                                  */
    int32_t dtype;        /* HYD_F16 | HYD_BF16 | HYD_F32; accumulation in fp32                    */
    int32_t rank, world;  /* world <= HYD_ALLREDUCE_MAX_WORLD                                      */
    int32_t timeout_log2_polls; /* 0 = default (27); 10..31: each wait gives up after 2^n polls    */
} hyd_allreduce_params;

HYD_API size_t hyd_allreduce_block_bytes(int32_t world, size_t max_bytes);
HYD_API int hyd_allreduce_sum(const hyd_allreduce_params* p, void* stream);
/* Device pointer of the status word inside a block (uint32: 0 = ok, 1 / 2 = a peer timed out in shot 1 / 2). */
HYD_API const uint32_t* hyd_allreduce_status(const void* own_block);

/* ------------------------------------------------------------------------------------------
 * fp8 unique (per-sequence) K/V caches.  The unique cache may hold OCP e4m3fn bytes (torch.float8_e4m3fn; NOT the fnuz
 * format of gfx942) with one fp32 scale per kv head, separately for K and V: the stored value is
 *     q8 = e4m3fn_rne(clamp(x / scale[h], -448, 448))        (correctly rounded division, round-half-even)
 * (hydragen_amd/kv_quant.py quantize_kv is the definition every kernel matches).  q, out, partials and the shared-prefix
 * caches stay 16-bit; only the unique cache is quantized.  Every e4m3fn value is exactly a bf16 and an f16 value, so the
 * kernels widen without rounding and the quantization is the only new rounding of the operator.
 *
 * The _kvq entry points take the existing parameter struct unchanged plus a hyd_kv_quant:
 *   - kq == NULL, or kq->kv_dtype == the q dtype: exactly the existing entry point;
 *   - kq->kv_dtype == HYD_FP8_E4M3: the unique K/V (suffix / decode) or the caches (rope append) are fp8; their strides
 *     are counted in 1-byte elements (still multiples of 8), and so is the "span < 2 GiB" check of a sequence's cache.
 * hyd_decode_attn_fused_kvq takes every phase.  The workspace query is unchanged: the unique partial of the two-stream form
 * stays in q's dtype.
 * Native fp8 shapes (hyd_kv_quant_supported), D 64 / 128 / 256:
 *   - grouped-query units, for callers that set HYD_KVQ_GQA in hyd_kv_quant.flags (the field was `reserved`, 0, when 0.5.0 was
 *     first released: callers of that time keep the shapes and refusals they were written against): every shape the suffix pass gives its matrix-core kernel with 16-bit caches -- nq * (Hq / Hkv) >= 3
 *     query rows per (sequence, kv head); at D = 256 only with at least 1024 (sequence, kv head, 16-row chunk) units or
 *     fewer than 128 keys.  `out` and `lse` are bit-identical to the 16-bit kernel run on the dequantized caches
 *     (float(q8) * scale[h], rounded to fp32 and then to the q dtype, ties to even: hydragen_amd/kv_quant.py dequantize_kv);
 *   - one query row (nq == 1), Hq == Hkv, and Hkv a multiple of the 64 / (D / 8) heads one wave instruction covers.
 * Other shapes -- units of 2 rows, Hq == Hkv with nq == 2, 2 heads at D = 128, other head dims -- return HYD_ERR_UNSUPPORTED; the
 * Python operators then dequantize into a 16-bit temporary and call the existing path (functional, not fast).
 * single_launch_small with fp8 caches: where the same call with 16-bit caches would run as ONE launch, a grouped-query call
 * returns HYD_ERR_UNSUPPORTED (that form has no fp8 kernel, and the prefix + suffix pair rounds a 16-bit prefix partial the
 * one-launch walk does not: it is not run in its place); Hq == Hkv calls ignore the flag and run the pair, as before.
 * hyd_decode_kv_quant_supported answers for a whole decode call, flags and phase included.
 * ------------------------------------------------------------------------------------------ */
#define HYD_KVQ_GQA 1 /* hyd_kv_quant.flags: grouped-query shapes run on the fp8 matrix-core kernel instead of being refused */
/* hyd_kv_quant.flags: the caller takes the fp8 CAUSAL-TAIL kernel (hyd_suffix_attn_causal_fwd_kvq, hyd_decode_params.causal_tail
 * with hyd_decode_attn_fused_kvq), which is always the matrix-core one: 2..8 query tokens, rows of D bytes, every unit shape the
 * 16-bit matrix-core kernel takes AND units of 2 rows (there is no fp8 one-unit-per-wave kernel); D = 256 only with at least 1024
 * units or fewer than 128 keys.  `out` and `lse` are bit-identical to the 16-bit causal matrix-core kernel on the dequantized
 * caches wherever both take the shape.  Without the flag a causal call with fp8 caches answers what it always has:
 * HYD_ERR_UNSUPPORTED.  With it, a shape no fp8 causal kernel takes is HYD_ERR_UNSUPPORTED: a causal call never runs without
 * the per-row key limit.  The one-launch small form stays off for causal calls. */
#define HYD_KVQ_CAUSAL 2
typedef struct hyd_kv_quant {
    int32_t kv_dtype;     /* HYD_FP8_E4M3, or the q dtype = no quantization                       */
    int32_t flags;        /* 0, or HYD_KVQ_GQA | HYD_KVQ_CAUSAL (formerly `reserved`)            */
    const float* k_scale; /* [Hkv] device, or NULL = 1                                           */
    const float* v_scale; /* [Hkv] device, or NULL = 1                                           */
} hyd_kv_quant;

HYD_API int hyd_suffix_attn_fwd_kvq(const hyd_suffix_params* p, const hyd_kv_quant* kq, void* stream);
HYD_API int hyd_decode_attn_fused_kvq(const hyd_decode_params* p, const hyd_kv_quant* kq, void* stream);
HYD_API int hyd_rope_append_decode_kvq(const hyd_rope_params* p, const hyd_kv_quant* kq, void* stream);
/* The causal tail over fp8 unique caches.  kq == NULL or kv_dtype == the q dtype: exactly hyd_suffix_attn_causal_fwd.  fp8 caches
 * need HYD_KVQ_CAUSAL in kq->flags (above); strides count bytes. */
HYD_API int hyd_suffix_attn_causal_fwd_kvq(const hyd_suffix_params* p, const hyd_kv_quant* kq /* nullable */, void* stream);
/* Shapes only (capture-safe, no device read): 1 when the suffix pass of these shapes runs natively with kq's cache dtype
 * (always 1 for kq == NULL or kv_dtype == dtype), else 0. */
HYD_API int hyd_kv_quant_supported(const hyd_suffix_params* p, const hyd_kv_quant* kq);
/* Shapes only (capture-safe, no device read): 1 exactly when hyd_decode_attn_fused_kvq takes this call natively with kq's
 * cache dtype -- phase, single_launch_small and the levels as given (always 1 for kq == NULL or kv_dtype == dtype) --, else 0. */
HYD_API int hyd_decode_kv_quant_supported(const hyd_decode_params* p, const hyd_kv_quant* kq);

/* Per-head q/k RMSNorm inside the preamble (Qwen3's self_attn.q_norm / k_norm: one gain vector of D elements for every query
 * head, one for every key head, applied between the projection and RoPE).  The _qkn entry points take the existing parameter
 * structs unchanged plus a hyd_qk_norm; qn == NULL is the existing call and launches the existing kernels.  With qn, for every
 * q row and k row x (the 16-bit input widened to fp32)
 *     r = rsqrt(mean_d(x_d^2) + eps),   n_d = x_d * r * w_d,   out = the rotation applied to n,
 * all in fp32 with ONE rounding to the 16-bit dtype at the end (the convention of hyd_add_rmsnorm); v rows are copied as before,
 * fp8 caches receive the quantized 16-bit value as before, and a token gets the same bits from the one-token and the multi-token
 * form.  D 64 / 128 / 256 only: a norm together with a narrow hyd_rope_params.head_dim is HYD_ERR_UNSUPPORTED.  A null or
 * misaligned weight, an eps that is not finite or not > 0, and flags != 0 are HYD_ERR_BAD_ARG. */
typedef struct hyd_qk_norm { const void* q_weight; const void* k_weight; /* [D], the q dtype, 16-byte aligned */
                             float eps; int32_t flags; /* 0 */ } hyd_qk_norm;

HYD_API int hyd_rope_append_decode_qkn(const hyd_rope_params* p, const hyd_kv_quant* kq /* nullable */, const hyd_qk_norm* qn /* nullable */,
                                       void* stream);
HYD_API int hyd_rope_append_multi_qkn(const hyd_rope_multi_params* p, const hyd_qk_norm* qn /* nullable */, void* stream);
/* The multi-token preamble on fp8 caches: token i of a row is rotated at position + i, quantized with its kv head's scale as
 * hyd_rope_append_decode_kvq quantizes it (the same bytes as T one-token calls at positions + i) and written at idx0 + i; a retired
 * row writes nothing, nothing is written at or past cache_len.  kq is checked by hyd_rope_append_decode_kvq's rules (cache strides in
 * bytes, scales 4-byte aligned, NULL scale = 1; its flags are not read); with kq and qn NULL the call is hyd_rope_append_multi. */
HYD_API int hyd_rope_append_multi_kvq(const hyd_rope_multi_params* p, const hyd_kv_quant* kq /* nullable */, const hyd_qk_norm* qn /* nullable */,
                                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Fork completions: promote rows of the UNIQUE K/V caches to a packed SHARED level, K and V in one launch (no forward pass: the
 * rotated K/V of the chosen completions already sit in the unique caches, and a level that comes directly after the levels in
 * use keeps their absolute RoPE positions valid).  For i < n, t < lens[i], every kv head h:
 *     dst[cu[i] + t, h, c] = src[rows[i], t, h, c]   for c < d_src,      = 0   for d_src <= c < d_dst
 * (the pad columns of a destination wider than the source rows are WRITTEN as zeros: the narrow-cache rule of the shared levels);
 * destination tokens at or past cu[n] are not touched.
 *   - source: the unique caches [B, src_rows, Hkv, d_src] by pointer and batch / token / head strides in elements (views of the
 *     [batch, K | V, rows, heads, dim] arena: the batch stride is NOT src_rows * Hkv * d_src), d_src contiguous; HYD_F16, HYD_BF16,
 *     or HYD_FP8_E4M3 (1-byte elements) with per-kv-head fp32 k_scale / v_scale (NULL = 1);
 *   - destination: packed [capacity, Hkv, d_dst] contiguous, HYD_F16 | HYD_BF16; d_dst >= d_src, and 64 / 128 / 256 or == d_src;
 *   - a 16-bit source is copied as BYTES (bit-exact, NaN payloads included; its dtype must be the destination's); an fp8 source
 *     is widened by the rule of the fp8 unique caches above: float(q8) * scale[h] as an fp32 product, rounded once to dst_dtype,
 *     ties to even (hydragen_amd/kv_quant.py dequantize_kv is the definition; bit-identical to it);
 *   - rows / lens / cu are DEVICE arrays read at launch time (capture-safe; cu[i + 1] - cu[i] == lens[i] is the caller's to keep).
 *     A sequence with rows[i] outside [0, B), lens[i] > max_len, cu[i] < 0 or cu[i] + lens[i] > capacity is skipped as a whole:
 *     nothing is indexed with such a value; lens[i] <= 0 copies nothing;
 *   - max_len is the HOST's bound on lens[] (0 = src_rows): the launch grid is sized by it and by n, never by device data.
 * HYD_ERR_BAD_ARG: a null k_src / v_src / k_dst / v_dst / rows / lens / cu, n <= 0, Hkv <= 0, B <= 0, src_rows <= 0, capacity < 0,
 * d_src <= 0 or d_src % 8 != 0, d_dst < d_src, max_len outside [0, src_rows], a 16-bit src_dtype that differs from dst_dtype,
 * strides that are no multiple of 8 elements (or head stride < d_src), pointers that are not 16-byte (rows / lens / cu / scales:
 * 4-byte) aligned.  HYD_ERR_UNSUPPORTED: dst_dtype other than HYD_F16 / HYD_BF16 (no fp8 or 32-bit shared levels), another
 * src_dtype, d_dst that is neither 64 / 128 / 256 nor d_src, n > 65535, max_len * Hkv * d_dst / 8 >= 2^31.
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_kv_promote_params {
    const void* k_src;      /* sequence b, token t, head h at k_src + b*k_batch_stride + t*k_tok_stride + h*k_head_stride */
    const void* v_src;
    void* k_dst;            /* [capacity, Hkv, d_dst] contiguous, dst_dtype                                  */
    void* v_dst;
    const int32_t* rows;    /* [n] source batch index                                                        */
    const int32_t* lens;    /* [n] tokens taken from the front of that row                                   */
    const int32_t* cu;      /* [n + 1] destination token offsets                                             */
    const float* k_scale;   /* [Hkv] or NULL = 1; fp8 sources only                                           */
    const float* v_scale;
    int64_t k_batch_stride, k_tok_stride, k_head_stride; /* elements of src_dtype                            */
    int64_t v_batch_stride, v_tok_stride, v_head_stride;
    int32_t src_dtype;      /* HYD_F16 | HYD_BF16 | HYD_FP8_E4M3                                             */
    int32_t dst_dtype;      /* HYD_F16 | HYD_BF16                                                            */
    int32_t n;              /* sequences to promote                                                          */
    int32_t B, src_rows;    /* sequences and token rows of the source caches                                 */
    int32_t Hkv, d_src, d_dst;
    int32_t capacity;       /* token rows of the destination                                                 */
    int32_t max_len;        /* host bound on lens[]; 0 = src_rows                                            */
} hyd_kv_promote_params;

HYD_API int hyd_kv_promote(const hyd_kv_promote_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fork with merged levels: gather each survivor's whole PATH since the prompt into one packed SHARED level, K and V in one launch.
 * The path of destination sequence i < n is, in order:
 *   - chain segments: for every chain level j < n_levels (0 <= n_levels <= HYD_MAX_LEVELS) the tokens [cu_j[p], cu_j[p + 1]) of
 *     that level, p = rows[i] / level_div[j] (the host passes level_div[j] = old_batch / level_s[j]: sequence r of the previous
 *     batch read shared sequence r / (old_batch / s_j) of a level of s_j sequences).  A level is packed [level_cap[j], Hkv, d_dst]
 *     contiguous K and V of dst_dtype with device offsets level_cu[j] [level_s[j] + 1]; its tokens are copied as BYTES;
 *   - the unique segment: the first lens[i] tokens of unique sequence rows[i], written exactly as hyd_kv_promote writes them
 *     (source layout, dtypes, scales, strides and d_src / d_dst as documented there: a 16-bit source is a byte copy, an e4m3fn
 *     source is widened by the dequantize_kv rule with per-head scales, the pad columns of a wider destination row are zeros).
 * It occupies packed tokens [cu_dst[i], cu_dst[i] + path_i) of k_dst / v_dst [capacity, Hkv, d_dst] contiguous; destination tokens
 * at or past cu_dst[n] are not touched (cu_dst[i + 1] - cu_dst[i] == path_i is the caller's to keep).  THE DESTINATION MUST NOT
 * OVERLAP ANY SOURCE (chain levels or unique caches): a workgroup reads while another writes, in no order.  To replace a chain
 * level by the gathered one, gather into a staging buffer and copy.
 *   - rows / lens / cu_dst and every level_cu[j] are DEVICE arrays read at launch time (capture-safe).  The kernel cannot raise:
 *     a destination sequence is skipped AS A WHOLE, and nothing is indexed with the bad value, when rows[i] is outside [0, B), a
 *     parent index rows[i] / level_div[j] is outside [0, level_s[j]), a segment is negative (cu_j[p] < 0 or cu_j[p + 1] < cu_j[p])
 *     or runs past level_cap[j], lens[i] is outside [0, max_len], the path is longer than max_path, or cu_dst[i] < 0 or
 *     cu_dst[i] + path_i > capacity;
 *   - max_len is the HOST's bound on lens[] (0 = src_rows), max_path the host's bound on a path in tokens (0 = capacity): the
 *     launch grid is sized by max_path, n and K | V, never by device data.  One launch, 16-byte loads and stores, no LDS, no
 *     scratch, no allocation, no synchronisation.
 * HYD_ERR_BAD_ARG: everything hyd_kv_promote refuses with it (cu_dst for cu), n_levels outside [0, HYD_MAX_LEVELS], a null or
 * misaligned level_k[j] / level_v[j] (16 bytes) / level_cu[j] (4 bytes), level_div[j] <= 0, level_s[j] <= 0, level_cap[j] < 0,
 * max_path outside [0, capacity].  HYD_ERR_UNSUPPORTED: what hyd_kv_promote refuses with it, and max_path * Hkv * d_dst / 8 >= 2^31.
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_kv_gather_params {
    const void* level_k[HYD_MAX_LEVELS];      /* chain level j: [level_cap[j], Hkv, d_dst] contiguous, dst_dtype         */
    const void* level_v[HYD_MAX_LEVELS];
    const int32_t* level_cu[HYD_MAX_LEVELS];  /* [level_s[j] + 1] token offsets (device)                                 */
    int32_t level_s[HYD_MAX_LEVELS];          /* sequences of the level                                                  */
    int32_t level_cap[HYD_MAX_LEVELS];        /* token rows of the level                                                 */
    int32_t level_div[HYD_MAX_LEVELS];        /* old_batch / level_s[j]                                                  */
    const void* k_src;      /* unique caches: as hyd_kv_promote_params                                       */
    const void* v_src;
    void* k_dst;            /* [capacity, Hkv, d_dst] contiguous, dst_dtype; overlaps no source              */
    void* v_dst;
    const int32_t* rows;    /* [n] batch index in the previous batch: the unique row, and the parents by it  */
    const int32_t* lens;    /* [n] tokens taken from the front of that unique row (0 is allowed)             */
    const int32_t* cu_dst;  /* [n + 1] destination token offsets                                             */
    const float* k_scale;   /* [Hkv] or NULL = 1; fp8 sources only                                           */
    const float* v_scale;
    int64_t k_batch_stride, k_tok_stride, k_head_stride; /* elements of src_dtype                            */
    int64_t v_batch_stride, v_tok_stride, v_head_stride;
    int32_t src_dtype;      /* HYD_F16 | HYD_BF16 | HYD_FP8_E4M3                                             */
    int32_t dst_dtype;      /* HYD_F16 | HYD_BF16                                                            */
    int32_t n;              /* destination sequences                                                         */
    int32_t n_levels;       /* chain levels, outermost first                                                 */
    int32_t B, src_rows;    /* sequences and token rows of the unique caches                                 */
    int32_t Hkv, d_src, d_dst;
    int32_t capacity;       /* token rows of the destination                                                 */
    int32_t max_len;        /* host bound on lens[]; 0 = src_rows                                            */
    int32_t max_path;       /* host bound on a path in tokens; 0 = capacity                                  */
} hyd_kv_gather_params;

HYD_API int hyd_kv_gather_paths(const hyd_kv_gather_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibrate the per-kv-head scales of the fp8 unique caches from 16-bit K / V (the prompt's, as the prefill computes them).
 *
 * hyd_kv_absmax: for every kv head h, the largest |x| over a strided view [n_outer, n_rows, Hkv, d] of K and of V, folded into
 * the caller's running buffer amax f32 [2, Hkv] (row 0: K, row 1: V) by an integer atomic max on the bit pattern:
 *     amax[t, h] = max(amax[t, h], max over o < n_outer, r < len(o), c < d of |x_t[o, r, h, c]|),  len(o) = row_lens ? row_lens[o] : n_rows
 * (row_lens[o] is clamped to [0, n_rows]).  NaN and +-inf elements are ignored; -0 and subnormals count by magnitude.  The result
 * is exact and does not depend on the order: hydragen_amd/kv_quant.py absmax_reference is the definition.  Rows at or past len(o)
 * and columns at or past d are never read.  amax must hold non-negative finite floats (zero it once); k or v may be NULL: that
 * tensor's row of amax is left as it is.  One launch: geometry from shapes only, no allocation, no synchronisation, no scratch;
 * capture-safe.  A workgroup covers HYD_KV_ABSMAX_PASSES * max(1, 256 / (Hkv * d / 8)) consecutive rows of one outer index.
 *   - element o, r, h, c of K at k + o*k_outer_stride + r*k_row_stride + h*k_head_stride + c (elements; d contiguous);
 *   - dtype HYD_F16 | HYD_BF16 (fp8 sources are not taken); d % 8 == 0, 8 <= d <= 256; Hkv >= 1.
 * HYD_ERR_BAD_ARG: null params or amax, k and v both null, d % 8 != 0 or outside 8..256, Hkv < 1, n_outer / n_rows < 0, k / v not
 * 16-byte aligned, amax / row_lens not 4-byte aligned, a stride that is no multiple of 8 elements.  HYD_ERR_UNSUPPORTED: another
 * dtype, n_rows > 2^30, Hkv * d / 8 > 2^24, more than 2^31 - 1 workgroups.  n_outer * n_rows == 0: HYD_OK, nothing launched.
 *
 * hyd_kv_scales_from_absmax: one small launch, amax [2, Hkv] -> k_scale [Hkv], v_scale [Hkv].  With t = amax * c as an fp32
 * product (c = (float)(margin / 448.0): the host computes it):
 *     scale = 1.0                                                       if amax == 0 (nothing observed, an all-zero head)
 *           = the smallest power of two >= t, clamped to [2^-100, 2^100]   if pow2 (a t that is a power of two is kept)
 *           = t clamped to [2^-100, 2^100]                              otherwise
 * by exponent arithmetic on the bits of t: reproducible bit for bit on the host (kv_quant.py scales_from_absmax_reference).
 * HYD_ERR_BAD_ARG: null params / amax / k_scale / v_scale, pointers not 4-byte aligned, Hkv < 1, c not finite and positive.
 * ------------------------------------------------------------------------------------------ */
#define HYD_KV_ABSMAX_PASSES 16

typedef struct hyd_kv_absmax_params {
    const void* k;           /* may be NULL (then v is not)                                                   */
    const void* v;           /* may be NULL (then k is not)                                                   */
    const int32_t* row_lens; /* [n_outer] or NULL = n_rows                                                    */
    float* amax;             /* [2, Hkv] running maxima, K row then V row                                     */
    int64_t k_outer_stride, k_row_stride, k_head_stride; /* elements                                          */
    int64_t v_outer_stride, v_row_stride, v_head_stride;
    int32_t dtype;           /* HYD_F16 | HYD_BF16                                                            */
    int32_t Hkv, d;
    int32_t n_outer, n_rows;
    int32_t reserved;
} hyd_kv_absmax_params;

typedef struct hyd_kv_scales_params {
    const float* amax;       /* [2, Hkv]                                                                      */
    float* k_scale;          /* [Hkv]                                                                         */
    float* v_scale;          /* [Hkv]                                                                         */
    int32_t Hkv;
    float c;                 /* (float)(margin / 448.0)                                                       */
    int32_t pow2;            /* 1: power-of-two scales; 0: amax * c                                           */
    int32_t reserved;
} hyd_kv_scales_params;

HYD_API int hyd_kv_absmax(const hyd_kv_absmax_params* p, void* stream);
HYD_API int hyd_kv_scales_from_absmax(const hyd_kv_scales_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp8 linear-layer weights (hydragen_amd/weight_quant.py is the definition): W is stored as e4m3fn codes w8 [N, K] with one
 * fp32 scale per output channel, activations and outputs stay 16-bit.  New symbols and structs only: the version stays 500.
 *
 * The skinny GEMM:  y[m, n] = round16(scale[n] * sum_k x[m, k] * w8[n, k]),  fp32 accumulation on the 16-bit matrix cores (the
 * codes are widened in registers, exactly), the scale applied to the fp32 sum, one rounding to the dtype of x (ties to even).
 * x [M, K] and y [M, N] are row-strided views (strides in elements, multiples of 8; unit last stride; 16-byte aligned), w8 is
 * contiguous and 16-byte aligned, K % 16 == 0; M >= 1 and N >= 1 of any size.  Shallow shapes are split along K: the partial
 * sums go to `workspace` as fp32 and a second launch adds them in a fixed order, so a call is bitwise reproducible; the split
 * is planned from M, N and K alone and the workspace-size query below says how many bytes it needs (0 when the plan does not
 * split).  A row of y depends on its own row of x only.  Nothing is allocated: capture-safe.
 * HYD_ERR_BAD_ARG: null params / x / w8 / scale / y, a pointer that is not 16-byte aligned (scale: 4), M / N / K < 1,
 * K % 16 != 0, x_row_stride < K, y_row_stride < N, a stride that is no multiple of 8.  HYD_ERR_UNSUPPORTED: dtype other
 * than HYD_F16 / HYD_BF16, more than 2^31 - 1 workgroups.  HYD_ERR_WORKSPACE: workspace null, misaligned or too small.
 *
 * The widening (the route of calls with more rows than the skinny kernel should take): out[n, k] = float(w8[n, k]) * scale[n]
 * as an fp32 product, rounded once to dtype -- weight_quant.dequantize_weight bit for bit.  out: [N, K] 16-bit with a row
 * stride (elements, a multiple of 8, >= K), 16-byte aligned; K % 8 == 0.  The refusals are those of the GEMM where they apply.
 * ------------------------------------------------------------------------------------------ */
typedef struct hyd_linear_w8_params {
    const void* x;           /* [M, K] dtype, row m at x + m * x_row_stride                                   */
    const void* w8;          /* [N, K] e4m3fn, contiguous                                                     */
    const float* scale;      /* [N]                                                                           */
    void* y;                 /* [M, N] dtype, row m at y + m * y_row_stride                                   */
    void* workspace;         /* fp32 partial sums of a split plan; may be NULL when the query answers 0       */
    size_t workspace_bytes;
    int64_t x_row_stride, y_row_stride;
    int32_t M, N, K;
    int32_t dtype;           /* HYD_F16 | HYD_BF16                                                            */
} hyd_linear_w8_params;

typedef struct hyd_weight_widen_params {
    const void* w8;          /* [N, K] e4m3fn, contiguous                                                     */
    const float* scale;      /* [N]                                                                           */
    void* out;               /* [N, K] dtype, row n at out + n * out_row_stride                               */
    int64_t out_row_stride;
    int32_t N, K;
    int32_t dtype;           /* HYD_F16 | HYD_BF16                                                            */
    int32_t reserved;
} hyd_weight_widen_params;

HYD_API size_t hyd_linear_w8_workspace_bytes(int32_t M, int32_t N, int32_t K);
HYD_API int hyd_linear_w8(const hyd_linear_w8_params* p, void* stream);
HYD_API int hyd_weight_widen(const hyd_weight_widen_params* p, void* stream);

HYD_API int hyd_version(void);
HYD_API const char* hyd_last_error_string(void);

/* Planner query: the split-KV factor, grid and keys per split the prefix pass derives from these shapes (what
 * hyd_prefix_workspace_bytes sizes the scratch for). */
HYD_API int hyd_prefix_plan(const hyd_prefix_params* p, int32_t* num_splits, int32_t* grid, int32_t* split_len);

#ifdef __cplusplus
}
#endif
#endif /* HYDRAGEN_HIP_H */
