// C ABI, attention: the prefix / suffix / causal-tail / combine entry points with the unique pass's one plan, the decode call with
// its one plan (which holds the former), the workspace and support queries.
#include <cstddef>
#include <cstdlib>

#include "api_core.h"

using namespace hyd;

namespace {

constexpr int kNumCU = 256;  // MI355X
constexpr int kMaxSplits = 32;

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Where the slices of one partial live: `count` output slices [rows, D] of esz-byte elements, then -- behind ALL of them --
// `count` fp32 LSE slices [rows].  Every slice is padded to 256 bytes; the strides only matter when there are several
// (slice j of a hyd_partial is at out + j * out_stride, lse + j * lse_stride), and a lone slice's LSE starts at lse_base
// like any other.  The one statement of the rule: workspace sizes, carving and the expansion of stacked partials all ask here.
struct SliceLayout {
    size_t out_stride, lse_stride, lse_base, bytes;
};
SliceLayout slice_layout(size_t rows, int D, size_t esz, int count) {
    SliceLayout l;
    l.out_stride = align_up(rows * D * esz, 256);
    l.lse_stride = align_up(rows * sizeof(float), 256);
    l.lse_base = (size_t)count * l.out_stride;
    l.bytes = (size_t)count * (l.out_stride + l.lse_stride);
    return l;
}

// Every slice of stacked partials in order: f(n, out, lse, is_f32) for slice number n.  *n_slices = how many there were.
template <typename F>
int for_each_slice(const hyd_partial* parts, int n_parts, size_t rows, int D, int* n_slices, F&& f) {
    int n = 0;
    for (int i = 0; i < n_parts; ++i) {
        if (!parts[i].out || !parts[i].lse || parts[i].count <= 0)
            return fail(HYD_ERR_BAD_ARG, "partial %d: null pointer or non-positive count", i);
        const SliceLayout l = slice_layout(rows, D, parts[i].is_f32 ? 4 : 2, parts[i].count);
        for (int j = 0; j < parts[i].count; ++j, ++n) {
            if (n >= kMaxCombine) return fail(HYD_ERR_UNSUPPORTED, "more than %d partials", kMaxCombine);
            f(n, static_cast<const char*>(parts[i].out) + (size_t)j * l.out_stride,
              reinterpret_cast<const float*>(reinterpret_cast<const char*>(parts[i].lse) + (size_t)j * l.lse_stride), parts[i].is_f32);
        }
    }
    *n_slices = n;
    return HYD_OK;
}

// Development switches exist only in HYD_ABLATION_BUILD libraries (A/B measurements on hardware); the product library
// reads no environment variable and keeps no mutable state.
inline int dev_switch(const char* name) {
#ifdef HYD_ABLATION_BUILD
    const char* e = getenv(name);
    return e ? atoi(e) : 0;
#else
    (void)name;
    return 0;
#endif
}

struct PrefixPlan {
    int g, per, row_blocks, nsplit, split_len, grid, qpg, wg_rows;
};

// softmax scale in base-2 exponent units: the caller's scale when it gives one, D^-0.5 otherwise
float scale_log2e_of(float softmax_scale, int D) {
    return (softmax_scale > 0.f ? softmax_scale : 1.0f / sqrtf((float)D)) * kLog2e;
}

int plan_prefix(const hyd_prefix_params* p, PrefixPlan* pl, int max_splits = kMaxSplits) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D);
    if (!rc) rc = check_scale(p->softmax_scale);
    if (rc) return rc;
    if (p->sb <= 0) return fail(HYD_ERR_BAD_ARG, "sb %d", p->sb);
    if (p->kv_len < 0) return fail(HYD_ERR_BAD_ARG, "kv_len %d", p->kv_len);
    pl->g = p->Hq / p->Hkv;
    int qtok_per_group;
    if (p->cu_seqlens_q) {
        if (p->nq != 1) return fail(HYD_ERR_BAD_ARG, "cu_seqlens_q requires nq == 1 (packed query tokens)");
        if (p->max_q_len <= 0) return fail(HYD_ERR_BAD_ARG, "cu_seqlens_q requires max_q_len > 0");
        qtok_per_group = p->max_q_len;
        pl->per = 1;
    } else {
        if (p->B % p->sb != 0) return fail(HYD_ERR_BAD_ARG, "batch %d not divisible by shared batch %d", p->B, p->sb);
        pl->per = p->B / p->sb;
        qtok_per_group = pl->per * p->nq;
    }
    pl->qpg = qtok_per_group;
    const int64_t mrows = (int64_t)qtok_per_group * pl->g;
    pl->row_blocks = (int)((mrows + 127) / 128);
    pl->wg_rows = 128;
    {
        // 256-row workgroups (D = 128) when 128-row ones would need more than one round of the chip anyway: half the
        // K/V staging per flop and no cross-half merge.
        const int force_rows = dev_switch("HYD_PREFIX_ROWS");  // 0 in product builds
        const int64_t units128 = (int64_t)p->sb * p->Hkv * pl->row_blocks;
        const bool can = p->D != 256;  // D = 256: one query block per wave, 128-row workgroups only
        if (can && (force_rows == 256 || (force_rows == 0 && units128 > kNumCU))) {
            pl->wg_rows = 256;
            pl->row_blocks = (int)((mrows + 255) / 256);
        }
    }
    const int64_t units = (int64_t)p->sb * p->Hkv * pl->row_blocks;
    int ns = p->num_splits;
    if (ns <= 0) {
        // shapes-only heuristic: the prefix kernel runs one workgroup per CU (128 KB of LDS), so aim for ONE round of
        // at most kNumCU workgroups (a second, partly filled round costs a whole extra pass plus its fixed ~12 us);
        // keep >= 256 keys per split
        ns = 1;
        if (units <= kNumCU / 2) {
            const int max_by_len = p->kv_len / 256 > 0 ? p->kv_len / 256 : 1;
            const int want = (int)(kNumCU / units);
            ns = want < max_by_len ? want : max_by_len;
            // ... but every split is one more fp32 slice of ALL rows written here and read back by the consumer.  With the
            // workgroups in one round the pass takes about fixed + (kv_len / ns) c + ns s1: c = 13.6 ns per key of a 128-row unit
            // (C2's key loop), s1 = what a slice costs, calibrated at twice its write + read time at 5 TB/s on the sweeps of
            // profiles/r05_split_plan_sweep.txt (the consumer's epilogue pays for it in latency as well).  The minimum is at
            // ns = sqrt(kv_len c / s1): C3 16, a TP = 8 shard of C2 (4/4 heads) 4 instead of 8 (whole call 48.4 -> 43.4 us),
            // B = 64, 32/8 heads, P = 4096 8 instead of 16 (37.1 -> 30.9), B = 256, 32/32, P = 512 unsplit (67.2 -> 62.8).
            // c is per key of a 128-row unit at D = 128; the loop's MFMAs per key (D / 16 for QK^T + D / 16 for PV) and the staged bytes
            // scale with D, and so does a slice (s1): the optimum is the same split count at every head dim.
            const double c_us = 0.0136 * (double)p->D / 128.0;
            const double s1_us = (double)p->B * p->nq * p->Hq * p->D * 16.0 / 5.0e6;
            const double best = sqrt((double)p->kv_len * c_us / s1_us);
            const int by_cost = best < 1.5 ? 1 : (int)(best + 0.5);
            if (by_cost < ns) ns = by_cost;
        }
    }
    if (p->cu_seqlens_q) ns = 1;  // merged LSE re-layout needs uniform query counts
    if (max_splits > kMaxSplits) max_splits = kMaxSplits;
    if (ns > max_splits) ns = max_splits;
    if (ns < 1) ns = 1;
    int split_len = (int)align_up((size_t)((p->kv_len + ns - 1) / ns), 128);
    if (split_len == 0) split_len = 128;
    ns = p->kv_len > 0 ? (p->kv_len + split_len - 1) / split_len : 1;
    // The prefix kernel addresses one split's keys through a 32-bit buffer resource + scalar offset (it issues blocks up
    // to 4 x 32 rows past the end, which must not wrap): cut longer spans into more splits, or refuse.
    {
        const int64_t ts = p->k_tok_stride > p->v_tok_stride ? p->k_tok_stride : p->v_tok_stride;
        const int64_t max_rows = ts > 0 ? (((int64_t)1 << 31) / (ts * 2)) - 512 : (int64_t)1 << 30;
        if (max_rows < 128) return fail(HYD_ERR_UNSUPPORTED, "token stride %lld elements is too large for 32-bit key offsets", (long long)ts);
        if (split_len > max_rows) {
            split_len = (int)(max_rows / 128 * 128);
            ns = (p->kv_len + split_len - 1) / split_len;
            if (ns > kMaxSplits || p->cu_seqlens_q)
                return fail(HYD_ERR_UNSUPPORTED, "%d keys at a token stride of %lld elements exceed the 2 GiB per split the prefix pass addresses",
                            p->kv_len, (long long)ts);
        }
    }
    pl->nsplit = ns;
    pl->split_len = split_len;
    const int64_t grid = units * ns;
    if (grid <= 0 || grid > 0x7fffffff) return fail(HYD_ERR_UNSUPPORTED, "grid too large");
    pl->grid = (int)grid;
    return HYD_OK;
}

// Split-KV slices are fp32 everywhere.  (16-bit slices on the fused decode path were measured: C3 80.5 -> 79.3 us,
// C5 145.7 -> 140.9 us flushed, but every slice then carries its own rounding and the bf16 mean relative difference
// of C3 / C5 / deep hierarchies rose from 0.8 % to 1.1-1.2 %, above the bound the parity tests state.)
size_t prefix_ws_bytes(const hyd_prefix_params* p, const PrefixPlan& pl) {
    if (pl.nsplit <= 1) return 0;
    return slice_layout((size_t)p->B * p->nq * p->Hq, p->D, sizeof(float), pl.nsplit).bytes;
}

void fill_prefix_args(const hyd_prefix_params* p, const PrefixPlan& pl, PrefixArgs* a) {
    memset(a, 0, sizeof(*a));
    a->q = p->q; a->k = p->k; a->v = p->v; a->cu_k = p->cu_seqlens_k; a->cu_q = p->cu_seqlens_q;
    a->k_gs = p->k_group_stride; a->k_ts = p->k_tok_stride; a->k_hs = p->k_head_stride; a->v_gs = p->v_group_stride; a->v_ts = p->v_tok_stride; a->v_hs = p->v_head_stride;
    a->B = p->B; a->nq = p->nq; a->Hq = p->Hq; a->Hkv = p->Hkv; a->g = pl.g; a->sb = p->sb; a->per = pl.per; a->kv_len = p->kv_len;
    a->row_blocks = pl.row_blocks; a->wg_rows = pl.wg_rows;
    // Two waves per SIMD (8-wave workgroups of 32-row waves) wherever that unit is built: D = 128, one workgroup per unit
    // (persistent launches keep the 4-wave unit: launch_prefix_w64_t).  Same rows per workgroup, rings and results; fewer
    // cycles (the SIMD issues one wave's VALU / LDS / DMA instructions beside the other's MFMAs), the same energy: 10 %
    // faster where the pass is short (P = 128: 9.8 against 11.0 us), equal where the chip runs at its power limit.
    {
        const int force_waves = dev_switch("HYD_PREFIX_WAVES");  // 0 in product builds
        a->waves = (p->D == 128 && force_waves != 4) ? 8 : 4;
    }
    a->nsplit = pl.nsplit; a->split_len = pl.split_len; a->vgrid = pl.grid; a->lse_q_stride = pl.qpg;
    a->scale_log2e = scale_log2e_of(p->softmax_scale, p->D); a->div_row_blocks = make_fastdiv((uint32_t)pl.row_blocks);
    a->div_nsplit = make_fastdiv((uint32_t)pl.nsplit); a->div_hkv = make_fastdiv((uint32_t)p->Hkv); a->div_g = make_fastdiv((uint32_t)pl.g);
    a->dbg = dev_switch("HYD_DBG");  // timing-ablation kernel variants; always 0 in product builds
}

// Run the prefix pass.  With nsplit > 1 the kernel writes fp32 slices + BQH LSEs into `ws`; if
// `merge` they are then combined into p->out / p->lse, otherwise the caller consumes the slices.
int launch_prefix_any(const PrefixArgs& a, int dtype, int D, bool causal, int grid, int max_wgs, hipStream_t s) {
    // max_wgs > 0: at most that many PERSISTENT workgroups walk the units (hyd_decode_params.shared_max_workgroups: the
    // rest of the chip stays free for work on another stream); 0 = one workgroup per unit
#ifdef HYD_ABLATION_BUILD
    if (const int np = dev_switch("HYD_PREFIX_PERSIST")) max_wgs = np;
#endif
    if (max_wgs > 0 && grid > max_wgs) grid = max_wgs;
    return launch_prefix_w64(a, dtype, D, causal, grid, s);
}

int run_prefix(const hyd_prefix_params* p, const PrefixPlan& pl, bool merge, hipStream_t s, int max_wgs = 0, bool out_f32 = false) {
    PrefixArgs a;
    fill_prefix_args(p, pl, &a);
    const size_t rows = (size_t)p->B * p->nq * p->Hq;
    if (pl.nsplit == 1) {
        a.out = p->out;
        a.lse = p->lse;
        a.out_f32 = out_f32 ? 1 : 0;  // only the decode entry asks for an fp32 partial (hyd_decode_params.f32_partials)
        a.lse_layout = p->lse_layout;
        return launched(launch_prefix_any(a, p->dtype, p->D, p->causal != 0, pl.grid, max_wgs, s), "prefix kernel launch");
    }
    const SliceLayout l = slice_layout(rows, p->D, sizeof(float), pl.nsplit);
    if (!p->workspace || p->workspace_bytes < l.bytes)
        return fail(HYD_ERR_WORKSPACE, "prefix pass needs %zu workspace bytes, got %zu", l.bytes, p->workspace_bytes);
    char* ws = static_cast<char*>(p->workspace);
    const hyd_partial slices = {ws, reinterpret_cast<float*>(ws + l.lse_base), pl.nsplit, /*is_f32=*/1};
    a.out = ws;
    a.lse = const_cast<float*>(slices.lse);
    a.out_f32 = 1;
    a.lse_layout = HYD_LSE_BQH;
    a.out_split_stride = (int64_t)(l.out_stride / sizeof(float));
    a.lse_split_stride = (int64_t)(l.lse_stride / sizeof(float));
    int rc = launched(launch_prefix_any(a, p->dtype, p->D, p->causal != 0, pl.grid, max_wgs, s), "prefix kernel launch");
    if (rc || !merge) return rc;
    CombineArgs c;
    memset(&c, 0, sizeof(c));
    if ((rc = for_each_slice(&slices, 1, rows, p->D, &c.n, [&c](int n, const void* out, const float* lse, int) {
            c.outs[n] = out;
            c.lses[n] = lse;
        })))
        return rc;
    c.rows = (int64_t)rows;
    c.D = p->D;
    c.dtype_in = HYD_F32;
    c.dtype_out = p->dtype;
    c.out = p->out;
    c.out_lse = p->lse;
    c.lse_layout = p->lse_layout;
    c.Hq = p->Hq;
    c.qpg = pl.qpg;
    return launched(launch_combine(c, s), "combine kernel launch");
}

// the elements per head of the unique cache rows when they are narrower than D, else 0
int narrow_kv_dim(const hyd_suffix_params* p) { return p->kv_dim != p->D ? p->kv_dim : 0; }
// the softmax scale of a call: the caller's, else that of the TRUE head dim (kv_dim when the unique rows are narrow)
float true_dim_scale(const hyd_suffix_params* p) {
    if (p->softmax_scale > 0.f || !narrow_kv_dim(p)) return p->softmax_scale;
    return (float)(1.0 / sqrt((double)p->kv_dim));
}

int check_suffix(const hyd_suffix_params* p) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D);
    if (!rc) rc = check_scale(p->softmax_scale);
    if (!rc) rc = check_narrow_dim(p->kv_dim, p->D, "kv_dim");
    if (rc) return rc;
    if (p->kv_len < 0) return fail(HYD_ERR_BAD_ARG, "kv_len %d", p->kv_len);
    if ((rc = check_ptrs_align({{p->q, "q"}, {p->out, "out"}}))) return rc;
    if (p->kv_len == 0) return HYD_OK;
    if ((rc = check_ptrs_align({{p->k, "k"}, {p->v, "v"}}))) return rc;
    return check_strides8({{p->k_batch_stride, "k_batch_stride"}, {p->k_tok_stride, "k_tok_stride"}, {p->k_head_stride, "k_head_stride"},
                           {p->v_batch_stride, "v_batch_stride"}, {p->v_tok_stride, "v_tok_stride"}, {p->v_head_stride, "v_head_stride"}});
}

void fill_suffix_args(const hyd_suffix_params* p, SuffixArgs* ap) {  // *ap is zeroed (plan_suffix, the one caller)
    SuffixArgs& a = *ap;
    a.q = p->q; a.k = p->k; a.v = p->v; a.out = p->out; a.lse = p->lse; a.sl32 = p->seq_lens_i32; a.sl64 = p->seq_lens_i64; a.order = p->seq_order;
    a.k_bs = p->k_batch_stride; a.k_ts = p->k_tok_stride; a.k_hs = p->k_head_stride; a.v_bs = p->v_batch_stride; a.v_ts = p->v_tok_stride; a.v_hs = p->v_head_stride;
    a.B = p->B; a.nq = p->nq; a.Hq = p->Hq; a.Hkv = p->Hkv;
    a.g = p->Hq / p->Hkv;
    a.kv_len = p->kv_len; a.rows = p->nq * a.g; a.units = p->B * p->Hkv; a.scale_log2e = scale_log2e_of(true_dim_scale(p), p->D);
    a.kv_dim = p->kv_len > 0 ? narrow_kv_dim(p) : 0;  // (no unique key, nothing narrow to read: the merge-only call of the D-wide kernels)
}

int fail_narrow_shapes(int kv_dim, int D) {
    return fail(HYD_ERR_UNSUPPORTED, "kv_dim %d: narrow unique caches run on the token-row kernel only (nq == 1, Hq == Hkv, Hkv a multiple of %d at D = %d, "
                                     "a sequence's cache within 2 GiB)", kv_dim, 64 / (D / 8), D);
}

// HYD_KVQ_GQA: the caller takes the grouped-query fp8 kernel; without it the entry points keep the shapes of ABI 0.5.0 as first
// released (callers of that time route refused shapes to a fallback of their own, and go on doing so)
bool kvq_takes_gqa(const hyd_kv_quant* kq) { return kq && (kq->flags & HYD_KVQ_GQA) != 0; }

int fail_kvq_shapes(int D) {
    return fail(HYD_ERR_UNSUPPORTED,
                "fp8 unique caches: shapes not native (grouped-query units of nq * Hq / Hkv >= 3 rows with hyd_kv_quant.flags & HYD_KVQ_GQA, or nq == 1, Hq == Hkv with Hkv a "
                "multiple of %d at D = %d; D 64 / 128 / 256)", D >= 8 ? 64 / (D / 8) : 0, D);
}

// HYD_KVQ_CAUSAL: the caller takes the fp8 causal-tail kernel; without it a causal call with fp8 caches keeps the refusal it has always had
bool kvq_takes_causal(const hyd_kv_quant* kq) { return kq && (kq->flags & HYD_KVQ_CAUSAL) != 0; }

// The causal tail (hyd_suffix_attn_causal_fwd[_kvq], hyd_decode_params.causal_tail): 2..8 query tokens, caches with rows of D elements.
int check_causal_tail(const hyd_suffix_params* p, const hyd_kv_quant* kq) {
    if (p->nq < 2 || p->nq > 8) return fail(HYD_ERR_BAD_ARG, "causal tail: nq = %d query tokens per sequence, 2 to 8 are taken", p->nq);
    if (kq && !kvq_takes_causal(kq)) return fail(HYD_ERR_UNSUPPORTED, "causal tail with fp8 unique caches: implemented for 16-bit caches only");
    if (p->kv_len > 0 && narrow_kv_dim(p)) return fail(HYD_ERR_UNSUPPORTED, "causal tail with kv_dim %d: narrow unique rows run on the token-row kernel, which has no causal form", p->kv_dim);
    return HYD_OK;
}

int fail_causal_shapes() { return fail(HYD_ERR_UNSUPPORTED, "causal tail: no kernel with the per-row key limit takes these shapes"); }

// ---- one plan per unique pass -----------------------------------------------------------------------------------------
// Which suffix kernel takes a call, if any: asked of the kernels' own *_eligible functions HERE and nowhere else in this file.  The
// support queries, the entry points' refusals and the launch all read a SuffixPlan, so they cannot disagree.  The plan holds facts,
// not a first refusal: each entry point answers bad input in an order of its own (tests/golden/abi_table.json pins every one).
enum SuffixRoute {
    kRoute16,         // launch_suffix, which goes on choosing between its grouped-query / token-row / narrow / one-unit-per-wave kernels
    kRouteFp8Rows,    // launch_suffix_fp8: the token-row kernel
    kRouteFp8Gqa,     // launch_suffix_gqa_fp8: the matrix-core kernel
    kRouteCausal16,   // launch_suffix_causal
    kRouteCausalFp8,  // launch_suffix_gqa_fp8_causal
    kRouteMergeOnly,  // no unique key, 16-bit, not causal: launch_suffix merges the partials (an fp8 or a causal call keeps its launcher)
};
struct SuffixPlan {
    bool valid;          // the shapes are what check_suffix takes (the queries ask about shapes nobody validated); false: nothing below is set
    const hyd_suffix_params* p;  // the call as planned ...
    const hyd_kv_quant* kq;      // ... null, or fp8 unique caches (K/V strides in bytes)
    bool causal;         // ... the causal tail
    SuffixRoute route;  // where the call goes once the verdicts its entry point answers for hold
    bool narrow;         // narrow rows are read (kv_dim set, unique keys present); with fp8 caches: no kernel
    bool narrow_native;  // ... and the narrow token-row kernel takes the shapes
    bool fp8_native;     // an fp8 kernel takes the shapes, with the caller's HYD_KVQ_GQA as it stands
    bool fp8_gqa;        // ... and it is the grouped-query one (whose 16-bit twin tiny decode calls fold into one launch)
    bool causal_native;  // a kernel with the per-row key limit takes the shapes; fp8: HYD_KVQ_CAUSAL given, and 2-row units are taken as well
    bool gqa_any_rows;   // the grouped-query kernel can walk these units at any row count (the one-launch decode form)
    bool span_ok, grid_ok;  // a sequence's K/V span is below 2 GiB at the cache's element size; kv heads and query rows fit the suffix grid
    SuffixArgs args;     // filled once; run_suffix adds the partial slices
};

// Shapes only: no HIP call, and no word to the error string unless the shapes themselves are invalid (which every launch entry point
// has refused before it plans).
void plan_suffix(const hyd_suffix_params* p, const hyd_kv_quant* kq, bool causal, SuffixPlan* pl) {
    memset(pl, 0, sizeof(*pl));
    if (check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D) || check_narrow_dim(p->kv_dim, p->D, "kv_dim")) return;
    pl->valid = true; pl->p = p; pl->kq = kq; pl->causal = causal;
    fill_suffix_args(p, &pl->args);
    const SuffixArgs& a = pl->args;
    const int D = p->D, esz = kq ? 1 : 2;
    pl->narrow = a.kv_dim != 0;
    pl->narrow_native = pl->narrow && suffix_narrow_eligible(a, D);
    // the 16-bit launcher's order: grouped-query shapes to the matrix-core kernel, one-row units to the token-row kernel
    pl->fp8_gqa = !pl->narrow && kvq_takes_gqa(kq) && suffix_gqa_fp8_eligible(a, D);
    pl->fp8_native = !pl->narrow && (pl->fp8_gqa || suffix_fp8_eligible(a, D));
    pl->causal_native = causal && (kq ? kvq_takes_causal(kq) && suffix_gqa_fp8_causal_eligible(a, D) : suffix_causal_eligible(a, D));
    pl->gqa_any_rows = suffix_gqa_eligible(a, D, /*any_shape=*/true);
    pl->span_ok = (int64_t)p->kv_len * p->k_tok_stride * esz < (1ll << 31) && (int64_t)p->kv_len * p->v_tok_stride * esz < (1ll << 31);
    pl->grid_ok = p->Hkv <= 4 * 65535 && a.rows <= 8 * 65535;
    pl->route = causal ? (kq ? kRouteCausalFp8 : kRouteCausal16) : kq ? (pl->fp8_gqa ? kRouteFp8Gqa : kRouteFp8Rows) : p->kv_len == 0 ? kRouteMergeOnly : kRoute16;
}

int check_suffix_limits(const SuffixPlan& pl) {
    if (!pl.span_ok) return fail(HYD_ERR_UNSUPPORTED, "unique K/V of one sequence spans >= 2 GiB (32-bit in-sequence offsets)");
    if (!pl.grid_ok) return fail(HYD_ERR_UNSUPPORTED, "too many kv heads / query rows for the suffix grid");
    return HYD_OK;
}

// The unique pass of a validated call (check_suffix, check_kvq, and check_causal_tail where it is causal): the partials, then the
// limits, then what no kernel takes, in the order the suffix entry points have always answered; then the launch the plan names.
int run_suffix(const SuffixPlan& pl, const hyd_partial* parts, int n_parts, hipStream_t s) {
    SuffixKvqArgs ka = {pl.kq ? pl.kq->k_scale : nullptr, pl.kq ? pl.kq->v_scale : nullptr, pl.args};  // (the scales: fp8 caches only)
    SuffixArgs& a = ka.a;
    const int dtype = pl.p->dtype, D = pl.p->D;
    int rc = for_each_slice(parts, n_parts, (size_t)a.B * a.nq * a.Hq, D, &a.n_partials, [&a](int n, const void* out, const float* lse, int is_f32) {
        a.partials[n] = {out, lse, is_f32, /*pad=*/0};
    });
    if (rc) return rc;
    a.n_pre = 0;
    while (a.n_pre < 2 && a.n_pre < a.n_partials && !a.partials[a.n_pre].is_f32) ++a.n_pre;
    if ((rc = check_suffix_limits(pl))) return rc;
    if (pl.causal && !pl.causal_native) return fail_causal_shapes();  // the causal tail: to a kernel with the per-row key limit or nowhere
    if (!pl.causal && pl.narrow && pl.kq) return fail_narrow_fp8();
    if (!pl.causal && pl.narrow && !pl.narrow_native) return fail_narrow_shapes(a.kv_dim, D);
    if (!pl.causal && pl.kq && !pl.fp8_native) return fail_kvq_shapes(D);
    switch (pl.route) {
        case kRouteFp8Rows: return launched(launch_suffix_fp8(ka, dtype, D, s), "fp8 suffix kernel launch");
        case kRouteFp8Gqa: return launched(launch_suffix_gqa_fp8(ka, dtype, D, s), "fp8 suffix kernel launch");
        case kRouteCausal16: return launched(launch_suffix_causal(a, dtype, D, s), "causal-tail suffix kernel launch");
        case kRouteCausalFp8: return launched(launch_suffix_gqa_fp8_causal(ka, dtype, D, s), "fp8 causal-tail suffix kernel launch");
        default: return launched(launch_suffix(a, dtype, D, s), "suffix kernel launch");  // kRoute16, kRouteMergeOnly
    }
}

void level_to_prefix(const hyd_decode_params* p, int i, hyd_prefix_params* pp) {
    const hyd_suffix_params& s = p->suffix;
    const hyd_level& lv = p->levels[i];
    memset(pp, 0, sizeof(*pp));
    pp->q = s.q; pp->k = lv.k; pp->v = lv.v; pp->cu_seqlens_k = lv.cu_seqlens_k;
    pp->k_group_stride = lv.k_group_stride; pp->k_tok_stride = lv.k_tok_stride; pp->k_head_stride = lv.k_head_stride;
    pp->v_group_stride = lv.v_group_stride; pp->v_tok_stride = lv.v_tok_stride; pp->v_head_stride = lv.v_head_stride;
    pp->dtype = s.dtype; pp->B = s.B; pp->nq = s.nq; pp->Hq = s.Hq; pp->Hkv = s.Hkv; pp->D = s.D; pp->softmax_scale = true_dim_scale(&s);
    pp->sb = lv.sb; pp->kv_len = lv.kv_len; pp->causal = 0; pp->lse_layout = HYD_LSE_BQH; pp->num_splits = 0;
}

// A shared level whose groups are small (few query rows per (group, kv head), short prefix) wastes the prefix
// kernel: one 512-thread workgroup with ~12 us of fixed cost per (group, head) for a fraction of a 128 x 128 tile
// (C4's second level, 32 groups x 32 queries x 64 keys: 1024 workgroups = 4 rounds = 52 us for 1 GFLOP).  Such a
// level is the matrix-core suffix kernel's problem with "sequence" = group: nq' = per * nq query tokens per group
// over the group's P keys, one wave per (group, kv head, 16-row chunk).  Shapes-only decision (capture-safe).
bool level_is_small(const hyd_prefix_params& pp, const PrefixPlan& pl) {
    if (dev_switch("HYD_LEVEL_PREFIX") || pp.cu_seqlens_k || pp.cu_seqlens_q || pp.causal) return false;
    if (pp.D != 64 && pp.D != 128) return false;
    const int64_t rows = (int64_t)pl.qpg * pl.g;  // query rows per (group, kv head)
    if (rows > 64 || pp.kv_len > 1024) return false;
    const int64_t ts = pp.k_tok_stride > pp.v_tok_stride ? pp.k_tok_stride : pp.v_tok_stride;
    return (int64_t)pp.kv_len * ts * 2 < ((int64_t)1 << 31) && pp.Hkv <= 65535;
}

int run_level_small(const hyd_prefix_params& pp, const PrefixPlan& pl, void* out, float* lse, hipStream_t s) {
    SuffixArgs a;
    memset(&a, 0, sizeof(a));
    a.q = pp.q; a.k = pp.k; a.v = pp.v; a.out = out; a.lse = lse;
    a.k_bs = pp.k_group_stride; a.k_ts = pp.k_tok_stride; a.k_hs = pp.k_head_stride;
    a.v_bs = pp.v_group_stride; a.v_ts = pp.v_tok_stride; a.v_hs = pp.v_head_stride;
    a.B = pp.sb; a.nq = pl.qpg; a.Hq = pp.Hq; a.Hkv = pp.Hkv; a.g = pl.g; a.kv_len = pp.kv_len;
    a.rows = pl.qpg * pl.g;
    a.units = pp.sb * pp.Hkv;
    a.scale_log2e = scale_log2e_of(pp.softmax_scale, pp.D);
    a.shared_kv = 1;
    return launched(launch_suffix_gqa(a, pp.dtype, pp.D, s), "small-level kernel launch");
}

// The suffix epilogue merges at most kMaxCombine partials, so the levels of one decode call share that budget:
// each level may cut its keys into at most kMaxCombine / n_levels slices (>= 8 with HYD_MAX_LEVELS = 8).
int level_split_cap(int n_levels) { return n_levels > 0 ? kMaxCombine / n_levels : kMaxSplits; }

// ---- one plan per decode call -----------------------------------------------------------------------------------------
// Everything the shapes of a hyd_decode_params decide, derived in ONE place: the size queries, the support queries and the
// launch all read a DecodePlan -- the levels, and the call's one SuffixPlan -- and plan nothing of their own, so they cannot disagree.
enum DecodeForm {
    kPrefixOnly,  // attention.py:273-274: a single shared level and no unique keys -> the prefix result IS the answer
    kOneLaunch,   // single_launch_small applies (16-bit caches): one grouped-query kernel walks both segments
    kInOrder,     // the level passes fill the workspace, the suffix pass merges them in its epilogue
    kTwoStream,   // HYD_PHASE_UNIQUE_PARTIAL / HYD_PHASE_MERGE: the unique pass leaves a partial of its own, one combine merges all
};
struct LevelPlan {
    hyd_prefix_params pp;  // the level as a prefix pass (out / lse / workspace are set when the workspace is carved)
    PrefixPlan pl;
    bool small;          // level_is_small: the grouped-query kernel runs it, unsplit, into a 16-bit partial
    int count, is_f32;   // its partial: `count` slices (split-KV slices are fp32 everywhere) ...
    SliceLayout layout;  // ... laid out like this in the level's layout.bytes of the workspace
};
struct DecodePlan {
    DecodeForm form;
    bool two_stream_ok;  // the shapes have both a shared and a unique part
    int rc;              // HYD_OK, or what plan_prefix said of level `n_planned` (the message is in g_err)
    int n_planned;       // levels planned: all of them when rc == HYD_OK
    LevelPlan level[HYD_MAX_LEVELS];
    int n_parts;          // slices of all levels' partials
    size_t levels_bytes;  // the levels' regions (kPrefixOnly: the split-KV slices of the one pass, which writes straight to `out`)
    SliceLayout unique;   // behind them, the unique pass's own 16-bit partial of the two-stream form; bytes = 0 without both parts
    SuffixPlan suffix;    // the unique pass, once for every phase; without unique keys the merge-only pass (last: plan_suffix zeroes it)
};

// hyd_decode_params.single_launch_small: one uniform shared level that already counts as small (few query rows per
// (group, kv head), short prefix), unique keys present, the same token strides in the shared and the unique tensors, and
// so few keys in all that the call is launch latency.  Measured per graph-replayed call (tests/probes/single_launch_probe.py,
// units x keys = B * Hkv * (P + S)): 1152 keys (BASELINE config 1) 6.8 -> 4.1 us, 2176 keys 11.4 -> 8.1, 8072 keys (two
// sequences on a 1000-key prefix) 19.5 -> 16.5, 8704 keys (32 sequences) 14.0 -> 14.1: even.  Shapes only: capture-safe.
constexpr int64_t kSingleLaunchMaxKeys = 8192;
bool decode_runs_as_one_launch(const hyd_decode_params* p, const LevelPlan& lv, const SuffixPlan& u) {
    const hyd_suffix_params& sp = p->suffix;
    if (p->phase != HYD_PHASE_ALL || !p->single_launch_small || p->n_levels != 1 || !lv.small || sp.kv_len <= 0) return false;
    if (p->causal_tail) return false;  // the walk over both segments has no per-row key limit: the pair of launches runs
    if (u.narrow) return false;  // narrow unique caches: the pair of launches runs (the rule Hq == Hkv fp8 calls have)
    if (sp.lse) return false;  // suffix.lse is the LSE of the unique keys alone in every form; one walk over both segments cannot give it
    const hyd_prefix_params& pp = lv.pp;
    if (pp.cu_seqlens_k || pp.sb <= 0 || sp.B % pp.sb != 0) return false;  // (a small level runs unsplit whatever the plan says)
    if (pp.k_tok_stride != sp.k_tok_stride || pp.v_tok_stride != sp.v_tok_stride) return false;
    if ((int64_t)sp.B * sp.Hkv * ((int64_t)pp.kv_len + sp.kv_len) > kSingleLaunchMaxKeys) return false;
    return u.gqa_any_rows;
}

bool levels_in_range(const hyd_decode_params* p) { return p->n_levels >= 0 && p->n_levels <= HYD_MAX_LEVELS; }

// Shapes only: the levels and the sizes, all that the size queries ask (they leave d->suffix unplanned); nothing without levels_in_range (each entry
// point has its own answer to that).  The prefix-only form plans its one pass with the default split cap, every other form shares the merge budget.
void plan_levels(const hyd_decode_params* p, DecodePlan* d) {
    const hyd_suffix_params& sp = p->suffix;
    memset(d, 0, offsetof(DecodePlan, suffix));
    if (!levels_in_range(p)) return;
    const bool prefix_only = p->n_levels == 1 && sp.kv_len == 0;
    d->two_stream_ok = p->n_levels > 0 && sp.kv_len > 0;
    // (a two-stream phase on prefix-only shapes is refused by the launch, and sized like the prefix-only form by the queries)
    d->form = (p->phase == HYD_PHASE_UNIQUE_PARTIAL || p->phase == HYD_PHASE_MERGE) ? kTwoStream : prefix_only ? kPrefixOnly : kInOrder;
    const int cap = prefix_only ? kMaxSplits : level_split_cap(p->n_levels);
    const size_t rows = (size_t)sp.B * sp.nq * sp.Hq;
    for (; d->n_planned < p->n_levels; ++d->n_planned) {
        LevelPlan& lv = d->level[d->n_planned];
        level_to_prefix(p, d->n_planned, &lv.pp);
        if ((d->rc = plan_prefix(&lv.pp, &lv.pl, cap))) return;
        if (prefix_only) {
            d->levels_bytes = prefix_ws_bytes(&lv.pp, lv.pl);
            continue;
        }
        lv.small = level_is_small(lv.pp, lv.pl);
        lv.count = (lv.pl.nsplit == 1 || lv.small) ? 1 : lv.pl.nsplit;
        lv.is_f32 = (lv.count > 1 || (p->f32_partials != 0 && !lv.small)) ? 1 : 0;
        lv.layout = slice_layout(rows, sp.D, lv.is_f32 ? 4 : 2, lv.count);
        d->levels_bytes += lv.layout.bytes;
        d->n_parts += lv.count;
    }
    if (d->two_stream_ok) d->unique = slice_layout(rows, sp.D, 2, 1);
}

// ... and the call's unique pass, planned once for every phase (kq: null, or fp8 unique caches).  Without unique keys it only merges:
// no fp8, no causal tail, no sequence lengths.
void plan_decode(const hyd_decode_params* p, const hyd_kv_quant* kq, DecodePlan* d) {
    const bool unique = p->suffix.kv_len > 0;
    plan_suffix(&p->suffix, unique ? kq : nullptr, unique && p->causal_tail != 0, &d->suffix);  // (first: plan_prefix's message, if any, stays the last)
    if (!unique) d->suffix.args.sl32 = nullptr, d->suffix.args.sl64 = nullptr;
    plan_levels(p, d);
    if (d->form == kInOrder && decode_runs_as_one_launch(p, d->level[0], d->suffix)) d->form = kOneLaunch;
}

int check_prefix_ptrs(const hyd_prefix_params* p) {
    if (int rc = check_ptrs_align({{p->q, "q"}, {p->k, "shared k"}, {p->v, "shared v"}})) return rc;
    return check_strides8({{p->k_group_stride, "k_group_stride"}, {p->k_tok_stride, "k_tok_stride"}, {p->k_head_stride, "k_head_stride"},
                           {p->v_group_stride, "v_group_stride"}, {p->v_tok_stride, "v_tok_stride"}, {p->v_head_stride, "v_head_stride"}});
}

}  // namespace

extern "C" {

int hyd_prefix_plan(const hyd_prefix_params* p, int32_t* num_splits, int32_t* grid, int32_t* split_len) {
    PrefixPlan pl;
    int rc = plan_prefix(p, &pl);
    if (rc) return rc;
    if (num_splits) *num_splits = pl.nsplit;
    if (grid) *grid = pl.grid;
    if (split_len) *split_len = pl.split_len;
    return HYD_OK;
}

size_t hyd_prefix_workspace_bytes(const hyd_prefix_params* p) {
    PrefixPlan pl;
    if (plan_prefix(p, &pl)) return 0;
    return prefix_ws_bytes(p, pl);
}

int hyd_prefix_attn_fwd(const hyd_prefix_params* p, void* stream) {
    PrefixPlan pl;
    int rc = plan_prefix(p, &pl);
    if (rc) return rc;
    if ((rc = check_prefix_ptrs(p))) return rc;
    if ((rc = check_ptr_align(p->out, "out"))) return rc;
    if (p->kv_len == 0) return fail(HYD_ERR_BAD_ARG, "kv_len == 0: attention over no keys is undefined");
    return run_prefix(p, pl, /*merge=*/true, static_cast<hipStream_t>(stream));
}

static int suffix_fwd(const hyd_suffix_params* p, const hyd_kv_quant* kq, bool causal, void* stream) {
    int rc = check_suffix(p);
    if (rc) return rc;
    if ((rc = check_kvq(&kq, p->dtype))) return rc;
    if (causal && (rc = check_causal_tail(p, kq))) return rc;
    if (p->n_partials < 0 || p->n_partials > HYD_MAX_LEVELS) return fail(HYD_ERR_BAD_ARG, "n_partials %d", p->n_partials);
    if (p->kv_len == 0 && p->n_partials == 0) return fail(HYD_ERR_BAD_ARG, "kv_len == 0 and no partials");
    SuffixPlan pl;  // (a causal call without unique keys drops its hyd_kv_quant, a plain one has always kept it)
    plan_suffix(p, causal && p->kv_len == 0 ? nullptr : kq, causal, &pl);
    return run_suffix(pl, p->partials, p->n_partials, static_cast<hipStream_t>(stream));
}

int hyd_suffix_attn_fwd_kvq(const hyd_suffix_params* p, const hyd_kv_quant* kq, void* stream) { return suffix_fwd(p, kq, false, stream); }
int hyd_suffix_attn_fwd(const hyd_suffix_params* p, void* stream) { return suffix_fwd(p, nullptr, false, stream); }
int hyd_suffix_attn_causal_fwd_kvq(const hyd_suffix_params* p, const hyd_kv_quant* kq, void* stream) { return suffix_fwd(p, kq, true, stream); }
int hyd_suffix_attn_causal_fwd(const hyd_suffix_params* p, void* stream) { return suffix_fwd(p, nullptr, true, stream); }

int hyd_kv_quant_supported(const hyd_suffix_params* p, const hyd_kv_quant* kq) {
    if (!p) return 0;
    const KvqKind kind = kvq_kind(kq, p->dtype);
    if (kind != kKvqFp8) return kind == kKvqNone ? 1 : 0;
    SuffixPlan pl;
    plan_suffix(p, kq, /*causal=*/false, &pl);
    return pl.valid && !narrow_kv_dim(p) && pl.fp8_native ? 1 : 0;  // (a narrow kv_dim answers 0 here even where no key is read)
}

int hyd_narrow_kv_supported(const hyd_suffix_params* p) {
    if (!p) return 0;
    SuffixPlan pl;
    plan_suffix(p, nullptr, /*causal=*/false, &pl);
    if (!pl.narrow) return pl.valid && p->kv_len >= 0 ? 1 : 0;  // nothing narrow is read: the existing call
    return pl.narrow_native ? 1 : 0;
}

int hyd_combine_lse(const void* const* outs, const float* const* lses, int32_t n, int64_t rows, int32_t D,
                    int32_t dtype, void* out, float* out_lse, void* stream) {
    if (!outs || !lses || !out) return fail(HYD_ERR_BAD_ARG, "null pointer");
    if (n <= 0 || n > kMaxCombine) return fail(HYD_ERR_UNSUPPORTED, "n = %d partials (1..%d supported)", n, kMaxCombine);
    if (rows < 0 || D <= 0) return fail(HYD_ERR_BAD_ARG, "rows %lld D %d", (long long)rows, D);
    if (dtype != HYD_F16 && dtype != HYD_BF16 && dtype != HYD_F32) return fail(HYD_ERR_UNSUPPORTED, "dtype %d", dtype);
    CombineArgs c;
    memset(&c, 0, sizeof(c));
    bool aligned = !misaligned(out, 16);
    for (int i = 0; i < n; ++i) {
        if (!outs[i] || !lses[i]) return fail(HYD_ERR_BAD_ARG, "partial %d is null", i);
        c.outs[i] = outs[i];
        c.lses[i] = lses[i];
        aligned = aligned && !misaligned(outs[i], 16);
    }
    c.n = n;
    c.rows = rows;
    c.D = D;
    c.dtype_in = dtype;
    c.dtype_out = dtype;
    c.out = out;
    c.out_lse = out_lse;
    c.lse_layout = HYD_LSE_BQH;
    c.scalar_only = aligned ? 0 : 1;  // unaligned views take the element-wise kernel
    return launched(launch_combine(c, static_cast<hipStream_t>(stream)), "combine kernel launch");
}

size_t hyd_decode_workspace_bytes(const hyd_decode_params* p) {
    if (!p || !levels_in_range(p)) return 0;
    DecodePlan d;
    plan_levels(p, &d);
    return d.rc ? 0 : d.levels_bytes + d.unique.bytes;  // (the unique partial counts in every phase: one size for the whole call)
}

size_t hyd_workspace_bytes(int32_t B, int32_t nq, int32_t Hq, int32_t Hkv, int32_t D, int32_t n_levels,
                           const int32_t* level_sb, const int32_t* level_kv_len) {
    if (n_levels < 0 || n_levels > HYD_MAX_LEVELS) return 0;
    hyd_decode_params p;
    memset(&p, 0, sizeof(p));
    p.suffix.dtype = HYD_BF16;
    p.suffix.B = B;
    p.suffix.nq = nq;
    p.suffix.Hq = Hq;
    p.suffix.Hkv = Hkv;
    p.suffix.D = D;
    p.suffix.kv_len = 1;  // a decode step has unique keys: size the unique partial of the two-stream form as well
    p.f32_partials = 1;   // an upper bound for every form of the call: an unsplit level's partial may be kept in fp32
    p.n_levels = n_levels;
    for (int i = 0; i < n_levels; ++i) {
        p.levels[i].sb = level_sb[i];
        p.levels[i].kv_len = level_kv_len[i];
    }
    return hyd_decode_workspace_bytes(&p);
}

// Shapes only: a grouped-query fp8 call whose 16-bit twin would run as ONE launch (decode_runs_as_one_launch).  The one-launch walk
// does not round a 16-bit prefix partial, the two-kernel pair does: the pair is not what the caller's 16-bit results are, so such a call is
// refused instead of quietly run as the pair.  (Hq == Hkv shapes keep ignoring the flag; a level that does not plan: decode_impl reports it.)
static bool decode_kvq_is_one_launch(const DecodePlan& d) { return d.suffix.fp8_gqa && d.form == kOneLaunch; }

int hyd_decode_kv_quant_supported(const hyd_decode_params* p, const hyd_kv_quant* kq) {
    if (!p) return 0;
    const KvqKind kind = kvq_kind(kq, p->suffix.dtype);
    if (kind != kKvqFp8) return kind == kKvqNone ? 1 : 0;
    if (!levels_in_range(p)) return 0;
    if (p->suffix.kv_len <= 0) return p->suffix.kv_len == 0 ? 1 : 0;  // no unique key is read: the existing path
    DecodePlan d;
    plan_decode(p, kq, &d);
    if (!d.suffix.valid) return 0;
    // the causal tail: the launch's own rules (check_causal_tail, then the fp8 causal kernel's shapes)
    if (p->causal_tail != 0) return p->causal_tail == 1 && !check_causal_tail(&p->suffix, kq) && d.suffix.causal_native ? 1 : 0;
    return d.suffix.fp8_native && !decode_kvq_is_one_launch(d) ? 1 : 0;
}

// kq: null, or fp8 unique caches that are read (kv_len > 0), validated with the suffix block by hyd_decode_attn_fused_kvq.  Such a call is
// never the one-launch form: Hq == Hkv shapes ignore single_launch_small, grouped-query ones are refused where the flag would have applied.
static int decode_impl(const hyd_decode_params* p, const hyd_kv_quant* kq, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    const hyd_suffix_params& sp = p->suffix;
    const bool causal = p->causal_tail != 0;
    DecodePlan d;  // the one plan of the call: every check below and every phase reads it
    plan_decode(p, kq, &d);
    const SuffixPlan& u = d.suffix;
    if (kq) {
        // fp8 unique caches: judged up front, in every phase, so that the phases of one call agree.  A causal call that takes the fp8 causal
        // kernel (HYD_KVQ_CAUSAL) is judged by that kernel's shapes, below, behind the checks of causal_tail itself
        if (u.narrow) return fail_narrow_fp8();
        if (!(causal && kvq_takes_causal(kq)) && !u.fp8_native) return fail_kvq_shapes(sp.D);
        if (decode_kvq_is_one_launch(d))
            return fail(HYD_ERR_UNSUPPORTED, "fp8 unique caches: a grouped-query call this small runs as ONE launch with 16-bit caches "
                                             "(single_launch_small), which has no fp8 form: clear the flag, or pass 16-bit caches");
    }
    if (!levels_in_range(p)) return fail(HYD_ERR_BAD_ARG, "n_levels %d", p->n_levels);
    if (p->phase < HYD_PHASE_ALL || p->phase > HYD_PHASE_MERGE) return fail(HYD_ERR_BAD_ARG, "phase %d", p->phase);
    if (p->shared_max_workgroups < 0) return fail(HYD_ERR_BAD_ARG, "shared_max_workgroups %d", p->shared_max_workgroups);
    if (p->f32_partials != 0 && p->f32_partials != 1) return fail(HYD_ERR_BAD_ARG, "f32_partials %d", p->f32_partials);
    int rc = check_suffix(&sp);
    if (rc) return rc;
    if (p->n_levels == 0 && sp.kv_len == 0) return fail(HYD_ERR_BAD_ARG, "no shared levels and no unique keys");
    if (u.narrow && !u.narrow_native) return fail_narrow_shapes(sp.kv_dim, sp.D);  // before the first launch, in every phase: the phases agree
    if (p->causal_tail != 0 && p->causal_tail != 1) return fail(HYD_ERR_BAD_ARG, "causal_tail %d", p->causal_tail);
    if (causal && (rc = check_causal_tail(&sp, kq))) return rc;
    if (u.causal && !u.causal_native) return fail_causal_shapes();  // (u.causal: the causal tail over unique keys)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rows = (size_t)sp.B * sp.nq * sp.Hq;
    const bool do_shared = p->phase == HYD_PHASE_ALL || p->phase == HYD_PHASE_SHARED;
    const bool do_unique = p->phase == HYD_PHASE_ALL || p->phase == HYD_PHASE_UNIQUE;
    // The two-stream form needs both a shared and a unique part; without one of them the in-order phases already are
    // the whole operator (the caller asks hyd_decode_two_stream_ok first).
    if (d.form == kTwoStream && !d.two_stream_ok)
        return fail(HYD_ERR_UNSUPPORTED, "two-stream phases need at least one shared level and unique keys");
    if (d.form == kPrefixOnly && !do_shared) return HYD_OK;  // nothing left for the unique phase

    // ---- validate everything before the first launch: the levels in order, each one's plan before its pointers -----------
    for (int i = 0; i < d.n_planned; ++i) {
        if ((rc = check_prefix_ptrs(&d.level[i].pp))) return rc;
        if (d.level[i].pp.kv_len == 0) return fail(HYD_ERR_BAD_ARG, "level %d has kv_len == 0", i);
    }
    if (d.rc) return d.rc;  // level n_planned did not plan: nothing above failed, so g_err still holds plan_prefix's message
    if (d.form == kPrefixOnly) {
        hyd_prefix_params pp = d.level[0].pp;
        pp.out = sp.out;
        pp.lse = nullptr;
        pp.workspace = p->workspace;
        pp.workspace_bytes = p->workspace_bytes;
        return run_prefix(&pp, d.level[0].pl, true, s, p->shared_max_workgroups);
    }
    const bool two_stream = d.form == kTwoStream;
    if (d.n_parts + (two_stream ? 1 : 0) > kMaxCombine) return fail(HYD_ERR_UNSUPPORTED, "%d partials (more than %d)", d.n_parts, kMaxCombine);
    if (d.form == kOneLaunch && !kq) {
        // launch latency, not work: the grouped-query kernel walks the group's shared keys, then the sequence's own
        const hyd_prefix_params& pp = d.level[0].pp;
        SuffixArgs& a = d.suffix.args;  // (the planned arguments, plus the shared segment)
        a.pk = pp.k; a.pv = pp.v;
        a.pk_gs = pp.k_group_stride; a.pk_hs = pp.k_head_stride;
        a.pv_gs = pp.v_group_stride; a.pv_hs = pp.v_head_stride;
        a.p_len = pp.kv_len; a.p_per = sp.B / pp.sb;
        a.shared_kv = 1;  // p_per sequences read the same prefix keys: default cache policy, not the read-once hint
        return launched(launch_suffix_gqa(a, sp.dtype, sp.D, s), "single-launch decode kernel");
    }
    const size_t need = d.levels_bytes + (two_stream ? d.unique.bytes : 0);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need))
        return fail(HYD_ERR_WORKSPACE, "decode needs %zu workspace bytes, got %zu", need, p->workspace_bytes);
    // what the unique pass of this call would refuse by its shapes: known now, so said before the level passes go out
    if ((do_unique || p->phase == HYD_PHASE_UNIQUE_PARTIAL) && (rc = check_suffix_limits(u))) return rc;

    hyd_partial parts[HYD_MAX_LEVELS];
    char* ws = static_cast<char*>(p->workspace);
    for (int i = 0; i < p->n_levels; ++i) {
        const LevelPlan& lv = d.level[i];
        float* lse = reinterpret_cast<float*>(ws + lv.layout.lse_base);
        parts[i] = {ws, lse, lv.count, lv.is_f32};
        if (do_shared) {
            hyd_prefix_params pp = lv.pp;
            if (lv.count == 1) {
                pp.out = ws;
                pp.lse = lse;
            } else {
                pp.workspace = ws;
                pp.workspace_bytes = lv.layout.bytes;
            }
            if (lv.small) rc = run_level_small(pp, lv.pl, ws, lse, s);
            else rc = run_prefix(&pp, lv.pl, /*merge=*/false, s, p->shared_max_workgroups, lv.is_f32 != 0);
            if (rc) return rc;
        }
        ws += lv.layout.bytes;
    }
    if (two_stream) {
        // the unique pass's partial lives behind the levels' regions
        char* u_out = static_cast<char*>(p->workspace) + d.levels_bytes;
        float* u_lse = reinterpret_cast<float*>(u_out + d.unique.lse_base);
        if (p->phase == HYD_PHASE_UNIQUE_PARTIAL) {
            d.suffix.args.out = u_out;
            d.suffix.args.lse = u_lse;
            return run_suffix(u, nullptr, 0, s);
        }
        CombineArgs c;  // HYD_PHASE_MERGE: every level's partial(s) + the unique partial -> out
        memset(&c, 0, sizeof(c));
        int n = 0;
        if ((rc = for_each_slice(parts, p->n_levels, rows, sp.D, &n, [&c](int i, const void* out, const float* lse, int is_f32) {
                c.outs[i] = out;
                c.lses[i] = lse;
                if (is_f32) c.f32_mask |= 1ull << i;
            })))
            return rc;
        c.outs[n] = u_out;
        c.lses[n] = u_lse;
        c.n = n + 1;
        c.rows = (int64_t)rows;
        c.D = sp.D;
        c.dtype_in = c.f32_mask ? HYD_MIXED : sp.dtype;
        c.dtype_out = sp.dtype;
        c.out = sp.out;
        c.lse_layout = HYD_LSE_BQH;
        return launched(launch_combine(c, s), "combine kernel launch");
    }
    if (!do_unique) return HYD_OK;
    // (several levels and no unique keys: the plan is the merge-only pass, whose suffix contributes lse = -inf)
    return run_suffix(u, parts, p->n_levels, s);
}

int hyd_decode_attn_fused(const hyd_decode_params* p, void* stream) { return decode_impl(p, nullptr, stream); }

int hyd_decode_attn_fused_kvq(const hyd_decode_params* p, const hyd_kv_quant* kq, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_suffix(&p->suffix);
    if (rc) return rc;
    if ((rc = check_kvq(&kq, p->suffix.dtype))) return rc;
    return decode_impl(p, p->suffix.kv_len > 0 ? kq : nullptr, stream);  // kv_len == 0 reads no unique key and takes the existing path
}

int hyd_decode_two_stream_ok(const hyd_decode_params* p) {
    if (!p || !levels_in_range(p)) return 0;
    DecodePlan d;
    plan_levels(p, &d);
    return d.two_stream_ok ? 1 : 0;
}

}  // extern "C"
