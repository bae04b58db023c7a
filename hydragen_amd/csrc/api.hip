// C ABI of libhydragen_hip.so (see include/hydragen_hip.h): argument validation, shapes-only launch
// planning, workspace carving.  No allocation, no synchronisation, no device reads on the host.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>

#include "hyd_kernels.h"

using namespace hyd;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// what a launcher returned -> HYD_OK, or HYD_ERR_LAUNCH with "<what> failed: hip error <rc>"
int launched(int rc, const char* what) { return rc ? fail(HYD_ERR_LAUNCH, "%s failed: hip error %d", what, rc) : HYD_OK; }

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

int check_scale(float s) {
    if (!(s >= 0.f) || s > 1.0e4f) return fail(HYD_ERR_BAD_ARG, "softmax_scale %g (0 = head_dim^-0.5, or a positive finite scale)", (double)s);
    return HYD_OK;
}

int check_common(int dtype, int B, int nq, int Hq, int Hkv, int D) {
    if (dtype != HYD_F16 && dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d: only f16/bf16", dtype);
    if (D != 64 && D != 128 && D != 256) return fail(HYD_ERR_UNSUPPORTED, "head_dim %d: only 64, 128 and 256 are implemented", D);
    if (B <= 0 || nq <= 0 || Hq <= 0 || Hkv <= 0) return fail(HYD_ERR_BAD_ARG, "non-positive size B=%d nq=%d Hq=%d Hkv=%d", B, nq, Hq, Hkv);
    if (Hq % Hkv != 0) return fail(HYD_ERR_BAD_ARG, "qheads %d not divisible by kvheads %d", Hq, Hkv);
    return HYD_OK;
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
    a->q = p->q;
    a->k = p->k;
    a->v = p->v;
    a->cu_k = p->cu_seqlens_k;
    a->cu_q = p->cu_seqlens_q;
    a->k_gs = p->k_group_stride;
    a->k_ts = p->k_tok_stride;
    a->k_hs = p->k_head_stride;
    a->v_gs = p->v_group_stride;
    a->v_ts = p->v_tok_stride;
    a->v_hs = p->v_head_stride;
    a->B = p->B;
    a->nq = p->nq;
    a->Hq = p->Hq;
    a->Hkv = p->Hkv;
    a->g = pl.g;
    a->sb = p->sb;
    a->per = pl.per;
    a->kv_len = p->kv_len;
    a->row_blocks = pl.row_blocks;
    a->wg_rows = pl.wg_rows;
    // Two waves per SIMD (8-wave workgroups of 32-row waves) wherever that unit is built: D = 128, one workgroup per unit
    // (persistent launches keep the 4-wave unit: launch_prefix_w64_t).  Same rows per workgroup, rings and results; fewer
    // cycles (the SIMD issues one wave's VALU / LDS / DMA instructions beside the other's MFMAs), the same energy: 10 %
    // faster where the pass is short (P = 128: 9.8 against 11.0 us), equal where the chip runs at its power limit.
    {
        const int force_waves = dev_switch("HYD_PREFIX_WAVES");  // 0 in product builds
        a->waves = (p->D == 128 && force_waves != 4) ? 8 : 4;
    }
    a->nsplit = pl.nsplit;
    a->split_len = pl.split_len;
    a->vgrid = pl.grid;
    a->lse_q_stride = pl.qpg;
    a->scale_log2e = scale_log2e_of(p->softmax_scale, p->D);
    a->div_row_blocks = make_fastdiv((uint32_t)pl.row_blocks);
    a->div_nsplit = make_fastdiv((uint32_t)pl.nsplit);
    a->div_hkv = make_fastdiv((uint32_t)p->Hkv);
    a->div_g = make_fastdiv((uint32_t)pl.g);
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

bool misaligned(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(to - 1)) != 0; }  // (null is aligned)

int check_ptr_align(const void* p, const char* name) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "%s is null", name);
    if (misaligned(p, 16)) return fail(HYD_ERR_BAD_ARG, "%s must be 16-byte aligned", name);
    return HYD_OK;
}
int check_stride8(int64_t s, const char* name) {
    if (s % 8 != 0) return fail(HYD_ERR_BAD_ARG, "%s (%lld) must be a multiple of 8 elements", name, (long long)s);
    return HYD_OK;
}

// Narrow rows (hyd_suffix_params.kv_dim, hyd_rope_params.head_dim): 0 or D = rows of D elements; else 16 <= n < D, n % 16 == 0.
int check_narrow_dim(int n, int D, const char* field) {
    if (n == 0 || n == D) return HYD_OK;
    if (n < 16 || n > D || n % 16 != 0)
        return fail(HYD_ERR_BAD_ARG, "%s %d: 0 or %d (rows of D elements), or a multiple of 16 in [16, %d)", field, n, D, D);
    return HYD_OK;
}
// the elements per head of the unique cache rows when they are narrower than D, else 0
int narrow_kv_dim(const hyd_suffix_params* p) { return p->kv_dim != p->D ? p->kv_dim : 0; }
// the softmax scale of a call: the caller's, else that of the TRUE head dim (kv_dim when the unique rows are narrow)
float true_dim_scale(const hyd_suffix_params* p) {
    if (p->softmax_scale > 0.f || !narrow_kv_dim(p)) return p->softmax_scale;
    return (float)(1.0 / sqrt((double)p->kv_dim));
}

int check_suffix(const hyd_suffix_params* p, bool need_kv) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D);
    if (!rc) rc = check_scale(p->softmax_scale);
    if (!rc) rc = check_narrow_dim(p->kv_dim, p->D, "kv_dim");
    if (rc) return rc;
    if (p->kv_len < 0) return fail(HYD_ERR_BAD_ARG, "kv_len %d", p->kv_len);
    if ((rc = check_ptr_align(p->q, "q"))) return rc;
    if ((rc = check_ptr_align(p->out, "out"))) return rc;
    if (need_kv && p->kv_len > 0) {
        if ((rc = check_ptr_align(p->k, "k"))) return rc;
        if ((rc = check_ptr_align(p->v, "v"))) return rc;
        if ((rc = check_stride8(p->k_batch_stride, "k_batch_stride")) || (rc = check_stride8(p->k_tok_stride, "k_tok_stride")) ||
            (rc = check_stride8(p->k_head_stride, "k_head_stride")) || (rc = check_stride8(p->v_batch_stride, "v_batch_stride")) ||
            (rc = check_stride8(p->v_tok_stride, "v_tok_stride")) || (rc = check_stride8(p->v_head_stride, "v_head_stride")))
            return rc;
    }
    return HYD_OK;
}

void fill_suffix_args(const hyd_suffix_params* p, SuffixArgs* ap) {
    SuffixArgs& a = *ap;
    memset(&a, 0, sizeof(a));
    a.q = p->q;
    a.k = p->k;
    a.v = p->v;
    a.out = p->out;
    a.lse = p->lse;
    a.sl32 = p->seq_lens_i32;
    a.sl64 = p->seq_lens_i64;
    a.order = p->seq_order;
    a.k_bs = p->k_batch_stride;
    a.k_ts = p->k_tok_stride;
    a.k_hs = p->k_head_stride;
    a.v_bs = p->v_batch_stride;
    a.v_ts = p->v_tok_stride;
    a.v_hs = p->v_head_stride;
    a.B = p->B;
    a.nq = p->nq;
    a.Hq = p->Hq;
    a.Hkv = p->Hkv;
    a.g = p->Hq / p->Hkv;
    a.kv_len = p->kv_len;
    a.rows = p->nq * a.g;
    a.units = p->B * p->Hkv;
    a.scale_log2e = scale_log2e_of(true_dim_scale(p), p->D);
    a.kv_dim = p->kv_len > 0 ? narrow_kv_dim(p) : 0;  // (no unique key, nothing narrow to read: the merge-only call of the D-wide kernels)
}

int fail_narrow_fp8() { return fail(HYD_ERR_UNSUPPORTED, "kv_dim / head_dim with fp8 caches: narrow rows are implemented for 16-bit caches only"); }
int fail_narrow_shapes(const hyd_suffix_params* p) {
    return fail(HYD_ERR_UNSUPPORTED, "kv_dim %d: narrow unique caches run on the token-row kernel only (nq == 1, Hq == Hkv, Hkv a multiple of %d at D = %d, "
                                     "a sequence's cache within 2 GiB)", p->kv_dim, 64 / (p->D / 8), p->D);
}
// shapes only: a narrow call (kv_dim set, unique keys present) the narrow token-row kernel takes
bool narrow_native(const hyd_suffix_params* p) {
    SuffixArgs a;
    fill_suffix_args(p, &a);
    return suffix_narrow_eligible(a, p->D);
}

// HYD_KVQ_GQA: the caller takes the grouped-query fp8 kernel; without it the entry points keep the shapes of ABI 0.5.0 as first
// released (callers of that time route refused shapes to a fallback of their own, and go on doing so)
bool kvq_takes_gqa(const hyd_kv_quant* kq) { return kq && (kq->flags & HYD_KVQ_GQA) != 0; }

int fail_kvq_shapes(int D) {
    return fail(HYD_ERR_UNSUPPORTED,
                "fp8 unique caches: shapes not native (grouped-query units of nq * Hq / Hkv >= 3 rows with hyd_kv_quant.flags & HYD_KVQ_GQA, or nq == 1, Hq == Hkv with Hkv a "
                "multiple of %d at D = %d; D 64 / 128 / 256)", D >= 8 ? 64 / (D / 8) : 0, D);
}

// The causal tail (hyd_suffix_attn_causal_fwd, hyd_decode_params.causal_tail): 2..8 query tokens, 16-bit caches with rows of D elements.
int check_causal_tail(const hyd_suffix_params* p, const hyd_kv_quant* kq) {
    if (p->nq < 2 || p->nq > 8) return fail(HYD_ERR_BAD_ARG, "causal tail: nq = %d query tokens per sequence, 2 to 8 are taken", p->nq);
    if (kq) return fail(HYD_ERR_UNSUPPORTED, "causal tail with fp8 unique caches: implemented for 16-bit caches only");
    if (p->kv_len > 0 && narrow_kv_dim(p)) return fail(HYD_ERR_UNSUPPORTED, "causal tail with kv_dim %d: narrow unique rows run on the token-row kernel, which has no causal form", p->kv_dim);
    return HYD_OK;
}

int fail_causal_shapes() { return fail(HYD_ERR_UNSUPPORTED, "causal tail: no kernel with the per-row key limit takes these shapes"); }

// kq: null, or fp8 unique caches (validated by check_kvq; K/V strides in bytes).  causal: the causal tail (check_causal_tail passed) --
// such a call goes to launch_suffix_causal or fails, never to a kernel without the per-row key limit.
int run_suffix(const hyd_suffix_params* p, const hyd_partial* parts, int n_parts, hipStream_t s, const hyd_kv_quant* kq = nullptr, bool causal = false) {
    SuffixArgs a;
    fill_suffix_args(p, &a);
    int rc = for_each_slice(parts, n_parts, (size_t)p->B * p->nq * p->Hq, p->D, &a.n_partials, [&a](int n, const void* out, const float* lse, int is_f32) {
        a.partials[n].out = out;
        a.partials[n].lse = lse;
        a.partials[n].is_f32 = is_f32;
    });
    if (rc) return rc;
    a.n_pre = 0;
    while (a.n_pre < 2 && a.n_pre < a.n_partials && !a.partials[a.n_pre].is_f32) ++a.n_pre;
    const int64_t esz = kq ? 1 : 2;
    if ((int64_t)p->kv_len * p->k_tok_stride * esz >= (1ll << 31) || (int64_t)p->kv_len * p->v_tok_stride * esz >= (1ll << 31))
        return fail(HYD_ERR_UNSUPPORTED, "unique K/V of one sequence spans >= 2 GiB (32-bit in-sequence offsets)");
    if (p->Hkv > 4 * 65535 || a.rows > 8 * 65535) return fail(HYD_ERR_UNSUPPORTED, "too many kv heads / query rows for the suffix grid");
    if (causal) {
        if (kq || !suffix_causal_eligible(a, p->D)) return fail_causal_shapes();
        return launched(launch_suffix_causal(a, p->dtype, p->D, s), "causal-tail suffix kernel launch");
    }
    if (a.kv_dim) {
        if (kq) return fail_narrow_fp8();
        if (!suffix_narrow_eligible(a, p->D)) return fail_narrow_shapes(p);
    }
    if (kq) {
        // the 16-bit launcher's order: grouped-query shapes to the matrix-core kernel, one-row units to the token-row kernel
        const bool gqa = kvq_takes_gqa(kq) && suffix_gqa_fp8_eligible(a, p->D);
        if (!gqa && !suffix_fp8_eligible(a, p->D)) return fail_kvq_shapes(p->D);
        SuffixKvqArgs ka;
        ka.k_scale = kq->k_scale;
        ka.v_scale = kq->v_scale;
        ka.a = a;
        return launched(gqa ? launch_suffix_gqa_fp8(ka, p->dtype, p->D, s) : launch_suffix_fp8(ka, p->dtype, p->D, s), "fp8 suffix kernel launch");
    }
    return launched(launch_suffix(a, p->dtype, p->D, s), "suffix kernel launch");
}

// What a hyd_kv_quant asks of a call whose q dtype is `dtype`: nothing (absent, or the q dtype), e4m3fn caches, or a dtype nobody has.
enum KvqKind { kKvqNone, kKvqFp8, kKvqUnsupported };
KvqKind kvq_kind(const hyd_kv_quant* kq, int dtype) {
    if (!kq || kq->kv_dtype == dtype) return kKvqNone;
    return kq->kv_dtype == HYD_FP8_E4M3 ? kKvqFp8 : kKvqUnsupported;
}

// Validates *kq and narrows it to what the launch paths take: null, or fp8 unique caches.
int check_kvq(const hyd_kv_quant** kq, int dtype) {
    const KvqKind kind = kvq_kind(*kq, dtype);
    if (kind == kKvqUnsupported)
        return fail(HYD_ERR_UNSUPPORTED, "kv_dtype %d: HYD_FP8_E4M3 (%d) or the q dtype (%d)", (*kq)->kv_dtype, HYD_FP8_E4M3, dtype);
    if (kind == kKvqNone) {
        *kq = nullptr;
        return HYD_OK;
    }
    if (misaligned((*kq)->k_scale, 4) || misaligned((*kq)->v_scale, 4))
        return fail(HYD_ERR_BAD_ARG, "k_scale / v_scale must be 4-byte aligned fp32 arrays");
    return HYD_OK;
}

// shapes-only: does an fp8 suffix kernel take these shapes (nothing is launched, no device memory read)
bool kvq_native(const hyd_suffix_params* p, const hyd_kv_quant* kq) {
    if (check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D) || narrow_kv_dim(p)) return false;
    SuffixArgs a;
    fill_suffix_args(p, &a);
    return (kvq_takes_gqa(kq) && suffix_gqa_fp8_eligible(a, p->D)) || suffix_fp8_eligible(a, p->D);
}
// ... and is it the grouped-query kernel that takes them (the one whose 16-bit twin tiny decode calls fold into one launch)
bool kvq_native_gqa(const hyd_suffix_params* p, const hyd_kv_quant* kq) {
    if (!kvq_takes_gqa(kq) || check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D)) return false;
    SuffixArgs a;
    fill_suffix_args(p, &a);
    return suffix_gqa_fp8_eligible(a, p->D);
}

void level_to_prefix(const hyd_decode_params* p, int i, hyd_prefix_params* pp) {
    const hyd_suffix_params& s = p->suffix;
    const hyd_level& lv = p->levels[i];
    memset(pp, 0, sizeof(*pp));
    pp->q = s.q;
    pp->k = lv.k;
    pp->v = lv.v;
    pp->cu_seqlens_k = lv.cu_seqlens_k;
    pp->k_group_stride = lv.k_group_stride;
    pp->k_tok_stride = lv.k_tok_stride;
    pp->k_head_stride = lv.k_head_stride;
    pp->v_group_stride = lv.v_group_stride;
    pp->v_tok_stride = lv.v_tok_stride;
    pp->v_head_stride = lv.v_head_stride;
    pp->dtype = s.dtype;
    pp->B = s.B;
    pp->nq = s.nq;
    pp->Hq = s.Hq;
    pp->Hkv = s.Hkv;
    pp->D = s.D;
    pp->softmax_scale = true_dim_scale(&s);
    pp->sb = lv.sb;
    pp->kv_len = lv.kv_len;
    pp->causal = 0;
    pp->lse_layout = HYD_LSE_BQH;
    pp->num_splits = 0;
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
// launch all read a DecodePlan and plan nothing of their own, so they cannot disagree.
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
};

// hyd_decode_params.single_launch_small: one uniform shared level that already counts as small (few query rows per
// (group, kv head), short prefix), unique keys present, the same token strides in the shared and the unique tensors, and
// so few keys in all that the call is launch latency.  Measured per graph-replayed call (tests/probes/single_launch_probe.py,
// units x keys = B * Hkv * (P + S)): 1152 keys (BASELINE config 1) 6.8 -> 4.1 us, 2176 keys 11.4 -> 8.1, 8072 keys (two
// sequences on a 1000-key prefix) 19.5 -> 16.5, 8704 keys (32 sequences) 14.0 -> 14.1: even.  Shapes only: capture-safe.
constexpr int64_t kSingleLaunchMaxKeys = 8192;
bool decode_runs_as_one_launch(const hyd_decode_params* p, const LevelPlan& lv) {
    const hyd_suffix_params& sp = p->suffix;
    if (p->phase != HYD_PHASE_ALL || !p->single_launch_small || p->n_levels != 1 || !lv.small || sp.kv_len <= 0) return false;
    if (p->causal_tail) return false;  // the walk over both segments has no per-row key limit: the pair of launches runs
    if (narrow_kv_dim(&sp)) return false;  // narrow unique caches: the pair of launches runs (the rule Hq == Hkv fp8 calls have)
    if (sp.lse) return false;  // suffix.lse is the LSE of the unique keys alone in every form; one walk over both segments cannot give it
    const hyd_prefix_params& pp = lv.pp;
    if (pp.cu_seqlens_k || pp.sb <= 0 || sp.B % pp.sb != 0) return false;  // (a small level runs unsplit whatever the plan says)
    if (pp.k_tok_stride != sp.k_tok_stride || pp.v_tok_stride != sp.v_tok_stride) return false;
    if ((int64_t)sp.B * sp.Hkv * ((int64_t)pp.kv_len + sp.kv_len) > kSingleLaunchMaxKeys) return false;
    SuffixArgs a;
    fill_suffix_args(&sp, &a);
    return suffix_gqa_eligible(a, sp.D, /*any_shape=*/true);
}

bool levels_in_range(const hyd_decode_params* p) { return p->n_levels >= 0 && p->n_levels <= HYD_MAX_LEVELS; }

// Shapes only.  The caller has checked levels_in_range (each entry point has its own answer to that).  The prefix-only form
// plans its one pass with the default split cap, every other form shares the merge budget among its levels.
void plan_decode(const hyd_decode_params* p, DecodePlan* d) {
    const hyd_suffix_params& sp = p->suffix;
    memset(d, 0, sizeof(*d));
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
    if (d->form == kInOrder && decode_runs_as_one_launch(p, d->level[0])) d->form = kOneLaunch;
}

int check_prefix_ptrs(const hyd_prefix_params* p) {
    int rc;
    if ((rc = check_ptr_align(p->q, "q"))) return rc;
    if ((rc = check_ptr_align(p->k, "shared k"))) return rc;
    if ((rc = check_ptr_align(p->v, "shared v"))) return rc;
    if ((rc = check_stride8(p->k_group_stride, "k_group_stride")) || (rc = check_stride8(p->k_tok_stride, "k_tok_stride")) ||
        (rc = check_stride8(p->k_head_stride, "k_head_stride")) || (rc = check_stride8(p->v_group_stride, "v_group_stride")) ||
        (rc = check_stride8(p->v_tok_stride, "v_tok_stride")) || (rc = check_stride8(p->v_head_stride, "v_head_stride")))
        return rc;
    return HYD_OK;
}

// ---- the logits entry points (hyd_sample_tokens, _filtered, _penalized, hyd_token_logprobs) ------------------------------------------
int logits_esz(int dtype) { return dtype == HYD_F32 ? 4 : 2; }

// The header of every [rows, n] logits call: dtype, row count, row length (max_n = 0: unbounded)
int check_logits_rows(int dtype, int64_t rows, int n, int max_n) {
    if (dtype != HYD_F16 && dtype != HYD_BF16 && dtype != HYD_F32) return fail(HYD_ERR_UNSUPPORTED, "dtype %d", dtype);
    if (rows < 0 || rows > (1LL << 31) || n <= 0) return fail(HYD_ERR_BAD_ARG, "rows %lld, n %d", (long long)rows, n);
    if (max_n && n > max_n) return fail(HYD_ERR_UNSUPPORTED, "n %d: rows of up to %d logits", n, max_n);
    return HYD_OK;
}
int check_row_stride(int64_t row_stride, int n) {
    return row_stride < n ? fail(HYD_ERR_BAD_ARG, "row_stride %lld < n %d", (long long)row_stride, n) : HYD_OK;
}
// 16-byte loads of a row: the base aligned and the row stride a multiple of `per16` elements
int logits_vec_ok(const void* logits, int64_t row_stride, int per16) { return (!misaligned(logits, 16) && row_stride % per16 == 0) ? 1 : 0; }

// What hyd_sample_tokens_filtered checks up to the row stride; the penalised sampler's parameters start with the same fields.
template <typename P>
int check_filter(const P* p) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    const int rc = check_logits_rows(p->dtype, p->rows, p->n, HYD_SAMPLE_FILTER_MAX_N);
    if (rc) return rc;
    if (!p->logits || !p->out) return fail(HYD_ERR_BAD_ARG, "logits / out is null");
    if (!(p->temperature >= 0.f)) return fail(HYD_ERR_BAD_ARG, "temperature %g must be >= 0", (double)p->temperature);
    if (p->top_k < 0) return fail(HYD_ERR_BAD_ARG, "top_k %d must be >= 0 (0 = off)", p->top_k);
    if (!(p->top_p > 0.f && p->top_p <= 1.f)) return fail(HYD_ERR_BAD_ARG, "top_p %g must be in (0, 1] (1 = off)", (double)p->top_p);
    if (!(p->min_p >= 0.f && p->min_p <= 1.f)) return fail(HYD_ERR_BAD_ARG, "min_p %g must be in [0, 1] (0 = off)", (double)p->min_p);
    return check_row_stride(p->row_stride, p->n);
}
// ... and its last check, the alignment of the four row tensors, with the argument block of the filtered draw
template <typename P>
int fill_filter_args(const P* p, FilterArgs* a) {
    const int esz = logits_esz(p->dtype);
    if (misaligned(p->logits, esz) || misaligned(p->out, 8) || misaligned(p->logprobs, 4) || misaligned(p->kept, 4))
        return fail(HYD_ERR_BAD_ARG, "logits / out / logprobs / kept is not aligned to its element size");
    memset(a, 0, sizeof(*a));
    a->logits = p->logits; a->out = p->out; a->logprobs = p->logprobs; a->kept = p->kept;
    a->row_stride = p->row_stride; a->seed = p->seed; a->offset = p->offset;
    a->rows = p->rows; a->n = p->n;
    a->inv_temperature = p->temperature > 0.f ? 1.0f / p->temperature : 0.f;  // (as hyd_sample_tokens: the same noise scale)
    a->top_k = p->top_k < p->n ? p->top_k : 0;
    a->top_p = p->top_p;
    a->log_min_p = p->min_p > 0.f ? (float)log((double)p->min_p) : -INFINITY;
    a->vec_ok = logits_vec_ok(p->logits, p->row_stride, 16 / esz);
    return HYD_OK;
}

// Everything hyd_sample_tokens_penalized checks, and the argument block of its kernel (shared with hyd_sample_tokens_constrained)
int fill_penalty_args(const hyd_sample_penalty_params* p, PenaltyArgs* ap) {
    PenaltyArgs& a = *ap;
    int rc = check_filter(p);
    if (rc) return rc;
    if (!(p->repetition_penalty > 0.0) || std::isinf(p->repetition_penalty))
        return fail(HYD_ERR_BAD_ARG, "repetition_penalty %g must be a finite number > 0 (1 = off)", p->repetition_penalty);
    if (!std::isfinite(p->frequency_penalty) || !std::isfinite(p->presence_penalty))
        return fail(HYD_ERR_BAD_ARG, "frequency_penalty %g / presence_penalty %g must be finite (0 = off)", p->frequency_penalty, p->presence_penalty);
    if (p->n_context < 0 || p->n_context > HYD_SAMPLE_MAX_CONTEXT)
        return fail(HYD_ERR_BAD_ARG, "n_context %d: 0 to %d context bitmaps", p->n_context, HYD_SAMPLE_MAX_CONTEXT);
    for (int l = 0; l < p->n_context; ++l) {
        if (!p->context[l].bits) return fail(HYD_ERR_BAD_ARG, "context[%d].bits is null", l);
        if (p->context[l].rows_per_group <= 0) return fail(HYD_ERR_BAD_ARG, "context[%d].rows_per_group %d must be > 0", l, p->context[l].rows_per_group);
        if (misaligned(p->context[l].bits, 4)) return fail(HYD_ERR_BAD_ARG, "context[%d].bits is not aligned to its element size", l);
    }
    if ((p->gen == nullptr) != (p->gen_len == nullptr)) return fail(HYD_ERR_BAD_ARG, "gen and gen_len go together (one of them is null)");
    if (p->gen_stride < 0) return fail(HYD_ERR_BAD_ARG, "gen_stride %d must be >= 0", p->gen_stride);
    if (p->gen_stride > HYD_SAMPLE_GEN_MAX) return fail(HYD_ERR_UNSUPPORTED, "gen_stride %d: up to %d generated tokens per row", p->gen_stride, HYD_SAMPLE_GEN_MAX);
    if (p->append_out && !p->gen) return fail(HYD_ERR_BAD_ARG, "append_out needs gen and gen_len (null)");
    if (p->n_bias < 0 || p->n_bias > HYD_SAMPLE_BIAS_MAX) return fail(HYD_ERR_BAD_ARG, "n_bias %d: 0 to %d logit-bias entries", p->n_bias, HYD_SAMPLE_BIAS_MAX);
    if (p->n_bias > 0 && (!p->bias_ids || !p->bias_values)) return fail(HYD_ERR_BAD_ARG, "n_bias %d needs bias_ids and bias_values (null)", p->n_bias);
    memset(&a, 0, sizeof(a));
    if ((rc = fill_filter_args(p, &a.f))) return rc;
    if (misaligned(p->gen, 4) || misaligned(p->gen_len, 4) || misaligned(p->bias_ids, 8) || misaligned(p->bias_values, 4))
        return fail(HYD_ERR_BAD_ARG, "gen / gen_len / bias_ids / bias_values is not aligned to its element size");
    a.rep = p->repetition_penalty; a.inv_rep = 1.0 / p->repetition_penalty; a.freq = p->frequency_penalty; a.pres = p->presence_penalty;
    a.n_ctx = p->n_context; a.words = (p->n + 31) / 32;
    for (int l = 0; l < p->n_context; ++l) {
        a.ctx[l] = p->context[l].bits;
        a.ctx_rpg[l] = p->context[l].rows_per_group;
    }
    a.gen = p->gen; a.gen_len = p->gen_len; a.gen_stride = p->gen_stride; a.append_out = p->append_out ? 1 : 0;
    a.bias_ids = p->bias_ids; a.bias_values = p->bias_values; a.n_bias = p->n_bias;
    return HYD_OK;
}

}  // namespace

extern "C" {

int hyd_version(void) { return HYD_VERSION; }

const char* hyd_last_error_string(void) { return g_err; }

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

int hyd_suffix_attn_fwd_kvq(const hyd_suffix_params* p, const hyd_kv_quant* kq, void* stream) {
    int rc = check_suffix(p, true);
    if (rc) return rc;
    if ((rc = check_kvq(&kq, p->dtype))) return rc;
    if (p->n_partials < 0 || p->n_partials > HYD_MAX_LEVELS) return fail(HYD_ERR_BAD_ARG, "n_partials %d", p->n_partials);
    if (p->kv_len == 0 && p->n_partials == 0) return fail(HYD_ERR_BAD_ARG, "kv_len == 0 and no partials");
    return run_suffix(p, p->partials, p->n_partials, static_cast<hipStream_t>(stream), kq);
}

int hyd_suffix_attn_fwd(const hyd_suffix_params* p, void* stream) { return hyd_suffix_attn_fwd_kvq(p, nullptr, stream); }

int hyd_suffix_attn_causal_fwd(const hyd_suffix_params* p, void* stream) {
    int rc = check_suffix(p, true);
    if (rc) return rc;
    if ((rc = check_causal_tail(p, nullptr))) return rc;
    if (p->n_partials < 0 || p->n_partials > HYD_MAX_LEVELS) return fail(HYD_ERR_BAD_ARG, "n_partials %d", p->n_partials);
    if (p->kv_len == 0 && p->n_partials == 0) return fail(HYD_ERR_BAD_ARG, "kv_len == 0 and no partials");
    return run_suffix(p, p->partials, p->n_partials, static_cast<hipStream_t>(stream), nullptr, /*causal=*/true);
}

int hyd_kv_quant_supported(const hyd_suffix_params* p, const hyd_kv_quant* kq) {
    if (!p) return 0;
    const KvqKind kind = kvq_kind(kq, p->dtype);
    return kind == kKvqNone || (kind == kKvqFp8 && kvq_native(p, kq)) ? 1 : 0;
}

int hyd_narrow_kv_supported(const hyd_suffix_params* p) {
    if (!p || check_common(p->dtype, p->B, p->nq, p->Hq, p->Hkv, p->D) || check_narrow_dim(p->kv_dim, p->D, "kv_dim")) return 0;
    if (!narrow_kv_dim(p) || p->kv_len <= 0) return p->kv_len >= 0 ? 1 : 0;  // nothing narrow is read: the existing call
    return narrow_native(p) ? 1 : 0;
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

int hyd_rope_append_decode_kvq(const hyd_rope_params* p, const hyd_kv_quant* kq, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_common(p->dtype, p->B, 1, p->Hq, p->Hkv, p->D);
    if (rc) return rc;
    if ((rc = check_narrow_dim(p->head_dim, p->D, "head_dim"))) return rc;
    if ((rc = check_kvq(&kq, p->dtype))) return rc;
    const int narrow = p->head_dim != p->D ? p->head_dim : 0;
    if (narrow && kq) return fail_narrow_fp8();
    if ((rc = check_ptr_align(p->q, "q")) || (rc = check_ptr_align(p->k, "k")) || (rc = check_ptr_align(p->v, "v")) ||
        (rc = check_ptr_align(p->q_out, "q_out")) || (rc = check_ptr_align(p->k_cache, "k_cache")) ||
        (rc = check_ptr_align(p->v_cache, "v_cache")) || (rc = check_ptr_align(p->cos, "cos")) ||
        (rc = check_ptr_align(p->sin, "sin")))
        return rc;
    if (!p->position_ids || !p->seq_lens) return fail(HYD_ERR_BAD_ARG, "position_ids / seq_lens is null");
    if ((rc = check_stride8(p->q_batch_stride, "q_batch_stride")) || (rc = check_stride8(p->k_batch_stride, "k_batch_stride")) ||
        (rc = check_stride8(p->v_batch_stride, "v_batch_stride")) || (rc = check_stride8(p->kc_batch_stride, "kc_batch_stride")) ||
        (rc = check_stride8(p->kc_tok_stride, "kc_tok_stride")) || (rc = check_stride8(p->kc_head_stride, "kc_head_stride")) ||
        (rc = check_stride8(p->vc_batch_stride, "vc_batch_stride")) || (rc = check_stride8(p->vc_tok_stride, "vc_tok_stride")) ||
        (rc = check_stride8(p->vc_head_stride, "vc_head_stride")))
        return rc;
    if (p->cs_stride % 4 != 0) return fail(HYD_ERR_BAD_ARG, "cos/sin row stride must be a multiple of 4 floats");
    if (p->cache_len <= 0) return fail(HYD_ERR_BAD_ARG, "cache_len %d", p->cache_len);
    if (p->max_pos <= 0) return fail(HYD_ERR_BAD_ARG, "max_pos %d: the cos/sin tables need at least one row", p->max_pos);
    RopeArgs a;
    memset(&a, 0, sizeof(a));
    a.q = p->q; a.k = p->k; a.v = p->v; a.q_out = p->q_out; a.k_cache = p->k_cache; a.v_cache = p->v_cache;
    a.cos = p->cos; a.sin = p->sin; a.pos = p->position_ids; a.shared_len = p->shared_len; a.seq_lens = p->seq_lens;
    a.q_bs = p->q_batch_stride; a.k_bs = p->k_batch_stride; a.v_bs = p->v_batch_stride;
    a.kc_bs = p->kc_batch_stride; a.kc_ts = p->kc_tok_stride; a.kc_hs = p->kc_head_stride;
    a.vc_bs = p->vc_batch_stride; a.vc_ts = p->vc_tok_stride; a.vc_hs = p->vc_head_stride;
    a.pos_stride = p->pos_stride; a.cs_stride = p->cs_stride;
    a.B = p->B; a.Hq = p->Hq; a.Hkv = p->Hkv; a.cache_len = p->cache_len; a.max_pos = p->max_pos;
    if (narrow) {
        RopeNarrowArgs na;
        na.a = a;
        na.D = p->D;
        na.d = narrow;
        return launched(launch_rope_append_narrow(na, p->dtype, static_cast<hipStream_t>(stream)), "rope_append (narrow head dim) kernel launch");
    }
    if (kq) {
        RopeKvqArgs ka;
        ka.a = a;
        ka.k_scale = kq->k_scale;
        ka.v_scale = kq->v_scale;
        return launched(launch_rope_append_fp8(ka, p->dtype, p->D, static_cast<hipStream_t>(stream)), "rope_append (fp8 caches) kernel launch");
    }
    return launched(launch_rope_append(a, p->dtype, p->D, static_cast<hipStream_t>(stream)), "rope_append kernel launch");
}

int hyd_rope_append_decode(const hyd_rope_params* p, void* stream) { return hyd_rope_append_decode_kvq(p, nullptr, stream); }

int hyd_rope_append_multi(const hyd_rope_multi_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->T < 2 || p->T > 8) return fail(HYD_ERR_BAD_ARG, "T = %d tokens per row, 2 to 8 are taken (hyd_rope_append_decode takes one)", p->T);
    int rc = check_common(p->dtype, p->B, p->T, p->Hq, p->Hkv, p->D);
    if (rc) return rc;
    if ((rc = check_ptr_align(p->q, "q")) || (rc = check_ptr_align(p->k, "k")) || (rc = check_ptr_align(p->v, "v")) ||
        (rc = check_ptr_align(p->q_out, "q_out")) || (rc = check_ptr_align(p->k_cache, "k_cache")) ||
        (rc = check_ptr_align(p->v_cache, "v_cache")) || (rc = check_ptr_align(p->cos, "cos")) ||
        (rc = check_ptr_align(p->sin, "sin")))
        return rc;
    if (!p->position_ids || !p->seq_lens) return fail(HYD_ERR_BAD_ARG, "position_ids / seq_lens is null");
    if (misaligned(p->position_ids, 8) || misaligned(p->shared_len, 8) || misaligned(p->seq_lens, 4))
        return fail(HYD_ERR_BAD_ARG, "position_ids / shared_len / seq_lens is not aligned to its element size");
    if ((rc = check_stride8(p->q_batch_stride, "q_batch_stride")) || (rc = check_stride8(p->k_batch_stride, "k_batch_stride")) ||
        (rc = check_stride8(p->v_batch_stride, "v_batch_stride")) || (rc = check_stride8(p->q_tok_stride, "q_tok_stride")) ||
        (rc = check_stride8(p->k_tok_stride, "k_tok_stride")) || (rc = check_stride8(p->v_tok_stride, "v_tok_stride")) ||
        (rc = check_stride8(p->kc_batch_stride, "kc_batch_stride")) || (rc = check_stride8(p->kc_tok_stride, "kc_tok_stride")) ||
        (rc = check_stride8(p->kc_head_stride, "kc_head_stride")) || (rc = check_stride8(p->vc_batch_stride, "vc_batch_stride")) ||
        (rc = check_stride8(p->vc_tok_stride, "vc_tok_stride")) || (rc = check_stride8(p->vc_head_stride, "vc_head_stride")))
        return rc;
    if (p->cs_stride % 4 != 0) return fail(HYD_ERR_BAD_ARG, "cos/sin row stride must be a multiple of 4 floats");
    if (p->cache_len <= 0) return fail(HYD_ERR_BAD_ARG, "cache_len %d", p->cache_len);
    if (p->max_pos <= 0) return fail(HYD_ERR_BAD_ARG, "max_pos %d: the cos/sin tables need at least one row", p->max_pos);
    return launched(launch_rope_append_multi(*p, static_cast<hipStream_t>(stream)), "rope_append (multi-token) kernel launch");
}

int hyd_add_rmsnorm(const hyd_add_rmsnorm_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->dtype != HYD_F16 && p->dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d (fp16 / bf16)", p->dtype);
    if (p->rows < 0 || p->rows > 0x7fffffff) return fail(HYD_ERR_BAD_ARG, "rows %lld", (long long)p->rows);
    if (p->n <= 0 || p->n % 8 != 0 || p->n > 16384) return fail(HYD_ERR_UNSUPPORTED, "n %d: a multiple of 8 up to 16384", p->n);
    if (!p->x || !p->weight || !p->norm_out) return fail(HYD_ERR_BAD_ARG, "x / weight / norm_out is null");
    int rc;
    if ((rc = check_ptr_align(p->x, "x")) || (rc = check_ptr_align(p->weight, "weight")) || (rc = check_ptr_align(p->norm_out, "norm_out")) ||
        (rc = check_stride8(p->x_row_stride, "x_row_stride")) || (rc = check_stride8(p->norm_row_stride, "norm_row_stride")))
        return rc;
    if (p->residual && ((rc = check_ptr_align(p->residual, "residual")) || (rc = check_stride8(p->residual_row_stride, "residual_row_stride"))))
        return rc;
    if (p->residual && p->sum_out && ((rc = check_ptr_align(p->sum_out, "sum_out")) || (rc = check_stride8(p->sum_row_stride, "sum_row_stride"))))
        return rc;
    NormArgs a;
    memset(&a, 0, sizeof(a));
    a.x = p->x; a.residual = p->residual; a.weight = p->weight; a.sum_out = p->residual ? p->sum_out : nullptr; a.norm_out = p->norm_out;
    a.x_rs = p->x_row_stride; a.r_rs = p->residual_row_stride; a.s_rs = p->sum_row_stride; a.o_rs = p->norm_row_stride;
    a.rows = p->rows; a.n = p->n; a.eps = p->eps;
    return launched(launch_add_rmsnorm(a, p->dtype, static_cast<hipStream_t>(stream)), "add_rmsnorm kernel launch");
}

int hyd_swiglu(const hyd_swiglu_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->dtype != HYD_F16 && p->dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d (fp16 / bf16)", p->dtype);
    if (p->rows < 0 || p->n <= 0 || p->n % 8 != 0) return fail(HYD_ERR_UNSUPPORTED, "rows %lld, n %d: n must be a positive multiple of 8", (long long)p->rows, p->n);
    if (p->rows * (p->n / 8) > 0x7fffffffLL * 256) return fail(HYD_ERR_UNSUPPORTED, "rows x n too large for one launch");
    if (!p->gate || !p->up || !p->out) return fail(HYD_ERR_BAD_ARG, "gate / up / out is null");
    int rc;
    if ((rc = check_ptr_align(p->gate, "gate")) || (rc = check_ptr_align(p->up, "up")) || (rc = check_ptr_align(p->out, "out")) ||
        (rc = check_stride8(p->gate_row_stride, "gate_row_stride")) || (rc = check_stride8(p->up_row_stride, "up_row_stride")) ||
        (rc = check_stride8(p->out_row_stride, "out_row_stride")))
        return rc;
    SwigluArgs a;
    memset(&a, 0, sizeof(a));
    a.gate = p->gate; a.up = p->up; a.out = p->out;
    a.g_rs = p->gate_row_stride; a.u_rs = p->up_row_stride; a.o_rs = p->out_row_stride;
    a.rows = p->rows; a.n = p->n;
    return launched(launch_swiglu(a, p->dtype, static_cast<hipStream_t>(stream)), "swiglu kernel launch");
}

int hyd_sample_tokens(const hyd_sample_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_logits_rows(p->dtype, p->rows, p->n, /*max_n=*/0);  // (the plain sampler has no upper bound on n)
    if (rc) return rc;
    if (!p->logits || !p->out) return fail(HYD_ERR_BAD_ARG, "logits / out is null");
    if (!(p->temperature >= 0.f)) return fail(HYD_ERR_BAD_ARG, "temperature %g must be >= 0", (double)p->temperature);
    if ((rc = check_row_stride(p->row_stride, p->n))) return rc;
    if (misaligned(p->logits, logits_esz(p->dtype)) || misaligned(p->out, 8)) return fail(HYD_ERR_BAD_ARG, "logits / out is not aligned to its element size");
    SampleArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = p->logits; a.out = p->out; a.row_stride = p->row_stride; a.seed = p->seed; a.offset = p->offset;
    a.rows = p->rows; a.n = p->n;
    a.inv_temperature = p->temperature > 0.f ? 1.0f / p->temperature : 0.f;
    a.vec_ok = logits_vec_ok(p->logits, p->row_stride, 8);  // (8 elements for every dtype, fp32 included: as released)
    return launched(launch_sample(a, p->dtype, static_cast<hipStream_t>(stream)), "sample kernel launch");
}

int hyd_sample_tokens_filtered(const hyd_sample_filter_params* p, void* stream) {
    FilterArgs a;
    int rc = check_filter(p);
    if (!rc) rc = fill_filter_args(p, &a);
    return rc ? rc : launched(launch_sample_filter(a, p->dtype, static_cast<hipStream_t>(stream)), "sample_filter kernel launch");
}

int hyd_sample_tokens_penalized(const hyd_sample_penalty_params* p, void* stream) {
    PenaltyArgs a;
    const int rc = fill_penalty_args(p, &a);
    return rc ? rc : launched(launch_sample_penalty(a, p->dtype, static_cast<hipStream_t>(stream)), "sample_penalty kernel launch");
}

int hyd_sample_tokens_constrained(const hyd_sample_penalty_params* p, const hyd_token_dfa* c, void* stream) {
    if (!c) return hyd_sample_tokens_penalized(p, stream);
    PenaltyArgs a;
    const int rc = fill_penalty_args(p, &a);
    if (rc) return rc;
    if (!c->allowed || !c->next || !c->state) return fail(HYD_ERR_BAD_ARG, "hyd_token_dfa: allowed / next / state is null");
    if (c->n_states <= 0) return fail(HYD_ERR_BAD_ARG, "hyd_token_dfa: n_states %d must be > 0", c->n_states);
    if (c->allowed_stride < (p->n + 31) / 32)
        return fail(HYD_ERR_BAD_ARG, "hyd_token_dfa: allowed_stride %lld < ceil(n / 32) = %d words", (long long)c->allowed_stride, (p->n + 31) / 32);
    if (c->next_stride < p->n) return fail(HYD_ERR_BAD_ARG, "hyd_token_dfa: next_stride %lld < n %d", (long long)c->next_stride, p->n);
    if (misaligned(c->allowed, 4) || misaligned(c->next, 4) || misaligned(c->state, 4))
        return fail(HYD_ERR_BAD_ARG, "hyd_token_dfa: allowed / next / state is not aligned to its element size");
    ConstrainArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.allowed = c->allowed; ca.next = c->next; ca.state = c->state;
    ca.allowed_stride = c->allowed_stride; ca.next_stride = c->next_stride;
    ca.n_states = c->n_states; ca.advance = c->advance ? 1 : 0;
    // every penalty neutral (and nothing to append): x = l, so the row keeps the keys of its own width (sample_filter.hip's cost)
    const bool neutral = p->repetition_penalty == 1.0 && p->frequency_penalty == 0.0 && p->presence_penalty == 0.0 && p->n_bias == 0 && !p->append_out;
    return launched(launch_sample_constrain(a, ca, neutral, p->dtype, static_cast<hipStream_t>(stream)), "sample_constrain kernel launch");
}

int hyd_token_bitmap_build(const hyd_token_bitmap_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->groups < 0 || p->groups > 65535 || p->L < 0) return fail(HYD_ERR_BAD_ARG, "groups %d (0 to 65535), L %d", p->groups, p->L);
    if (p->n <= 0 || p->n > HYD_SAMPLE_FILTER_MAX_N) return fail(HYD_ERR_BAD_ARG, "n %d: 1 to %d", p->n, HYD_SAMPLE_FILTER_MAX_N);
    if (!p->ids || !p->bits) return fail(HYD_ERR_BAD_ARG, "ids / bits is null");
    if (p->id_stride < p->L) return fail(HYD_ERR_BAD_ARG, "id_stride %lld < L %d", (long long)p->id_stride, p->L);
    if (misaligned(p->ids, 8) || misaligned(p->lens, 8) || misaligned(p->bits, 4))
        return fail(HYD_ERR_BAD_ARG, "ids / lens / bits is not aligned to its element size");
    BitmapArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = p->ids; a.lens = p->lens; a.bits = p->bits; a.id_stride = p->id_stride;
    a.groups = p->groups; a.L = p->L; a.n = p->n; a.words = (p->n + 31) / 32;
    return launched(launch_token_bitmap(a, static_cast<hipStream_t>(stream)), "token_bitmap kernel launch");
}

int hyd_token_logprobs(const hyd_token_logprob_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_logits_rows(p->dtype, p->rows, p->n, HYD_SAMPLE_FILTER_MAX_N);
    if (rc) return rc;
    if (!p->logits || !p->targets || !p->logprobs || !p->greedy) return fail(HYD_ERR_BAD_ARG, "logits / targets / logprobs / greedy is null");
    if (p->top_n < 0 || p->top_n > HYD_TOP_LOGPROBS_MAX) return fail(HYD_ERR_BAD_ARG, "top_n %d must be in [0, %d]", p->top_n, HYD_TOP_LOGPROBS_MAX);
    if (p->top_n > 0 && (!p->top_ids || !p->top_logprobs)) return fail(HYD_ERR_BAD_ARG, "top_n %d needs top_ids and top_logprobs (null)", p->top_n);
    if ((rc = check_row_stride(p->row_stride, p->n))) return rc;
    const int esz = logits_esz(p->dtype);
    if (misaligned(p->logits, esz) || misaligned(p->targets, 8) || misaligned(p->logprobs, 4) || misaligned(p->top_ids, 8) || misaligned(p->top_logprobs, 4))
        return fail(HYD_ERR_BAD_ARG, "logits / targets / logprobs / top_ids / top_logprobs is not aligned to its element size");
    TokenLogprobArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = p->logits; a.targets = p->targets; a.logprobs = p->logprobs; a.greedy = p->greedy;
    a.top_ids = p->top_ids; a.top_logprobs = p->top_logprobs;
    a.row_stride = p->row_stride; a.rows = p->rows; a.n = p->n; a.top_n = p->top_n;
    a.vec_ok = logits_vec_ok(p->logits, p->row_stride, 16 / esz);
    return launched(launch_token_logprob(a, p->dtype, static_cast<hipStream_t>(stream)), "token_logprob kernel launch");
}

int hyd_stop_update(const hyd_stop_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->rows < 0) return fail(HYD_ERR_BAD_ARG, "rows %d", p->rows);
    if (p->n_eos < 0 || p->n_eos > HYD_STOP_MAX_EOS) return fail(HYD_ERR_BAD_ARG, "n_eos %d: 0 to %d EOS ids", p->n_eos, HYD_STOP_MAX_EOS);
    if (p->n_stop < 0 || p->n_stop > HYD_STOP_MAX_SEQS) return fail(HYD_ERR_BAD_ARG, "n_stop %d: 0 to %d stop sequences", p->n_stop, HYD_STOP_MAX_SEQS);
    for (int k = 0; k < p->n_stop; ++k)
        if (p->stop_lens[k] < 1 || p->stop_lens[k] > HYD_STOP_MAX_LEN)
            return fail(HYD_ERR_BAD_ARG, "stop_lens[%d] = %d: a stop sequence holds 1 to %d tokens", k, p->stop_lens[k], HYD_STOP_MAX_LEN);
    if (p->t < 0 || p->t >= p->out_stride) return fail(HYD_ERR_BAD_ARG, "t %d outside [0, out_stride = %lld)", p->t, (long long)p->out_stride);
    if (!p->tok || !p->out || !p->length || !p->reason || !p->stop_index || !p->live)
        return fail(HYD_ERR_BAD_ARG, "tok / out / length / reason / stop_index / live is null");
    if (!p->start_pos || !p->feed || !p->next_pos) return fail(HYD_ERR_BAD_ARG, "start_pos / feed / next_pos is null");
    if (p->n_stop > 0 && !p->stop_tokens) return fail(HYD_ERR_BAD_ARG, "n_stop %d needs stop_tokens (null)", p->n_stop);
    if (misaligned(p->tok, 8) || misaligned(p->out, 8) || misaligned(p->stop_tokens, 8) || misaligned(p->start_pos, 8) ||
        misaligned(p->shared_len, 8) || misaligned(p->feed, 8) || misaligned(p->next_pos, 8))
        return fail(HYD_ERR_BAD_ARG, "tok / out / stop_tokens / start_pos / shared_len / feed / next_pos is not aligned to its element size");
    if (misaligned(p->length, 4) || misaligned(p->reason, 4) || misaligned(p->stop_index, 4) || misaligned(p->live, 4))
        return fail(HYD_ERR_BAD_ARG, "length / reason / stop_index / live is not aligned to its element size");
    if (p->rows == 0) return HYD_OK;
    StopArgs a;
    memset(&a, 0, sizeof(a));
    a.tok = p->tok; a.out = p->out; a.length = p->length; a.reason = p->reason; a.stop_index = p->stop_index; a.live = p->live;
    a.stop_tokens = p->stop_tokens; a.start_pos = p->start_pos; a.shared_len = p->shared_len; a.feed = p->feed; a.next_pos = p->next_pos;
    a.out_stride = p->out_stride; a.pad = p->pad;
    for (int i = 0; i < p->n_eos; ++i) a.eos[i] = p->eos[i];
    for (int k = 0; k < p->n_stop; ++k) a.stop_lens[k] = p->stop_lens[k];
    a.rows = p->rows; a.t = p->t; a.n_eos = p->n_eos; a.n_stop = p->n_stop;
    a.include_stop = p->include_stop ? 1 : 0; a.retire = p->retire ? 1 : 0;
    return launched(launch_stop_update(a, static_cast<hipStream_t>(stream)), "stop_update kernel launch");
}

int hyd_draft_lookup(const hyd_draft_lookup_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->B < 0) return fail(HYD_ERR_BAD_ARG, "B %d", p->B);
    if (p->K < 1 || p->K > 7) return fail(HYD_ERR_BAD_ARG, "K = %d drafts per row, 1 to 7 are taken", p->K);
    if (p->ngram_min < 1 || p->ngram_max < p->ngram_min || p->ngram_max > HYD_DRAFT_MAX_NGRAM)
        return fail(HYD_ERR_BAD_ARG, "ngram (%d, %d): 1 <= min <= max <= %d", p->ngram_min, p->ngram_max, HYD_DRAFT_MAX_NGRAM);
    if (p->n_segments < 1 || p->n_segments > HYD_DRAFT_MAX_SEGMENTS)
        return fail(HYD_ERR_BAD_ARG, "n_segments %d: 1 to %d segments", p->n_segments, HYD_DRAFT_MAX_SEGMENTS);
    if (!p->drafts || !p->n_proposed) return fail(HYD_ERR_BAD_ARG, "drafts / n_proposed is null");
    if (misaligned(p->drafts, 8) || misaligned(p->n_proposed, 4)) return fail(HYD_ERR_BAD_ARG, "drafts / n_proposed is not aligned to its element size");
    if (p->drafts_stride < p->K) return fail(HYD_ERR_BAD_ARG, "drafts_stride %lld < K = %d", (long long)p->drafts_stride, p->K);
    for (int i = 0; i < p->n_segments; ++i) {
        const hyd_draft_segment& g = p->segments[i];
        if (g.div < 1) return fail(HYD_ERR_BAD_ARG, "segment %d: div %d (rows of the batch per row of the segment) must be positive", i, g.div);
        if (g.len < 0) return fail(HYD_ERR_BAD_ARG, "segment %d: len %d", i, g.len);
        if (!g.ids && g.len != 0) return fail(HYD_ERR_BAD_ARG, "segment %d: ids is null", i);
        if (misaligned(g.ids, 8) || misaligned(g.lens_i64, 8) || misaligned(g.lens_i32, 4))
            return fail(HYD_ERR_BAD_ARG, "segment %d: ids / lens is not aligned to its element size", i);
    }
    return launched(launch_draft_lookup(*p, static_cast<hipStream_t>(stream)), "draft_lookup kernel launch");
}

int hyd_dfa_forced_tokens(const hyd_dfa_forced_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->n_states <= 0 || p->n <= 0) return fail(HYD_ERR_BAD_ARG, "n_states %d, n %d must be > 0", p->n_states, p->n);
    if (p->allowed_stride < (p->n + 31) / 32)
        return fail(HYD_ERR_BAD_ARG, "allowed_stride %lld < ceil(n / 32) = %d words", (long long)p->allowed_stride, (p->n + 31) / 32);
    if (!p->allowed || !p->forced) return fail(HYD_ERR_BAD_ARG, "allowed / forced is null");
    if (misaligned(p->allowed, 4) || misaligned(p->forced, 4)) return fail(HYD_ERR_BAD_ARG, "allowed / forced is not aligned to its element size");
    return launched(launch_dfa_forced(*p, static_cast<hipStream_t>(stream)), "dfa_forced kernel launch");
}

int hyd_draft_constrain(const hyd_draft_constrain_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->B < 0) return fail(HYD_ERR_BAD_ARG, "B %d", p->B);
    if (p->K < 1 || p->K > 7) return fail(HYD_ERR_BAD_ARG, "K = %d drafts per row, 1 to 7 are taken", p->K);
    if (p->n_states <= 0 || p->n <= 0) return fail(HYD_ERR_BAD_ARG, "n_states %d, n %d must be > 0", p->n_states, p->n);
    if (p->next_stride < p->n) return fail(HYD_ERR_BAD_ARG, "next_stride %lld < n %d", (long long)p->next_stride, p->n);
    if (p->fed_stride < p->K + 1) return fail(HYD_ERR_BAD_ARG, "fed_stride %lld < K + 1 = %d", (long long)p->fed_stride, p->K + 1);
    if (!p->state || !p->fed || !p->forced || !p->next || !p->step_state || !p->n_forced)
        return fail(HYD_ERR_BAD_ARG, "state / fed / forced / next / step_state / n_forced is null");
    if (misaligned(p->fed, 8) || misaligned(p->state, 4) || misaligned(p->n_proposed, 4) || misaligned(p->forced, 4) ||
        misaligned(p->next, 4) || misaligned(p->step_state, 4) || misaligned(p->n_forced, 4))
        return fail(HYD_ERR_BAD_ARG, "state / fed / n_proposed / forced / next / step_state / n_forced is not aligned to its element size");
    return launched(launch_draft_constrain(*p, static_cast<hipStream_t>(stream)), "draft_constrain kernel launch");
}

static int check_draft_accept(const hyd_draft_accept_params* p);

int hyd_draft_accept_states(const hyd_draft_accept_params* p, const int32_t* step_state_after, int32_t* state, void* stream) {
    if (!step_state_after && !state) return hyd_draft_accept(p, stream);
    const int rc = check_draft_accept(p);
    if (rc) return rc;
    if (!step_state_after || !state) return fail(HYD_ERR_BAD_ARG, "step_state_after and state go together: one of them is null");
    if (misaligned(step_state_after, 4) || misaligned(state, 4)) return fail(HYD_ERR_BAD_ARG, "step_state_after / state is not aligned to its element size");
    return launched(launch_draft_accept_states(*p, step_state_after, state, static_cast<hipStream_t>(stream)), "draft_accept kernel launch");
}

int hyd_draft_accept(const hyd_draft_accept_params* p, void* stream) {
    const int rc = check_draft_accept(p);
    return rc ? rc : launched(launch_draft_accept(*p, static_cast<hipStream_t>(stream)), "draft_accept kernel launch");
}

static int check_draft_accept(const hyd_draft_accept_params* p) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->rows < 0) return fail(HYD_ERR_BAD_ARG, "rows %d", p->rows);
    if (p->T < 1 || p->T > 8) return fail(HYD_ERR_BAD_ARG, "T = %d tokens per row (K = %d drafts): 1 to 8 tokens are taken", p->T, p->T - 1);
    if (p->n_eos < 0 || p->n_eos > HYD_STOP_MAX_EOS) return fail(HYD_ERR_BAD_ARG, "n_eos %d: 0 to %d EOS ids", p->n_eos, HYD_STOP_MAX_EOS);
    if (p->max_new_tokens < 1 || p->max_new_tokens > p->out_stride)
        return fail(HYD_ERR_BAD_ARG, "max_new_tokens %d outside [1, out_stride = %lld]", p->max_new_tokens, (long long)p->out_stride);
    if (!p->fed || !p->sampled || !p->out || !p->length || !p->reason || !p->stop_index || !p->accepted || !p->live)
        return fail(HYD_ERR_BAD_ARG, "fed / sampled / out / length / reason / stop_index / accepted / live is null");
    if (!p->start_pos || !p->feed || !p->next_pos) return fail(HYD_ERR_BAD_ARG, "start_pos / feed / next_pos is null");
    if (misaligned(p->fed, 8) || misaligned(p->sampled, 8) || misaligned(p->out, 8) || misaligned(p->start_pos, 8) ||
        misaligned(p->shared_len, 8) || misaligned(p->feed, 8) || misaligned(p->next_pos, 8))
        return fail(HYD_ERR_BAD_ARG, "fed / sampled / out / start_pos / shared_len / feed / next_pos is not aligned to its element size");
    if (misaligned(p->length, 4) || misaligned(p->reason, 4) || misaligned(p->stop_index, 4) || misaligned(p->accepted, 4) ||
        misaligned(p->live, 4) || misaligned(p->logprobs, 4) || misaligned(p->out_logprobs, 4))
        return fail(HYD_ERR_BAD_ARG, "length / reason / stop_index / accepted / live / logprobs / out_logprobs is not aligned to its element size");
    return HYD_OK;
}

int hyd_kv_promote(const hyd_kv_promote_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->dst_dtype != HYD_F16 && p->dst_dtype != HYD_BF16)
        return fail(HYD_ERR_UNSUPPORTED, "dst_dtype %d: shared levels are f16 / bf16 (no fp8 or 32-bit destination)", p->dst_dtype);
    if (p->src_dtype != HYD_F16 && p->src_dtype != HYD_BF16 && p->src_dtype != HYD_FP8_E4M3)
        return fail(HYD_ERR_UNSUPPORTED, "src_dtype %d: f16, bf16 or HYD_FP8_E4M3 (%d)", p->src_dtype, HYD_FP8_E4M3);
    if (p->src_dtype != HYD_FP8_E4M3 && p->src_dtype != p->dst_dtype)
        return fail(HYD_ERR_BAD_ARG, "src_dtype %d differs from dst_dtype %d: a 16-bit source is copied as bytes", p->src_dtype, p->dst_dtype);
    if (p->n <= 0) return fail(HYD_ERR_BAD_ARG, "n %d must be > 0", p->n);
    if (p->Hkv <= 0) return fail(HYD_ERR_BAD_ARG, "Hkv %d must be > 0", p->Hkv);
    if (p->B <= 0 || p->src_rows <= 0 || p->capacity < 0)
        return fail(HYD_ERR_BAD_ARG, "B %d / src_rows %d must be > 0, capacity %d >= 0", p->B, p->src_rows, p->capacity);
    if (p->d_src <= 0 || p->d_src % 8 != 0) return fail(HYD_ERR_BAD_ARG, "d_src %d must be a positive multiple of 8 (16-byte vectors)", p->d_src);
    if (p->d_dst < p->d_src) return fail(HYD_ERR_BAD_ARG, "d_dst %d < d_src %d", p->d_dst, p->d_src);
    if (p->d_dst != p->d_src && p->d_dst != 64 && p->d_dst != 128 && p->d_dst != 256)
        return fail(HYD_ERR_UNSUPPORTED, "d_dst %d: 64, 128, 256 or d_src (%d)", p->d_dst, p->d_src);
    if (p->max_len < 0 || p->max_len > p->src_rows) return fail(HYD_ERR_BAD_ARG, "max_len %d outside [0, src_rows = %d]", p->max_len, p->src_rows);
    if (p->n > 65535) return fail(HYD_ERR_UNSUPPORTED, "n %d: up to 65535 sequences per launch", p->n);
    if (int rc = check_ptr_align(p->k_src, "k_src")) return rc;
    if (int rc = check_ptr_align(p->v_src, "v_src")) return rc;
    if (int rc = check_ptr_align(p->k_dst, "k_dst")) return rc;
    if (int rc = check_ptr_align(p->v_dst, "v_dst")) return rc;
    if (!p->rows || !p->lens || !p->cu) return fail(HYD_ERR_BAD_ARG, "rows / lens / cu is null");
    if (misaligned(p->rows, 4) || misaligned(p->lens, 4) || misaligned(p->cu, 4) || misaligned(p->k_scale, 4) || misaligned(p->v_scale, 4))
        return fail(HYD_ERR_BAD_ARG, "rows / lens / cu / k_scale / v_scale is not aligned to its element size");
    if (int rc = check_stride8(p->k_batch_stride, "k_batch_stride")) return rc;
    if (int rc = check_stride8(p->k_tok_stride, "k_tok_stride")) return rc;
    if (int rc = check_stride8(p->k_head_stride, "k_head_stride")) return rc;
    if (int rc = check_stride8(p->v_batch_stride, "v_batch_stride")) return rc;
    if (int rc = check_stride8(p->v_tok_stride, "v_tok_stride")) return rc;
    if (int rc = check_stride8(p->v_head_stride, "v_head_stride")) return rc;
    if (p->Hkv > 1 && (p->k_head_stride < p->d_src || p->v_head_stride < p->d_src))
        return fail(HYD_ERR_BAD_ARG, "k_head_stride %lld / v_head_stride %lld < d_src %d", (long long)p->k_head_stride, (long long)p->v_head_stride, p->d_src);
    const int max_len = p->max_len ? p->max_len : p->src_rows;
    const int64_t vec_per_tok = (int64_t)p->Hkv * (p->d_dst / 8);
    if (vec_per_tok * max_len >= (1LL << 31))
        return fail(HYD_ERR_UNSUPPORTED, "max_len %d x Hkv %d x d_dst %d: a sequence of more than 2^31 16-byte vectors", max_len, p->Hkv, p->d_dst);
    KvPromoteArgs a;
    memset(&a, 0, sizeof(a));
    a.k_src = p->k_src; a.v_src = p->v_src; a.k_dst = p->k_dst; a.v_dst = p->v_dst;
    a.rows = p->rows; a.lens = p->lens; a.cu = p->cu;
    if (p->src_dtype == HYD_FP8_E4M3) { a.k_scale = p->k_scale; a.v_scale = p->v_scale; }
    a.k_bs = p->k_batch_stride; a.k_ts = p->k_tok_stride; a.k_hs = p->k_head_stride;
    a.v_bs = p->v_batch_stride; a.v_ts = p->v_tok_stride; a.v_hs = p->v_head_stride;
    a.n = p->n; a.B = p->B; a.max_len = max_len; a.capacity = p->capacity; a.d_src = p->d_src;
    a.vec_per_head = p->d_dst / 8; a.vec_per_tok = (int32_t)vec_per_tok;
    a.div_vec_per_head = make_fastdiv((uint32_t)a.vec_per_head);
    a.div_vec_per_tok = make_fastdiv((uint32_t)a.vec_per_tok);
    return launched(launch_kv_promote(a, p->src_dtype, p->dst_dtype, static_cast<hipStream_t>(stream)), "kv_promote kernel launch");
}

int hyd_kv_gather_paths(const hyd_kv_gather_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->dst_dtype != HYD_F16 && p->dst_dtype != HYD_BF16)
        return fail(HYD_ERR_UNSUPPORTED, "dst_dtype %d: shared levels are f16 / bf16 (no fp8 or 32-bit destination)", p->dst_dtype);
    if (p->src_dtype != HYD_F16 && p->src_dtype != HYD_BF16 && p->src_dtype != HYD_FP8_E4M3)
        return fail(HYD_ERR_UNSUPPORTED, "src_dtype %d: f16, bf16 or HYD_FP8_E4M3 (%d)", p->src_dtype, HYD_FP8_E4M3);
    if (p->src_dtype != HYD_FP8_E4M3 && p->src_dtype != p->dst_dtype)
        return fail(HYD_ERR_BAD_ARG, "src_dtype %d differs from dst_dtype %d: a 16-bit source is copied as bytes", p->src_dtype, p->dst_dtype);
    if (p->n <= 0) return fail(HYD_ERR_BAD_ARG, "n %d must be > 0", p->n);
    if (p->n_levels < 0 || p->n_levels > HYD_MAX_LEVELS) return fail(HYD_ERR_BAD_ARG, "n_levels %d outside [0, %d]", p->n_levels, HYD_MAX_LEVELS);
    if (p->Hkv <= 0) return fail(HYD_ERR_BAD_ARG, "Hkv %d must be > 0", p->Hkv);
    if (p->B <= 0 || p->src_rows <= 0 || p->capacity < 0)
        return fail(HYD_ERR_BAD_ARG, "B %d / src_rows %d must be > 0, capacity %d >= 0", p->B, p->src_rows, p->capacity);
    if (p->d_src <= 0 || p->d_src % 8 != 0) return fail(HYD_ERR_BAD_ARG, "d_src %d must be a positive multiple of 8 (16-byte vectors)", p->d_src);
    if (p->d_dst < p->d_src) return fail(HYD_ERR_BAD_ARG, "d_dst %d < d_src %d", p->d_dst, p->d_src);
    if (p->d_dst != p->d_src && p->d_dst != 64 && p->d_dst != 128 && p->d_dst != 256)
        return fail(HYD_ERR_UNSUPPORTED, "d_dst %d: 64, 128, 256 or d_src (%d)", p->d_dst, p->d_src);
    if (p->max_len < 0 || p->max_len > p->src_rows) return fail(HYD_ERR_BAD_ARG, "max_len %d outside [0, src_rows = %d]", p->max_len, p->src_rows);
    if (p->max_path < 0 || p->max_path > p->capacity) return fail(HYD_ERR_BAD_ARG, "max_path %d outside [0, capacity = %d]", p->max_path, p->capacity);
    if (p->n > 65535) return fail(HYD_ERR_UNSUPPORTED, "n %d: up to 65535 sequences per launch", p->n);
    if (int rc = check_ptr_align(p->k_src, "k_src")) return rc;
    if (int rc = check_ptr_align(p->v_src, "v_src")) return rc;
    if (int rc = check_ptr_align(p->k_dst, "k_dst")) return rc;
    if (int rc = check_ptr_align(p->v_dst, "v_dst")) return rc;
    if (!p->rows || !p->lens || !p->cu_dst) return fail(HYD_ERR_BAD_ARG, "rows / lens / cu_dst is null");
    if (misaligned(p->rows, 4) || misaligned(p->lens, 4) || misaligned(p->cu_dst, 4) || misaligned(p->k_scale, 4) || misaligned(p->v_scale, 4))
        return fail(HYD_ERR_BAD_ARG, "rows / lens / cu_dst / k_scale / v_scale is not aligned to its element size");
    if (int rc = check_stride8(p->k_batch_stride, "k_batch_stride")) return rc;
    if (int rc = check_stride8(p->k_tok_stride, "k_tok_stride")) return rc;
    if (int rc = check_stride8(p->k_head_stride, "k_head_stride")) return rc;
    if (int rc = check_stride8(p->v_batch_stride, "v_batch_stride")) return rc;
    if (int rc = check_stride8(p->v_tok_stride, "v_tok_stride")) return rc;
    if (int rc = check_stride8(p->v_head_stride, "v_head_stride")) return rc;
    if (p->Hkv > 1 && (p->k_head_stride < p->d_src || p->v_head_stride < p->d_src))
        return fail(HYD_ERR_BAD_ARG, "k_head_stride %lld / v_head_stride %lld < d_src %d", (long long)p->k_head_stride, (long long)p->v_head_stride, p->d_src);
    for (int j = 0; j < p->n_levels; ++j) {
        char name[32];
        snprintf(name, sizeof(name), "level_k[%d]", j);
        if (int rc = check_ptr_align(p->level_k[j], name)) return rc;
        snprintf(name, sizeof(name), "level_v[%d]", j);
        if (int rc = check_ptr_align(p->level_v[j], name)) return rc;
        if (!p->level_cu[j] || misaligned(p->level_cu[j], 4)) return fail(HYD_ERR_BAD_ARG, "level_cu[%d] is null or not 4-byte aligned", j);
        if (p->level_div[j] <= 0) return fail(HYD_ERR_BAD_ARG, "level_div[%d] = %d must be > 0 (old_batch / s_j)", j, p->level_div[j]);
        if (p->level_s[j] <= 0 || p->level_cap[j] < 0)
            return fail(HYD_ERR_BAD_ARG, "level_s[%d] = %d must be > 0, level_cap[%d] = %d >= 0", j, p->level_s[j], j, p->level_cap[j]);
    }
    const int max_len = p->max_len ? p->max_len : p->src_rows;
    const int max_path = p->max_path ? p->max_path : p->capacity;
    const int64_t vec_per_tok = (int64_t)p->Hkv * (p->d_dst / 8);
    if (vec_per_tok * max_len >= (1LL << 31))
        return fail(HYD_ERR_UNSUPPORTED, "max_len %d x Hkv %d x d_dst %d: a sequence of more than 2^31 16-byte vectors", max_len, p->Hkv, p->d_dst);
    if (vec_per_tok * max_path >= (1LL << 31))
        return fail(HYD_ERR_UNSUPPORTED, "max_path %d x Hkv %d x d_dst %d: a path of more than 2^31 16-byte vectors", max_path, p->Hkv, p->d_dst);
    if (max_path == 0) return HYD_OK;  // (an empty destination: nothing can be written)
    KvGatherArgs g;
    memset(&g, 0, sizeof(g));
    for (int j = 0; j < p->n_levels; ++j) {
        g.lk[j] = p->level_k[j]; g.lv[j] = p->level_v[j]; g.lcu[j] = p->level_cu[j];
        g.ls[j] = p->level_s[j]; g.lcap[j] = p->level_cap[j];
        g.ldiv[j] = make_fastdiv((uint32_t)p->level_div[j]);
    }
    g.n_levels = p->n_levels; g.max_path = max_path;
    KvPromoteArgs& a = g.u;
    a.k_src = p->k_src; a.v_src = p->v_src; a.k_dst = p->k_dst; a.v_dst = p->v_dst;
    a.rows = p->rows; a.lens = p->lens; a.cu = p->cu_dst;
    if (p->src_dtype == HYD_FP8_E4M3) { a.k_scale = p->k_scale; a.v_scale = p->v_scale; }
    a.k_bs = p->k_batch_stride; a.k_ts = p->k_tok_stride; a.k_hs = p->k_head_stride;
    a.v_bs = p->v_batch_stride; a.v_ts = p->v_tok_stride; a.v_hs = p->v_head_stride;
    a.n = p->n; a.B = p->B; a.max_len = max_len; a.capacity = p->capacity; a.d_src = p->d_src;
    a.vec_per_head = p->d_dst / 8; a.vec_per_tok = (int32_t)vec_per_tok;
    a.div_vec_per_head = make_fastdiv((uint32_t)a.vec_per_head);
    a.div_vec_per_tok = make_fastdiv((uint32_t)a.vec_per_tok);
    return launched(launch_kv_gather(g, p->src_dtype, p->dst_dtype, static_cast<hipStream_t>(stream)), "kv_gather kernel launch");
}

int hyd_kv_absmax(const hyd_kv_absmax_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->dtype != HYD_F16 && p->dtype != HYD_BF16)
        return fail(HYD_ERR_UNSUPPORTED, "dtype %d: the observed K / V are f16 / bf16 (no fp8 or 32-bit source)", p->dtype);
    if (p->Hkv < 1) return fail(HYD_ERR_BAD_ARG, "Hkv %d must be >= 1", p->Hkv);
    if (p->d < 8 || p->d > 256 || p->d % 8 != 0) return fail(HYD_ERR_BAD_ARG, "d %d must be a multiple of 8 in 8..256 (16-byte vectors)", p->d);
    if (p->n_outer < 0 || p->n_rows < 0) return fail(HYD_ERR_BAD_ARG, "n_outer %d / n_rows %d must be >= 0", p->n_outer, p->n_rows);
    if (!p->amax) return fail(HYD_ERR_BAD_ARG, "amax is null");
    if (!p->k && !p->v) return fail(HYD_ERR_BAD_ARG, "k and v are both null");
    if (misaligned(p->k, 16)) return fail(HYD_ERR_BAD_ARG, "k must be 16-byte aligned");
    if (misaligned(p->v, 16)) return fail(HYD_ERR_BAD_ARG, "v must be 16-byte aligned");
    if (misaligned(p->amax, 4) || misaligned(p->row_lens, 4)) return fail(HYD_ERR_BAD_ARG, "amax / row_lens is not aligned to its element size");
    if (p->k) {
        if (int rc = check_stride8(p->k_outer_stride, "k_outer_stride")) return rc;
        if (int rc = check_stride8(p->k_row_stride, "k_row_stride")) return rc;
        if (int rc = check_stride8(p->k_head_stride, "k_head_stride")) return rc;
    }
    if (p->v) {
        if (int rc = check_stride8(p->v_outer_stride, "v_outer_stride")) return rc;
        if (int rc = check_stride8(p->v_row_stride, "v_row_stride")) return rc;
        if (int rc = check_stride8(p->v_head_stride, "v_head_stride")) return rc;
    }
    if (p->n_rows > (1 << 30)) return fail(HYD_ERR_UNSUPPORTED, "n_rows %d: up to 2^30 rows per outer index", p->n_rows);
    const int64_t vpr = (int64_t)p->Hkv * (p->d / 8);
    if (vpr > (1 << 24)) return fail(HYD_ERR_UNSUPPORTED, "Hkv %d x d %d: a token row of more than 2^24 16-byte vectors", p->Hkv, p->d);
    if (p->n_outer == 0 || p->n_rows == 0) return HYD_OK;
    KvAbsmaxArgs a;
    memset(&a, 0, sizeof(a));
    a.k = p->k; a.v = p->v; a.row_lens = p->row_lens; a.amax = reinterpret_cast<unsigned*>(p->amax);
    a.k_os = p->k_outer_stride; a.k_rs = p->k_row_stride; a.k_hs = p->k_head_stride;
    a.v_os = p->v_outer_stride; a.v_rs = p->v_row_stride; a.v_hs = p->v_head_stride;
    a.Hkv = p->Hkv; a.n_outer = p->n_outer; a.n_rows = p->n_rows;
    a.pph = p->d / 8; a.vpr = (int32_t)vpr;
    a.cols = a.vpr < 256 ? a.vpr : 256;
    a.rstep = 256 / a.cols;
    a.group = a.pph & -a.pph;  // (pph <= 32)
    const int rows_per_wg = HYD_KV_ABSMAX_PASSES * a.rstep;
    a.chunks = (p->n_rows + rows_per_wg - 1) / rows_per_wg;
    a.only = p->k && p->v ? 0 : (p->k ? 1 : 2);
    a.div_pph = make_fastdiv((uint32_t)a.pph);
    a.div_cols = make_fastdiv((uint32_t)a.cols);
    a.div_chunks = make_fastdiv((uint32_t)a.chunks);
    if ((int64_t)a.chunks * a.n_outer > 0x7fffffffLL || (a.vpr + a.cols - 1) / a.cols > 65535)
        return fail(HYD_ERR_UNSUPPORTED, "n_outer %d x n_rows %d x Hkv %d: more workgroups than one launch takes", p->n_outer, p->n_rows, p->Hkv);
    return launched(launch_kv_absmax(a, p->dtype, static_cast<hipStream_t>(stream)), "kv_absmax kernel launch");
}

int hyd_kv_scales_from_absmax(const hyd_kv_scales_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (!p->amax || !p->k_scale || !p->v_scale) return fail(HYD_ERR_BAD_ARG, "amax / k_scale / v_scale is null");
    if (misaligned(p->amax, 4) || misaligned(p->k_scale, 4) || misaligned(p->v_scale, 4))
        return fail(HYD_ERR_BAD_ARG, "amax / k_scale / v_scale is not aligned to its element size");
    if (p->Hkv < 1) return fail(HYD_ERR_BAD_ARG, "Hkv %d must be >= 1", p->Hkv);
    if (!(p->c > 0.f) || std::isinf(p->c)) return fail(HYD_ERR_BAD_ARG, "c %g must be finite and positive (margin / 448)", (double)p->c);
    KvScalesArgs a;
    memset(&a, 0, sizeof(a));
    a.amax = p->amax; a.k_scale = p->k_scale; a.v_scale = p->v_scale;
    a.Hkv = p->Hkv; a.pow2 = p->pow2 ? 1 : 0; a.c = p->c;
    return launched(launch_kv_scales(a, static_cast<hipStream_t>(stream)), "kv_scales kernel launch");
}

// ---- fp8 linear-layer weights (linear_w8.hip) --------------------------------------------------------------------------------
static int check_w8_common(const void* w8, const float* scale, int32_t N, int32_t K, int32_t dtype, int k_multiple) {
    if (dtype != HYD_F16 && dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d: f16 / bf16 activations (the weights are e4m3fn)", dtype);
    if (N < 1 || K < 1) return fail(HYD_ERR_BAD_ARG, "N %d / K %d must be >= 1", N, K);
    if (K % k_multiple != 0) return fail(HYD_ERR_BAD_ARG, "K %d must be a multiple of %d", K, k_multiple);
    if (int rc = check_ptr_align(w8, "w8")) return rc;
    if (!scale) return fail(HYD_ERR_BAD_ARG, "scale is null");
    if (misaligned(scale, 4)) return fail(HYD_ERR_BAD_ARG, "scale is not aligned to its element size");
    return HYD_OK;
}

size_t hyd_linear_w8_workspace_bytes(int32_t M, int32_t N, int32_t K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    return plan_linear_w8(M, N, K).bytes;
}

int hyd_linear_w8(const hyd_linear_w8_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->M < 1) return fail(HYD_ERR_BAD_ARG, "M %d must be >= 1", p->M);
    if (int rc = check_w8_common(p->w8, p->scale, p->N, p->K, p->dtype, 16)) return rc;
    if (int rc = check_ptr_align(p->x, "x")) return rc;
    if (int rc = check_ptr_align(p->y, "y")) return rc;
    if (int rc = check_stride8(p->x_row_stride, "x_row_stride")) return rc;
    if (int rc = check_stride8(p->y_row_stride, "y_row_stride")) return rc;
    if (p->x_row_stride < p->K || p->y_row_stride < p->N)
        return fail(HYD_ERR_BAD_ARG, "x_row_stride %lld < K %d or y_row_stride %lld < N %d", (long long)p->x_row_stride, p->K, (long long)p->y_row_stride, p->N);
    const LinearW8Plan pl = plan_linear_w8(p->M, p->N, p->K);
    if ((int64_t)pl.ngroups * pl.mtiles > 0x7fffffffLL || ((int64_t)p->M * (pl.np / 4) + 255) / 256 > 0x7fffffffLL)
        return fail(HYD_ERR_UNSUPPORTED, "M %d x N %d: more workgroups than one launch takes", p->M, p->N);
    if (pl.bytes) {
        if (!p->workspace || p->workspace_bytes < pl.bytes)
            return fail(HYD_ERR_WORKSPACE, "linear_w8 needs %zu workspace bytes for M %d N %d K %d, got %zu", pl.bytes, p->M, p->N, p->K, p->workspace ? p->workspace_bytes : (size_t)0);
        if (misaligned(p->workspace, 16)) return fail(HYD_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    }
    LinearW8Args a;
    memset(&a, 0, sizeof(a));
    a.x = p->x; a.w8 = static_cast<const uint8_t*>(p->w8); a.scale = p->scale; a.y = p->y;
    a.ws = pl.bytes ? static_cast<float*>(p->workspace) : nullptr;
    a.xs = p->x_row_stride; a.ys = p->y_row_stride; a.np = pl.np;
    a.M = p->M; a.N = p->N; a.K = p->K;
    a.mtiles = pl.mtiles; a.steps = pl.steps; a.splits = pl.splits;
    return launched(launch_linear_w8(a, pl, p->dtype, static_cast<hipStream_t>(stream)), "linear_w8 kernel launch");
}

int hyd_weight_widen(const hyd_weight_widen_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (int rc = check_w8_common(p->w8, p->scale, p->N, p->K, p->dtype, 8)) return rc;
    if (int rc = check_ptr_align(p->out, "out")) return rc;
    if (int rc = check_stride8(p->out_row_stride, "out_row_stride")) return rc;
    if (p->out_row_stride < p->K) return fail(HYD_ERR_BAD_ARG, "out_row_stride %lld < K %d", (long long)p->out_row_stride, p->K);
    WeightWidenArgs a;
    memset(&a, 0, sizeof(a));
    a.w8 = static_cast<const uint8_t*>(p->w8); a.scale = p->scale; a.out = p->out; a.os = p->out_row_stride;
    a.N = p->N; a.K = p->K;
    return launched(launch_weight_widen(a, p->dtype, static_cast<hipStream_t>(stream)), "weight_widen kernel launch");
}

int hyd_ipc_get_handle(const void* dev_ptr, void* handle_out) {
    static_assert(sizeof(hipIpcMemHandle_t) == HYD_IPC_HANDLE_BYTES, "IPC handle size");
    if (!dev_ptr || !handle_out) return fail(HYD_ERR_BAD_ARG, "null pointer");
    hipIpcMemHandle_t h;
    const hipError_t e = hipIpcGetMemHandle(&h, const_cast<void*>(dev_ptr));
    if (e != hipSuccess) return fail(HYD_ERR_LAUNCH, "hipIpcGetMemHandle: %s", hipGetErrorString(e));
    memcpy(handle_out, &h, sizeof(h));
    return HYD_OK;
}

int hyd_ipc_open_handle(const void* handle, void** dev_ptr_out) {
    if (!handle || !dev_ptr_out) return fail(HYD_ERR_BAD_ARG, "null pointer");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    const hipError_t e = hipIpcOpenMemHandle(dev_ptr_out, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(HYD_ERR_LAUNCH, "hipIpcOpenMemHandle: %s", hipGetErrorString(e));
    return HYD_OK;
}

int hyd_ipc_close_handle(void* dev_ptr) {
    if (!dev_ptr) return fail(HYD_ERR_BAD_ARG, "null pointer");
    const hipError_t e = hipIpcCloseMemHandle(dev_ptr);
    return e == hipSuccess ? HYD_OK : fail(HYD_ERR_LAUNCH, "hipIpcCloseMemHandle: %s", hipGetErrorString(e));
}

size_t hyd_allreduce_block_bytes(int32_t world, size_t max_bytes) {
    if (world < 1 || world > HYD_ALLREDUCE_MAX_WORLD || max_bytes == 0) return 0;
    return allreduce_block_bytes(world, max_bytes);
}

const uint32_t* hyd_allreduce_status(const void* own_block) {
    // layout of allreduce.hip: 2 x 8 flags of 32 words, then the local words {epoch, arrivals, status}
    return own_block ? static_cast<const uint32_t*>(own_block) + 2 * HYD_ALLREDUCE_MAX_WORLD * 32 + 2 : nullptr;
}

int hyd_allreduce_sum(const hyd_allreduce_params* p, void* stream) {
    if (!p || !p->blocks) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->world < 1 || p->world > HYD_ALLREDUCE_MAX_WORLD) return fail(HYD_ERR_UNSUPPORTED, "world %d (1..%d)", p->world, HYD_ALLREDUCE_MAX_WORLD);
    if (p->rank < 0 || p->rank >= p->world) return fail(HYD_ERR_BAD_ARG, "rank %d of %d", p->rank, p->world);
    if (p->dtype != HYD_F16 && p->dtype != HYD_BF16 && p->dtype != HYD_F32) return fail(HYD_ERR_UNSUPPORTED, "dtype %d", p->dtype);
    if (p->count < 0) return fail(HYD_ERR_BAD_ARG, "count %lld", (long long)p->count);
    if (p->timeout_log2_polls != 0 && (p->timeout_log2_polls < 10 || p->timeout_log2_polls > 31))
        return fail(HYD_ERR_BAD_ARG, "timeout_log2_polls %d (0 = default, or 10..31)", p->timeout_log2_polls);
    if (p->count == 0) return HYD_OK;
    const size_t bytes = (size_t)p->count * (p->dtype == HYD_F32 ? 4 : 2);
    if (bytes > p->max_bytes) return fail(HYD_ERR_WORKSPACE, "%zu bytes exceed the blocks' max_bytes %zu", bytes, p->max_bytes);
    int rc;
    if ((rc = check_ptr_align(p->in, "in")) || (rc = check_ptr_align(p->out, "out"))) return rc;
    char* blocks[HYD_ALLREDUCE_MAX_WORLD];
    for (int i = 0; i < p->world; ++i) {
        if ((rc = check_ptr_align(p->blocks[i], "block"))) return rc;
        blocks[i] = static_cast<char*>(p->blocks[i]);
    }
    if (p->world == 1) {
        if (p->in != p->out) (void)hipMemcpyAsync(p->out, p->in, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
        return HYD_OK;
    }
    return launched(launch_allreduce(blocks, allreduce_block_bytes(p->world, p->max_bytes), p->in, p->out, p->count, p->dtype, p->rank,
                                     p->world, p->max_bytes, p->timeout_log2_polls, static_cast<hipStream_t>(stream)),
                    "all-reduce kernel launch");
}

size_t hyd_decode_workspace_bytes(const hyd_decode_params* p) {
    if (!p || !levels_in_range(p)) return 0;
    DecodePlan d;
    plan_decode(p, &d);
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

static int decode_impl(const hyd_decode_params* p, const hyd_kv_quant* kq, void* stream);

// Shapes only: a grouped-query fp8 call whose 16-bit twin would run as ONE launch (decode_runs_as_one_launch).  The one-launch walk
// does not round a 16-bit prefix partial, the two-kernel pair does: the pair is not what the caller's 16-bit results are, so such a
// call is refused instead of quietly run as the pair.  (Hq == Hkv shapes keep ignoring the flag, as they always have.)
static bool decode_kvq_is_one_launch(const hyd_decode_params* p, const hyd_kv_quant* kq) {
    if (!levels_in_range(p) || !kvq_native_gqa(&p->suffix, kq)) return false;
    DecodePlan d;
    plan_decode(p, &d);
    return !d.rc && d.form == kOneLaunch;  // (a level that does not plan: decode_impl reports it)
}

int hyd_decode_attn_fused(const hyd_decode_params* p, void* stream) { return decode_impl(p, nullptr, stream); }

int hyd_decode_attn_fused_kvq(const hyd_decode_params* p, const hyd_kv_quant* kq, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_suffix(&p->suffix, true);
    if (rc) return rc;
    if ((rc = check_kvq(&kq, p->suffix.dtype))) return rc;
    if (!kq) return decode_impl(p, nullptr, stream);
    // fp8 unique caches: validated up front (every phase, also those that do not read the unique cache) so that the phases of one
    // call agree; kv_len == 0 reads no unique key and takes the existing path
    if (p->suffix.kv_len > 0 && narrow_kv_dim(&p->suffix)) return fail_narrow_fp8();
    if (p->suffix.kv_len > 0 && !kvq_native(&p->suffix, kq)) return fail_kvq_shapes(p->suffix.D);
    if (decode_kvq_is_one_launch(p, kq))
        return fail(HYD_ERR_UNSUPPORTED, "fp8 unique caches: a grouped-query call this small runs as ONE launch with 16-bit caches "
                                         "(single_launch_small), which has no fp8 form: clear the flag, or pass 16-bit caches");
    return decode_impl(p, p->suffix.kv_len > 0 ? kq : nullptr, stream);
}

int hyd_decode_kv_quant_supported(const hyd_decode_params* p, const hyd_kv_quant* kq) {
    if (!p) return 0;
    const KvqKind kind = kvq_kind(kq, p->suffix.dtype);
    if (kind != kKvqFp8) return kind == kKvqNone ? 1 : 0;
    if (!levels_in_range(p)) return 0;
    if (p->suffix.kv_len <= 0) return p->suffix.kv_len == 0 ? 1 : 0;  // no unique key is read: the existing path
    return kvq_native(&p->suffix, kq) && !decode_kvq_is_one_launch(p, kq) ? 1 : 0;
}

// kq: null, or validated fp8 unique caches (then the unique pass is an fp8 kernel and the call is never the one-launch form: Hq == Hkv
// shapes ignore single_launch_small, grouped-query ones were refused by the caller where the flag would have applied)
static int decode_impl(const hyd_decode_params* p, const hyd_kv_quant* kq, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (!levels_in_range(p)) return fail(HYD_ERR_BAD_ARG, "n_levels %d", p->n_levels);
    if (p->phase < HYD_PHASE_ALL || p->phase > HYD_PHASE_MERGE) return fail(HYD_ERR_BAD_ARG, "phase %d", p->phase);
    if (p->shared_max_workgroups < 0) return fail(HYD_ERR_BAD_ARG, "shared_max_workgroups %d", p->shared_max_workgroups);
    if (p->f32_partials != 0 && p->f32_partials != 1) return fail(HYD_ERR_BAD_ARG, "f32_partials %d", p->f32_partials);
    const hyd_suffix_params& sp = p->suffix;
    int rc = check_suffix(&sp, true);
    if (rc) return rc;
    if (p->n_levels == 0 && sp.kv_len == 0) return fail(HYD_ERR_BAD_ARG, "no shared levels and no unique keys");
    if (narrow_kv_dim(&sp) && sp.kv_len > 0) {  // refused before the first launch, in every phase, so that the phases of one call agree
        if (kq) return fail_narrow_fp8();
        if (!narrow_native(&sp)) return fail_narrow_shapes(&sp);
    }
    if (p->causal_tail != 0 && p->causal_tail != 1) return fail(HYD_ERR_BAD_ARG, "causal_tail %d", p->causal_tail);
    const bool causal = p->causal_tail != 0;
    if (causal && (rc = check_causal_tail(&sp, kq))) return rc;  // in every phase, so that the phases of one call agree
    if (causal && sp.kv_len > 0) {  // ... and so is a shape no kernel with the per-row key limit takes: before the level passes go out
        SuffixArgs ca;
        fill_suffix_args(&sp, &ca);
        if (!suffix_causal_eligible(ca, sp.D)) return fail_causal_shapes();
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rows = (size_t)sp.B * sp.nq * sp.Hq;
    const bool do_shared = p->phase == HYD_PHASE_ALL || p->phase == HYD_PHASE_SHARED;
    const bool do_unique = p->phase == HYD_PHASE_ALL || p->phase == HYD_PHASE_UNIQUE;
    DecodePlan d;
    plan_decode(p, &d);
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
        SuffixArgs a;
        fill_suffix_args(&sp, &a);
        a.pk = pp.k; a.pv = pp.v;
        a.pk_gs = pp.k_group_stride; a.pk_hs = pp.k_head_stride;
        a.pv_gs = pp.v_group_stride; a.pv_hs = pp.v_head_stride;
        a.p_len = pp.kv_len;
        a.p_per = sp.B / pp.sb;
        a.shared_kv = 1;  // p_per sequences read the same prefix keys: default cache policy, not the read-once hint
        return launched(launch_suffix_gqa(a, sp.dtype, sp.D, s), "single-launch decode kernel");
    }
    const size_t need = d.levels_bytes + (two_stream ? d.unique.bytes : 0);
    if (need > 0 && (!p->workspace || p->workspace_bytes < need))
        return fail(HYD_ERR_WORKSPACE, "decode needs %zu workspace bytes, got %zu", need, p->workspace_bytes);

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
            hyd_suffix_params su = sp;
            su.out = u_out;
            su.lse = u_lse;
            return run_suffix(&su, nullptr, 0, s, kq, causal);
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
    if (sp.kv_len == 0) {
        // several levels, no unique keys: merge the level partials only (suffix contributes lse = -inf)
        hyd_suffix_params s0 = sp;
        s0.seq_lens_i32 = nullptr;
        s0.seq_lens_i64 = nullptr;
        return run_suffix(&s0, parts, p->n_levels, s);
    }
    return run_suffix(&sp, parts, p->n_levels, s, kq, causal);
}

int hyd_decode_two_stream_ok(const hyd_decode_params* p) {
    if (!p || !levels_in_range(p)) return 0;
    DecodePlan d;
    plan_decode(p, &d);
    return d.two_stream_ok ? 1 : 0;
}

}  // extern "C"
