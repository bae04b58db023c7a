// C ABI, work on whole K/V caches: promoting unique rows to a shared level (fork), gathering whole paths into one level, and the
// fp8 scale calibration (absolute maxima, scales from them).
#include "api_core.h"

using namespace hyd;

namespace {

// hyd_kv_promote_params and hyd_kv_gather_params describe the unique segment with the same fields, but for the name of the destination
// offsets (cu / cu_dst).  The gather call's n_levels and max_path are checked between them; a promote is a path of no levels with no
// bound of its own (0, 0: both pass).
template <typename P>
int check_kv_unique(const P* p, const int32_t* cu, const char* cu_name, int n_levels, int max_path) {
    if (p->dst_dtype != HYD_F16 && p->dst_dtype != HYD_BF16)
        return fail(HYD_ERR_UNSUPPORTED, "dst_dtype %d: shared levels are f16 / bf16 (no fp8 or 32-bit destination)", p->dst_dtype);
    if (p->src_dtype != HYD_F16 && p->src_dtype != HYD_BF16 && p->src_dtype != HYD_FP8_E4M3)
        return fail(HYD_ERR_UNSUPPORTED, "src_dtype %d: f16, bf16 or HYD_FP8_E4M3 (%d)", p->src_dtype, HYD_FP8_E4M3);
    if (p->src_dtype != HYD_FP8_E4M3 && p->src_dtype != p->dst_dtype)
        return fail(HYD_ERR_BAD_ARG, "src_dtype %d differs from dst_dtype %d: a 16-bit source is copied as bytes", p->src_dtype, p->dst_dtype);
    if (p->n <= 0) return fail(HYD_ERR_BAD_ARG, "n %d must be > 0", p->n);
    if (n_levels < 0 || n_levels > HYD_MAX_LEVELS) return fail(HYD_ERR_BAD_ARG, "n_levels %d outside [0, %d]", n_levels, HYD_MAX_LEVELS);
    if (p->Hkv <= 0) return fail(HYD_ERR_BAD_ARG, "Hkv %d must be > 0", p->Hkv);
    if (p->B <= 0 || p->src_rows <= 0 || p->capacity < 0)
        return fail(HYD_ERR_BAD_ARG, "B %d / src_rows %d must be > 0, capacity %d >= 0", p->B, p->src_rows, p->capacity);
    if (p->d_src <= 0 || p->d_src % 8 != 0) return fail(HYD_ERR_BAD_ARG, "d_src %d must be a positive multiple of 8 (16-byte vectors)", p->d_src);
    if (p->d_dst < p->d_src) return fail(HYD_ERR_BAD_ARG, "d_dst %d < d_src %d", p->d_dst, p->d_src);
    if (p->d_dst != p->d_src && p->d_dst != 64 && p->d_dst != 128 && p->d_dst != 256)
        return fail(HYD_ERR_UNSUPPORTED, "d_dst %d: 64, 128, 256 or d_src (%d)", p->d_dst, p->d_src);
    if (p->max_len < 0 || p->max_len > p->src_rows) return fail(HYD_ERR_BAD_ARG, "max_len %d outside [0, src_rows = %d]", p->max_len, p->src_rows);
    if (max_path < 0 || max_path > p->capacity) return fail(HYD_ERR_BAD_ARG, "max_path %d outside [0, capacity = %d]", max_path, p->capacity);
    if (p->n > 65535) return fail(HYD_ERR_UNSUPPORTED, "n %d: up to 65535 sequences per launch", p->n);
    int rc = check_ptrs_align({{p->k_src, "k_src"}, {p->v_src, "v_src"}, {p->k_dst, "k_dst"}, {p->v_dst, "v_dst"}});
    if (!rc) rc = check_not_null({{p->rows, "rows"}, {p->lens, "lens"}, {cu, cu_name}});
    if (!rc) rc = check_elem_align({{p->rows, 4, "rows"}, {p->lens, 4, "lens"}, {cu, 4, cu_name}, {p->k_scale, 4, "k_scale"}, {p->v_scale, 4, "v_scale"}});
    if (!rc) rc = check_strides8({{p->k_batch_stride, "k_batch_stride"}, {p->k_tok_stride, "k_tok_stride"}, {p->k_head_stride, "k_head_stride"},
                                  {p->v_batch_stride, "v_batch_stride"}, {p->v_tok_stride, "v_tok_stride"}, {p->v_head_stride, "v_head_stride"}});
    if (rc) return rc;
    if (p->Hkv > 1 && (p->k_head_stride < p->d_src || p->v_head_stride < p->d_src))
        return fail(HYD_ERR_BAD_ARG, "k_head_stride %lld / v_head_stride %lld < d_src %d", (long long)p->k_head_stride, (long long)p->v_head_stride, p->d_src);
    return HYD_OK;
}

// ... and its last check, the 32-bit vector index within a sequence, with the argument block of the unique segment
template <typename P>
int fill_kv_promote_args(const P* p, const int32_t* cu, KvPromoteArgs* ap) {
    KvPromoteArgs& a = *ap;
    const int max_len = p->max_len ? p->max_len : p->src_rows;
    const int64_t vec_per_tok = (int64_t)p->Hkv * (p->d_dst / 8);
    if (vec_per_tok * max_len >= (1LL << 31))
        return fail(HYD_ERR_UNSUPPORTED, "max_len %d x Hkv %d x d_dst %d: a sequence of more than 2^31 16-byte vectors", max_len, p->Hkv, p->d_dst);
    a.k_src = p->k_src; a.v_src = p->v_src; a.k_dst = p->k_dst; a.v_dst = p->v_dst;
    a.rows = p->rows; a.lens = p->lens; a.cu = cu;
    if (p->src_dtype == HYD_FP8_E4M3) { a.k_scale = p->k_scale; a.v_scale = p->v_scale; }
    a.k_bs = p->k_batch_stride; a.k_ts = p->k_tok_stride; a.k_hs = p->k_head_stride;
    a.v_bs = p->v_batch_stride; a.v_ts = p->v_tok_stride; a.v_hs = p->v_head_stride;
    a.n = p->n; a.B = p->B; a.max_len = max_len; a.capacity = p->capacity; a.d_src = p->d_src;
    a.vec_per_head = p->d_dst / 8; a.vec_per_tok = (int32_t)vec_per_tok;
    a.div_vec_per_head = make_fastdiv((uint32_t)a.vec_per_head);
    a.div_vec_per_tok = make_fastdiv((uint32_t)a.vec_per_tok);
    return HYD_OK;
}

}  // namespace

extern "C" {

int hyd_kv_promote(const hyd_kv_promote_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_kv_unique(p, p->cu, "cu", 0, 0);
    if (rc) return rc;
    KvPromoteArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = fill_kv_promote_args(p, p->cu, &a))) return rc;
    return launched(launch_kv_promote(a, p->src_dtype, p->dst_dtype, static_cast<hipStream_t>(stream)), "kv_promote kernel launch");
}

int hyd_kv_gather_paths(const hyd_kv_gather_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_kv_unique(p, p->cu_dst, "cu_dst", p->n_levels, p->max_path);
    if (rc) return rc;
    for (int j = 0; j < p->n_levels; ++j) {
        char name[32];
        snprintf(name, sizeof(name), "level_k[%d]", j);
        if ((rc = check_ptr_align(p->level_k[j], name))) return rc;
        snprintf(name, sizeof(name), "level_v[%d]", j);
        if ((rc = check_ptr_align(p->level_v[j], name))) return rc;
        if (!p->level_cu[j] || misaligned(p->level_cu[j], 4)) return fail(HYD_ERR_BAD_ARG, "level_cu[%d] is null or not 4-byte aligned", j);
        if (p->level_div[j] <= 0) return fail(HYD_ERR_BAD_ARG, "level_div[%d] = %d must be > 0 (old_batch / s_j)", j, p->level_div[j]);
        if (p->level_s[j] <= 0 || p->level_cap[j] < 0)
            return fail(HYD_ERR_BAD_ARG, "level_s[%d] = %d must be > 0, level_cap[%d] = %d >= 0", j, p->level_s[j], j, p->level_cap[j]);
    }
    KvGatherArgs g;
    memset(&g, 0, sizeof(g));
    if ((rc = fill_kv_promote_args(p, p->cu_dst, &g.u))) return rc;
    const int max_path = p->max_path ? p->max_path : p->capacity;
    if ((int64_t)g.u.vec_per_tok * max_path >= (1LL << 31))  // (vec_per_tok is exact in 32 bits: one row of max_len >= 1 passed above)
        return fail(HYD_ERR_UNSUPPORTED, "max_path %d x Hkv %d x d_dst %d: a path of more than 2^31 16-byte vectors", max_path, p->Hkv, p->d_dst);
    if (max_path == 0) return HYD_OK;  // (an empty destination: nothing can be written)
    for (int j = 0; j < p->n_levels; ++j) {
        g.lk[j] = p->level_k[j]; g.lv[j] = p->level_v[j]; g.lcu[j] = p->level_cu[j];
        g.ls[j] = p->level_s[j]; g.lcap[j] = p->level_cap[j];
        g.ldiv[j] = make_fastdiv((uint32_t)p->level_div[j]);
    }
    g.n_levels = p->n_levels; g.max_path = max_path;
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
    int rc = check_elem_align({{p->amax, 4, "amax"}, {p->row_lens, 4, "row_lens"}});
    if (!rc && p->k) rc = check_strides8({{p->k_outer_stride, "k_outer_stride"}, {p->k_row_stride, "k_row_stride"}, {p->k_head_stride, "k_head_stride"}});
    if (!rc && p->v) rc = check_strides8({{p->v_outer_stride, "v_outer_stride"}, {p->v_row_stride, "v_row_stride"}, {p->v_head_stride, "v_head_stride"}});
    if (rc) return rc;
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
    int rc = check_not_null({{p->amax, "amax"}, {p->k_scale, "k_scale"}, {p->v_scale, "v_scale"}});
    if (!rc) rc = check_elem_align({{p->amax, 4, "amax"}, {p->k_scale, 4, "k_scale"}, {p->v_scale, 4, "v_scale"}});
    if (rc) return rc;
    if (p->Hkv < 1) return fail(HYD_ERR_BAD_ARG, "Hkv %d must be >= 1", p->Hkv);
    if (!(p->c > 0.f) || std::isinf(p->c)) return fail(HYD_ERR_BAD_ARG, "c %g must be finite and positive (margin / 448)", (double)p->c);
    KvScalesArgs a;
    memset(&a, 0, sizeof(a));
    a.amax = p->amax; a.k_scale = p->k_scale; a.v_scale = p->v_scale;
    a.Hkv = p->Hkv; a.pow2 = p->pow2 ? 1 : 0; a.c = p->c;
    return launched(launch_kv_scales(a, static_cast<hipStream_t>(stream)), "kv_scales kernel launch");
}

}  // extern "C"
