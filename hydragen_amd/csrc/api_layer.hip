// C ABI, the layer around attention: RoPE + cache append (one token, fp8 caches, several tokens), add + RMSNorm, SwiGLU, and the
// fp8 linear-layer weights (linear_w8.hip).
#include "api_core.h"

using namespace hyd;

namespace {

// What the one-token and the multi-token form check alike, from the pointers on.  Between the shared parts each form has its own:
// the index arrays whose alignment it checks (the one-token form: none) and the strides of its q / k / v inputs.
template <typename P>
int check_rope(const P* p, std::initializer_list<SizedPtr> index_arrays, std::initializer_list<NamedStride> input_strides) {
    int rc = check_ptrs_align({{p->q, "q"}, {p->k, "k"}, {p->v, "v"}, {p->q_out, "q_out"}, {p->k_cache, "k_cache"}, {p->v_cache, "v_cache"},
                               {p->cos, "cos"}, {p->sin, "sin"}});
    if (!rc) rc = check_not_null({{p->position_ids, "position_ids"}, {p->seq_lens, "seq_lens"}});
    if (!rc) rc = check_elem_align(index_arrays);
    if (!rc) rc = check_strides8(input_strides);
    if (!rc) rc = check_strides8({{p->kc_batch_stride, "kc_batch_stride"}, {p->kc_tok_stride, "kc_tok_stride"}, {p->kc_head_stride, "kc_head_stride"},
                                  {p->vc_batch_stride, "vc_batch_stride"}, {p->vc_tok_stride, "vc_tok_stride"}, {p->vc_head_stride, "vc_head_stride"}});
    if (rc) return rc;
    if (p->cs_stride % 4 != 0) return fail(HYD_ERR_BAD_ARG, "cos/sin row stride must be a multiple of 4 floats");
    if (p->cache_len <= 0) return fail(HYD_ERR_BAD_ARG, "cache_len %d", p->cache_len);
    if (p->max_pos <= 0) return fail(HYD_ERR_BAD_ARG, "max_pos %d: the cos/sin tables need at least one row", p->max_pos);
    return HYD_OK;
}

// hyd_qk_norm beside a call whose kernels run at head dim D on rows of `head_dim` (0 or D: native) elements
int check_qk_norm(const hyd_qk_norm* qn, int head_dim, int D) {
    if (!qn) return HYD_OK;
    if (int rc = check_ptrs_align({{qn->q_weight, "q_weight"}, {qn->k_weight, "k_weight"}})) return rc;
    if (!std::isfinite(qn->eps) || qn->eps <= 0.f) return fail(HYD_ERR_BAD_ARG, "qk_norm eps %g must be finite and > 0", (double)qn->eps);
    if (qn->flags != 0) return fail(HYD_ERR_BAD_ARG, "qk_norm flags %d must be 0", qn->flags);
    if (head_dim != 0 && head_dim != D)
        return fail(HYD_ERR_UNSUPPORTED, "qk_norm with head_dim %d: the per-head norm is implemented for rows of D = %d elements (64 / 128 / 256) only", head_dim, D);
    return HYD_OK;
}

// RopeArgs from either public struct: what the one-token and the multi-token form name alike, and the norm's gains.  Each form
// adds its own fields: fp8 scales and a narrow row width, or T and the token strides.
template <typename P>
RopeArgs rope_args(const P* p, const hyd_qk_norm* qn) {
    RopeArgs a;
    a.q = p->q; a.k = p->k; a.v = p->v; a.q_out = p->q_out; a.k_cache = p->k_cache; a.v_cache = p->v_cache;
    a.cos = p->cos; a.sin = p->sin; a.pos = p->position_ids; a.shared_len = p->shared_len; a.seq_lens = p->seq_lens;
    a.q_bs = p->q_batch_stride; a.k_bs = p->k_batch_stride; a.v_bs = p->v_batch_stride;
    a.kc_bs = p->kc_batch_stride; a.kc_ts = p->kc_tok_stride; a.kc_hs = p->kc_head_stride;
    a.vc_bs = p->vc_batch_stride; a.vc_ts = p->vc_tok_stride; a.vc_hs = p->vc_head_stride;
    a.pos_stride = p->pos_stride; a.cs_stride = p->cs_stride;
    a.B = p->B; a.Hq = p->Hq; a.Hkv = p->Hkv; a.cache_len = p->cache_len; a.max_pos = p->max_pos;
    a.D = a.d = p->D;
    if (qn) {
        a.q_weight = qn->q_weight;
        a.k_weight = qn->k_weight;
        a.eps = qn->eps;
    }
    return a;
}

int check_w8_common(const void* w8, const float* scale, int32_t N, int32_t K, int32_t dtype, int k_multiple) {
    if (dtype != HYD_F16 && dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d: f16 / bf16 activations (the weights are e4m3fn)", dtype);
    if (N < 1 || K < 1) return fail(HYD_ERR_BAD_ARG, "N %d / K %d must be >= 1", N, K);
    if (K % k_multiple != 0) return fail(HYD_ERR_BAD_ARG, "K %d must be a multiple of %d", K, k_multiple);
    if (int rc = check_ptr_align(w8, "w8")) return rc;
    if (int rc = check_not_null({{scale, "scale"}})) return rc;
    return check_elem_align({{scale, 4, "scale"}});
}

}  // namespace

extern "C" {

int hyd_rope_append_decode_qkn(const hyd_rope_params* p, const hyd_kv_quant* kq, const hyd_qk_norm* qn, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_common(p->dtype, p->B, 1, p->Hq, p->Hkv, p->D);
    if (rc) return rc;
    if ((rc = check_narrow_dim(p->head_dim, p->D, "head_dim"))) return rc;
    if ((rc = check_kvq(&kq, p->dtype))) return rc;
    const int narrow = p->head_dim != p->D ? p->head_dim : 0;
    if (narrow && kq) return fail_narrow_fp8();
    if ((rc = check_rope(p, {}, {{p->q_batch_stride, "q_batch_stride"}, {p->k_batch_stride, "k_batch_stride"}, {p->v_batch_stride, "v_batch_stride"}})))
        return rc;
    if ((rc = check_qk_norm(qn, p->head_dim, p->D))) return rc;
    RopeArgs a = rope_args(p, qn);
    if (narrow) a.d = narrow;
    if (kq) {
        a.fp8 = 1;
        a.k_scale = kq->k_scale;
        a.v_scale = kq->v_scale;
    }
    return launched(launch_rope_append(a, p->dtype, static_cast<hipStream_t>(stream)),
                    qn ? "rope_append (q/k norm) kernel launch" : narrow ? "rope_append (narrow head dim) kernel launch"
                    : kq ? "rope_append (fp8 caches) kernel launch" : "rope_append kernel launch");
}

int hyd_rope_append_decode_kvq(const hyd_rope_params* p, const hyd_kv_quant* kq, void* stream) { return hyd_rope_append_decode_qkn(p, kq, nullptr, stream); }

int hyd_rope_append_decode(const hyd_rope_params* p, void* stream) { return hyd_rope_append_decode_qkn(p, nullptr, nullptr, stream); }

int hyd_rope_append_multi_kvq(const hyd_rope_multi_params* p, const hyd_kv_quant* kq, const hyd_qk_norm* qn, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->T < 2 || p->T > 8) return fail(HYD_ERR_BAD_ARG, "T = %d tokens per row, 2 to 8 are taken (hyd_rope_append_decode takes one)", p->T);
    int rc = check_common(p->dtype, p->B, p->T, p->Hq, p->Hkv, p->D);
    if (rc) return rc;
    if ((rc = check_kvq(&kq, p->dtype))) return rc;  // (where the one-token form checks it: behind the shapes, in front of the pointers)
    if ((rc = check_rope(p, {{p->position_ids, 8, "position_ids"}, {p->shared_len, 8, "shared_len"}, {p->seq_lens, 4, "seq_lens"}},
                         {{p->q_batch_stride, "q_batch_stride"}, {p->k_batch_stride, "k_batch_stride"}, {p->v_batch_stride, "v_batch_stride"},
                          {p->q_tok_stride, "q_tok_stride"}, {p->k_tok_stride, "k_tok_stride"}, {p->v_tok_stride, "v_tok_stride"}})))
        return rc;
    if ((rc = check_qk_norm(qn, 0, p->D))) return rc;
    RopeArgs a = rope_args(p, qn);
    a.T = p->T;
    a.q_ts = p->q_tok_stride; a.k_ts = p->k_tok_stride; a.v_ts = p->v_tok_stride;
    if (kq) {
        a.fp8 = 1;
        a.k_scale = kq->k_scale;
        a.v_scale = kq->v_scale;
    }
    return launched(launch_rope_append(a, p->dtype, static_cast<hipStream_t>(stream)),
                    qn ? "rope_append (multi-token, q/k norm) kernel launch"
                    : kq ? "rope_append (multi-token, fp8 caches) kernel launch" : "rope_append (multi-token) kernel launch");
}

int hyd_rope_append_multi_qkn(const hyd_rope_multi_params* p, const hyd_qk_norm* qn, void* stream) { return hyd_rope_append_multi_kvq(p, nullptr, qn, stream); }

int hyd_rope_append_multi(const hyd_rope_multi_params* p, void* stream) { return hyd_rope_append_multi_kvq(p, nullptr, nullptr, stream); }

int hyd_add_rmsnorm(const hyd_add_rmsnorm_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->dtype != HYD_F16 && p->dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d (fp16 / bf16)", p->dtype);
    if (p->rows < 0 || p->rows > 0x7fffffff) return fail(HYD_ERR_BAD_ARG, "rows %lld", (long long)p->rows);
    if (p->n <= 0 || p->n % 8 != 0 || p->n > 16384) return fail(HYD_ERR_UNSUPPORTED, "n %d: a multiple of 8 up to 16384", p->n);
    int rc = check_not_null({{p->x, "x"}, {p->weight, "weight"}, {p->norm_out, "norm_out"}});
    if (!rc) rc = check_ptrs_align({{p->x, "x"}, {p->weight, "weight"}, {p->norm_out, "norm_out"}});
    if (!rc) rc = check_strides8({{p->x_row_stride, "x_row_stride"}, {p->norm_row_stride, "norm_row_stride"}});
    if (rc) return rc;
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
    int rc = check_not_null({{p->gate, "gate"}, {p->up, "up"}, {p->out, "out"}});
    if (!rc) rc = check_ptrs_align({{p->gate, "gate"}, {p->up, "up"}, {p->out, "out"}});
    if (!rc) rc = check_strides8({{p->gate_row_stride, "gate_row_stride"}, {p->up_row_stride, "up_row_stride"}, {p->out_row_stride, "out_row_stride"}});
    if (rc) return rc;
    SwigluArgs a;
    memset(&a, 0, sizeof(a));
    a.gate = p->gate; a.up = p->up; a.out = p->out;
    a.g_rs = p->gate_row_stride; a.u_rs = p->up_row_stride; a.o_rs = p->out_row_stride;
    a.rows = p->rows; a.n = p->n;
    return launched(launch_swiglu(a, p->dtype, static_cast<hipStream_t>(stream)), "swiglu kernel launch");
}

size_t hyd_linear_w8_workspace_bytes(int32_t M, int32_t N, int32_t K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    return plan_linear_w8(M, N, K).bytes;
}

int hyd_linear_w8(const hyd_linear_w8_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->M < 1) return fail(HYD_ERR_BAD_ARG, "M %d must be >= 1", p->M);
    int rc = check_w8_common(p->w8, p->scale, p->N, p->K, p->dtype, 16);
    if (!rc) rc = check_ptrs_align({{p->x, "x"}, {p->y, "y"}});
    if (!rc) rc = check_strides8({{p->x_row_stride, "x_row_stride"}, {p->y_row_stride, "y_row_stride"}});
    if (rc) return rc;
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

}  // extern "C"
