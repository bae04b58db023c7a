// C ABI, the mixture-of-experts MLP (moe.hip, moe_w8.hip): hyd_moe_workspace_bytes, hyd_moe_mlp, hyd_moe_mlp_w8,
// hyd_moe_mlp_w4 (moe_w4.hip), hyd_moe_grouped_workspace_bytes and hyd_moe_mlp_grouped (moe_grouped.hip), hyd_moe_mlp_grouped_w8
// (moe_grouped_w8.hip).
#include "api_core.h"

using namespace hyd;

namespace {

// the ranges of moe.hip (max_rows = kMoeMaxRows) and of moe_grouped.hip (kMoeGroupedMaxRows); `say` false: the size query's silent form
int check_moe_shapes(int T, int E, int k, int H, int I, int dtype, bool say, int max_rows = kMoeMaxRows) {
    const bool ok_dtype = dtype == HYD_F16 || dtype == HYD_BF16;
    const bool ok = T >= 1 && T <= max_rows && E >= 1 && E <= kMoeMaxExperts && k >= 1 && k <= kMoeMaxTopK && k <= E && H >= 64 && H % 64 == 0 &&
                    I >= 32 && I % 32 == 0;
    if (!say) return ok && ok_dtype ? HYD_OK : HYD_ERR_BAD_ARG;
    if (!ok_dtype) return fail(HYD_ERR_UNSUPPORTED, "dtype %d: f16 / bf16 activations and expert weights", dtype);
    if (T < 1 || T > max_rows) return fail(HYD_ERR_BAD_ARG, "T %d: 1 to %d rows per call (longer inputs are chunked by the caller)", T, max_rows);
    if (E < 1 || E > kMoeMaxExperts) return fail(HYD_ERR_BAD_ARG, "E %d: 1 to %d experts", E, kMoeMaxExperts);
    if (k < 1 || k > kMoeMaxTopK) return fail(HYD_ERR_BAD_ARG, "k %d: 1 to %d experts per row", k, kMoeMaxTopK);
    if (k > E) return fail(HYD_ERR_BAD_ARG, "k %d exceeds E %d", k, E);
    if (H < 64 || H % 64 != 0) return fail(HYD_ERR_BAD_ARG, "H %d must be a positive multiple of 64", H);
    if (I < 32 || I % 32 != 0) return fail(HYD_ERR_BAD_ARG, "I %d must be a positive multiple of 32", I);
    return HYD_OK;
}

// the checks and the kernel arguments that hyd_moe_params, hyd_moe_w8_params and hyd_moe_w4_params share (P: either; the fields carry the same names);
// `grouped`: hyd_moe_mlp_grouped's range of T and its workspace slices (the tile table goes to grouped->tiles), `grouped_name`: the grouped call's
// name in the workspace message
template <typename P>
int moe_args(const P* p, MoeArgs& a, MoeGroupedArgs* grouped = nullptr, const char* grouped_name = "moe_mlp_grouped") {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_moe_shapes(p->T, p->E, p->k, p->H, p->I, p->dtype, true, grouped ? kMoeGroupedMaxRows : kMoeMaxRows);
    if (rc) return rc;
    if (p->renormalize != 0 && p->renormalize != 1) return fail(HYD_ERR_BAD_ARG, "renormalize %d must be 0 or 1", p->renormalize);
    if ((rc = check_ptrs_align({{p->x, "x"}, {p->gate_up, "gate_up"}, {p->down, "down"}, {p->y, "y"}}))) return rc;
    if ((rc = check_not_null({{p->logits, "logits"}}))) return rc;
    if ((rc = check_elem_align({{p->logits, 2, "logits"}, {p->ids_out, 4, "ids_out"}, {p->weights_out, 4, "weights_out"}}))) return rc;
    if ((rc = check_strides8({{p->x_row_stride, "x_row_stride"}, {p->y_row_stride, "y_row_stride"}}))) return rc;
    if (p->x_row_stride < p->H || p->y_row_stride < p->H)
        return fail(HYD_ERR_BAD_ARG, "x_row_stride %lld or y_row_stride %lld < H %d", (long long)p->x_row_stride, (long long)p->y_row_stride, p->H);
    MoeLayout l = moe_layout(p->T, p->E, p->k, p->H, p->I);
    const MoeGroupedLayout gl = moe_grouped_layout(p->T, p->E, p->k, p->H, p->I);
    if (grouped)  // (no offsets slice: the tile table stands in its place, and a.offsets is not handed out)
        l = MoeLayout{gl.ids, gl.weights, gl.counts, gl.tiles, gl.slots, gl.act, gl.yslot, gl.bytes};
    if (!p->workspace || p->workspace_bytes < l.bytes)
        return fail(HYD_ERR_WORKSPACE, "%s needs %zu workspace bytes for T %d E %d k %d H %d I %d, got %zu", grouped ? grouped_name : "moe_mlp", l.bytes,
                    p->T, p->E, p->k, p->H, p->I, p->workspace ? p->workspace_bytes : (size_t)0);
    if (misaligned(p->workspace, 16)) return fail(HYD_ERR_WORKSPACE, "workspace must be 16-byte aligned");
    char* ws = static_cast<char*>(p->workspace);
    memset(&a, 0, sizeof(a));
    a.x = p->x; a.logits = p->logits; a.gate_up = p->gate_up; a.down = p->down; a.y = p->y;
    a.ids = reinterpret_cast<int32_t*>(ws + l.ids); a.weights = reinterpret_cast<float*>(ws + l.weights);
    a.counts = reinterpret_cast<int32_t*>(ws + l.counts); a.offsets = reinterpret_cast<int32_t*>(ws + l.offsets);
    a.slots = reinterpret_cast<int32_t*>(ws + l.slots); a.act = ws + l.act; a.yslot = reinterpret_cast<float*>(ws + l.yslot);
    a.ids_out = p->ids_out; a.weights_out = p->weights_out;
    a.xs = p->x_row_stride; a.ys = p->y_row_stride;
    a.T = p->T; a.E = p->E; a.k = p->k; a.H = p->H; a.I = p->I; a.renorm = p->renormalize;
    if (grouped) {
        a.offsets = nullptr;
        grouped->tiles = reinterpret_cast<int32_t*>(ws + gl.tiles);
    }
    return HYD_OK;
}

// the two scale pointers of the quantized forms (P: hyd_moe_w8_params or hyd_moe_w4_params)
template <typename P>
int moe_scales(const P* p, MoeW8Args& a) {
    if (int rc = check_not_null({{p->gate_up_scale, "gate_up_scale"}, {p->down_scale, "down_scale"}})) return rc;
    if (int rc = check_elem_align({{p->gate_up_scale, 4, "gate_up_scale"}, {p->down_scale, 4, "down_scale"}})) return rc;
    a.gate_up_scale = p->gate_up_scale;
    a.down_scale = p->down_scale;
    return HYD_OK;
}

}  // namespace

extern "C" {

size_t hyd_moe_workspace_bytes(int32_t T, int32_t E, int32_t k, int32_t H, int32_t I, int32_t dtype) {
    if (check_moe_shapes(T, E, k, H, I, dtype, false)) return 0;
    return moe_layout(T, E, k, H, I).bytes;
}

int hyd_moe_mlp(const hyd_moe_params* p, void* stream) {
    MoeArgs a;
    const int rc = moe_args(p, a);
    if (rc) return rc;
    return launched(launch_moe_mlp(a, p->dtype, static_cast<hipStream_t>(stream)), "moe_mlp kernel launches");
}

size_t hyd_moe_grouped_workspace_bytes(int32_t T, int32_t E, int32_t k, int32_t H, int32_t I, int32_t dtype) {
    if (check_moe_shapes(T, E, k, H, I, dtype, false, kMoeGroupedMaxRows)) return 0;
    return moe_grouped_layout(T, E, k, H, I).bytes;
}

int hyd_moe_mlp_grouped(const hyd_moe_params* p, void* stream) {
    MoeGroupedArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = moe_args(p, a.c, &a);
    if (rc) return rc;
    return launched(launch_moe_mlp_grouped(a, p->dtype, static_cast<hipStream_t>(stream)), "moe_mlp_grouped kernel launches");
}

int hyd_moe_mlp_grouped_w8(const hyd_moe_w8_params* p, void* stream) {
    MoeGroupedW8Args a;
    memset(&a, 0, sizeof(a));
    MoeW8Args scales;
    int rc = moe_args(p, a.g.c, &a.g, "moe_mlp_grouped_w8");
    if (rc || (rc = moe_scales(p, scales))) return rc;
    a.gate_up_scale = scales.gate_up_scale;
    a.down_scale = scales.down_scale;
    return launched(launch_moe_mlp_grouped_w8(a, p->dtype, static_cast<hipStream_t>(stream)), "moe_mlp_grouped_w8 kernel launches");
}

int hyd_moe_mlp_w8(const hyd_moe_w8_params* p, void* stream) {
    MoeW8Args a;
    int rc = moe_args(p, a.c);
    if (rc || (rc = moe_scales(p, a))) return rc;
    return launched(launch_moe_mlp_w8(a, p->dtype, static_cast<hipStream_t>(stream)), "moe_mlp_w8 kernel launches");
}

int hyd_moe_mlp_w4(const hyd_moe_w4_params* p, void* stream) {
    MoeW4Args a;
    int rc = moe_args(p, a.c.c);
    if (rc || (rc = moe_scales(p, a.c))) return rc;
    if ((rc = check_not_null({{p->gate_up_shift, "gate_up_shift"}, {p->down_shift, "down_shift"}}))) return rc;
    // a K that is whole steps (K % 256 == 0) reads a half step's four shift bytes of a row as one aligned load: rows are K / 32 = 8 n bytes
    if ((p->H % 256 == 0 && misaligned(p->gate_up_shift, 8)) || (p->I % 256 == 0 && misaligned(p->down_shift, 8)))
        return fail(HYD_ERR_BAD_ARG, "gate_up_shift (H %d) / down_shift (I %d) must be 8-byte aligned where the depth is a multiple of 256", p->H, p->I);
    a.gate_up_shift = p->gate_up_shift;
    a.down_shift = p->down_shift;
    return launched(launch_moe_mlp_w4(a, p->dtype, static_cast<hipStream_t>(stream)), "moe_mlp_w4 kernel launches");
}

}  // extern "C"
