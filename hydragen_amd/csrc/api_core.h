// What the translation units of the C ABI layer (api_*.hip) share: the error string and the argument checkers.  Host code only,
// internal to the library (built with hidden visibility; include/hydragen_hip.h is the whole public surface).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "hyd_kernels.h"

namespace hyd {

int fail(int code, const char* fmt, ...);  // sets the calling thread's hyd_last_error_string() and returns `code` (api_core.hip)
// what a launcher returned -> HYD_OK, or HYD_ERR_LAUNCH with "<what> failed: hip error <rc>"
inline int launched(int rc, const char* what) { return rc ? fail(HYD_ERR_LAUNCH, "%s failed: hip error %d", what, rc) : HYD_OK; }

inline bool misaligned(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(to - 1)) != 0; }  // (null is aligned)

inline int check_ptr_align(const void* p, const char* name) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "%s is null", name);
    if (misaligned(p, 16)) return fail(HYD_ERR_BAD_ARG, "%s must be 16-byte aligned", name);
    return HYD_OK;
}
inline int check_stride8(int64_t s, const char* name) {
    return s % 8 != 0 ? fail(HYD_ERR_BAD_ARG, "%s (%lld) must be a multiple of 8 elements", name, (long long)s) : HYD_OK;
}

// ---- lists of fields checked alike: the first failing item in listed order answers ------------------------------------------------------
struct NamedPtr { const void* p; const char* name; };
struct SizedPtr { const void* p; size_t size; const char* name; };
struct NamedStride { int64_t s; const char* name; };

inline int check_ptrs_align(std::initializer_list<NamedPtr> ptrs) {  // check_ptr_align of each
    for (const NamedPtr& x : ptrs)
        if (int rc = check_ptr_align(x.p, x.name)) return rc;
    return HYD_OK;
}
inline int check_strides8(std::initializer_list<NamedStride> strides) {  // check_stride8 of each
    for (const NamedStride& x : strides)
        if (int rc = check_stride8(x.s, x.name)) return rc;
    return HYD_OK;
}
// "<prefix>a / b / c <what>" from the names of a list
template <typename T>
int fail_joined(std::initializer_list<T> items, const char* prefix, const char* what) {
    char names[256] = "";
    for (const T& x : items) {
        if (names[0]) strncat(names, " / ", sizeof(names) - strlen(names) - 1);
        strncat(names, x.name, sizeof(names) - strlen(names) - 1);
    }
    return fail(HYD_ERR_BAD_ARG, "%s%s %s", prefix, names, what);
}
inline int check_not_null(std::initializer_list<NamedPtr> ptrs, const char* prefix = "") {  // any null: "a / b / c is null"
    for (const NamedPtr& x : ptrs)
        if (!x.p) return fail_joined(ptrs, prefix, "is null");
    return HYD_OK;
}
inline int check_elem_align(std::initializer_list<SizedPtr> ptrs, const char* prefix = "") {  // any off its element size (null is aligned)
    for (const SizedPtr& x : ptrs)
        if (misaligned(x.p, x.size)) return fail_joined(ptrs, prefix, "is not aligned to its element size");
    return HYD_OK;
}

// ---- shapes ---------------------------------------------------------------------------------------------------------------------------
inline int check_scale(float s) {
    if (!(s >= 0.f) || s > 1.0e4f) return fail(HYD_ERR_BAD_ARG, "softmax_scale %g (0 = head_dim^-0.5, or a positive finite scale)", (double)s);
    return HYD_OK;
}
inline int check_common(int dtype, int B, int nq, int Hq, int Hkv, int D) {
    if (dtype != HYD_F16 && dtype != HYD_BF16) return fail(HYD_ERR_UNSUPPORTED, "dtype %d: only f16/bf16", dtype);
    if (D != 64 && D != 128 && D != 256) return fail(HYD_ERR_UNSUPPORTED, "head_dim %d: only 64, 128 and 256 are implemented", D);
    if (B <= 0 || nq <= 0 || Hq <= 0 || Hkv <= 0) return fail(HYD_ERR_BAD_ARG, "non-positive size B=%d nq=%d Hq=%d Hkv=%d", B, nq, Hq, Hkv);
    if (Hq % Hkv != 0) return fail(HYD_ERR_BAD_ARG, "qheads %d not divisible by kvheads %d", Hq, Hkv);
    return HYD_OK;
}
// Narrow rows (hyd_suffix_params.kv_dim, hyd_rope_params.head_dim): 0 or D = rows of D elements; else 16 <= n < D, n % 16 == 0.
inline int check_narrow_dim(int n, int D, const char* field) {
    if (n == 0 || n == D) return HYD_OK;
    if (n < 16 || n > D || n % 16 != 0)
        return fail(HYD_ERR_BAD_ARG, "%s %d: 0 or %d (rows of D elements), or a multiple of 16 in [16, %d)", field, n, D, D);
    return HYD_OK;
}
inline int fail_narrow_fp8() { return fail(HYD_ERR_UNSUPPORTED, "kv_dim / head_dim with fp8 caches: narrow rows are implemented for 16-bit caches only"); }

// What a hyd_kv_quant asks of a call whose q dtype is `dtype`: nothing (absent, or the q dtype), e4m3fn caches, or a dtype nobody has.
enum KvqKind { kKvqNone, kKvqFp8, kKvqUnsupported };
inline KvqKind kvq_kind(const hyd_kv_quant* kq, int dtype) {
    if (!kq || kq->kv_dtype == dtype) return kKvqNone;
    return kq->kv_dtype == HYD_FP8_E4M3 ? kKvqFp8 : kKvqUnsupported;
}
// Validates *kq and narrows it to what the launch paths take: null, or fp8 unique caches.
inline int check_kvq(const hyd_kv_quant** kq, int dtype) {
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

// A token automaton's tables over n tokens (hyd_token_dfa, hyd_dfa_forced_params, hyd_draft_constrain_params): a state's bitmap row
// holds ceil(n / 32) words, its transition row n entries.
inline int check_allowed_stride(int64_t stride, int n, const char* prefix = "") {
    const int words = (n + 31) / 32;
    return stride < words ? fail(HYD_ERR_BAD_ARG, "%sallowed_stride %lld < ceil(n / 32) = %d words", prefix, (long long)stride, words) : HYD_OK;
}
inline int check_next_stride(int64_t stride, int n, const char* prefix = "") {
    return stride < n ? fail(HYD_ERR_BAD_ARG, "%snext_stride %lld < n %d", prefix, (long long)stride, n) : HYD_OK;
}

}  // namespace hyd
