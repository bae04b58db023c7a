// C ABI, the [rows, n] logits calls: the samplers (plain, filtered, penalised, under a token automaton, with per-row values), the token bitmaps
// the penalties read, and the log-probs of given tokens.
#include "api_core.h"

using namespace hyd;

namespace {

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
    int rc = check_logits_rows(p->dtype, p->rows, p->n, HYD_SAMPLE_FILTER_MAX_N);
    if (!rc) rc = check_not_null({{p->logits, "logits"}, {p->out, "out"}});
    if (rc) return rc;
    if (!(p->temperature >= 0.f)) return fail(HYD_ERR_BAD_ARG, "temperature %g must be >= 0", (double)p->temperature);
    if (p->top_k < 0) return fail(HYD_ERR_BAD_ARG, "top_k %d must be >= 0 (0 = off)", p->top_k);
    if (!(p->top_p > 0.f && p->top_p <= 1.f)) return fail(HYD_ERR_BAD_ARG, "top_p %g must be in (0, 1] (1 = off)", (double)p->top_p);
    if (!(p->min_p >= 0.f && p->min_p <= 1.f)) return fail(HYD_ERR_BAD_ARG, "min_p %g must be in [0, 1] (0 = off)", (double)p->min_p);
    return check_row_stride(p->row_stride, p->n);
}
// ... and its last check, the alignment of the four row tensors, with the argument block of the filtered draw
template <typename P>
int fill_filter_args(const P* p, FilterArgs* a) {
    const size_t esz = logits_esz(p->dtype);
    if (int rc = check_elem_align({{p->logits, esz, "logits"}, {p->out, 8, "out"}, {p->logprobs, 4, "logprobs"}, {p->kept, 4, "kept"}})) return rc;
    memset(a, 0, sizeof(*a));
    a->logits = p->logits; a->out = p->out; a->logprobs = p->logprobs; a->kept = p->kept;
    a->row_stride = p->row_stride; a->seed = p->seed; a->offset = p->offset;
    a->rows = p->rows; a->n = p->n;
    a->inv_temperature = p->temperature > 0.f ? 1.0f / p->temperature : 0.f;  // (as hyd_sample_tokens: the same noise scale)
    a->top_k = p->top_k < p->n ? p->top_k : 0;
    a->top_p = p->top_p;
    a->log_min_p = p->min_p > 0.f ? (float)log((double)p->min_p) : -INFINITY;
    a->vec_ok = logits_vec_ok(p->logits, p->row_stride, 16 / (int)esz);
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
    if ((rc = check_elem_align({{p->gen, 4, "gen"}, {p->gen_len, 4, "gen_len"}, {p->bias_ids, 8, "bias_ids"}, {p->bias_values, 4, "bias_values"}}))) return rc;
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

// What hyd_sample_tokens_constrained checks of its automaton, and the kernels' argument block of it
int fill_constrain_args(const hyd_sample_penalty_params* p, const hyd_token_dfa* c, ConstrainArgs* ca) {
    int rc = check_not_null({{c->allowed, "allowed"}, {c->next, "next"}, {c->state, "state"}}, "hyd_token_dfa: ");
    if (rc) return rc;
    if (c->n_states <= 0) return fail(HYD_ERR_BAD_ARG, "hyd_token_dfa: n_states %d must be > 0", c->n_states);
    if ((rc = check_allowed_stride(c->allowed_stride, p->n, "hyd_token_dfa: "))) return rc;
    if ((rc = check_next_stride(c->next_stride, p->n, "hyd_token_dfa: "))) return rc;
    if ((rc = check_elem_align({{c->allowed, 4, "allowed"}, {c->next, 4, "next"}, {c->state, 4, "state"}}, "hyd_token_dfa: "))) return rc;
    memset(ca, 0, sizeof(*ca));
    ca->allowed = c->allowed; ca->next = c->next; ca->state = c->state;
    ca->allowed_stride = c->allowed_stride; ca->next_stride = c->next_stride;
    ca->n_states = c->n_states; ca->advance = c->advance ? 1 : 0;
    return HYD_OK;
}
// every penalty neutral (and nothing to append): x = l, so the row keeps the keys of its own width (sample_filter.hip's cost)
bool penalties_neutral(const hyd_sample_penalty_params* p) {
    return p->repetition_penalty == 1.0 && p->frequency_penalty == 0.0 && p->presence_penalty == 0.0 && p->n_bias == 0 && !p->append_out;
}

}  // namespace

extern "C" {

int hyd_sample_tokens(const hyd_sample_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_logits_rows(p->dtype, p->rows, p->n, /*max_n=*/0);  // (the plain sampler has no upper bound on n)
    if (!rc) rc = check_not_null({{p->logits, "logits"}, {p->out, "out"}});
    if (rc) return rc;
    if (!(p->temperature >= 0.f)) return fail(HYD_ERR_BAD_ARG, "temperature %g must be >= 0", (double)p->temperature);
    if ((rc = check_row_stride(p->row_stride, p->n))) return rc;
    if ((rc = check_elem_align({{p->logits, (size_t)logits_esz(p->dtype), "logits"}, {p->out, 8, "out"}}))) return rc;
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

int hyd_sample_tokens_penalized_drafts(const hyd_sample_penalty_params* p, const int64_t* fed, int32_t T, void* stream) {
    PenaltyArgs a;
    int rc = fill_penalty_args(p, &a);
    if (rc) return rc;
    if (T < 1 || T > 8) return fail(HYD_ERR_BAD_ARG, "T = %d tokens per sequence: 1 to 8 are taken", T);
    if (p->rows % T != 0) return fail(HYD_ERR_BAD_ARG, "rows %d is not a multiple of T = %d", p->rows, T);
    if (p->append_out) return fail(HYD_ERR_BAD_ARG, "append_out: the lists of a speculative step are kept by hyd_draft_accept_stop, not by the sampler");
    if (p->gen && !fed) return fail(HYD_ERR_BAD_ARG, "gen needs fed (null): the drafts in front of a position count as generated tokens");
    if ((rc = check_elem_align({{fed, 8, "fed"}}))) return rc;
    return launched(launch_sample_penalty_drafts(a, fed, T, p->dtype, static_cast<hipStream_t>(stream)), "sample_penalty_drafts kernel launch");
}

int hyd_sample_tokens_constrained(const hyd_sample_penalty_params* p, const hyd_token_dfa* c, void* stream) {
    if (!c) return hyd_sample_tokens_penalized(p, stream);
    PenaltyArgs a;
    ConstrainArgs ca;
    int rc = fill_penalty_args(p, &a);
    if (!rc) rc = fill_constrain_args(p, c, &ca);
    if (rc) return rc;
    return launched(launch_sample_constrain(a, ca, penalties_neutral(p), p->dtype, static_cast<hipStream_t>(stream)), "sample_constrain kernel launch");
}

int hyd_sample_tokens_rows(const hyd_sample_penalty_params* p, const hyd_token_dfa* c, const float* temperature, const int32_t* top_k,
                           const float* top_p, const float* min_p, const float* repetition_penalty, const float* frequency_penalty,
                           const float* presence_penalty, const uint64_t* seed, void* stream) {
    if (!temperature && !top_k && !top_p && !min_p && !repetition_penalty && !frequency_penalty && !presence_penalty && !seed)
        return hyd_sample_tokens_constrained(p, c, stream);
    PenaltyArgs a;
    ConstrainArgs ca;
    int rc = fill_penalty_args(p, &a);
    if (!rc && c) rc = fill_constrain_args(p, c, &ca);
    if (!rc) rc = check_elem_align({{temperature, 4, "temperature"}, {top_k, 4, "top_k"}, {top_p, 4, "top_p"}, {min_p, 4, "min_p"},
                                    {repetition_penalty, 4, "repetition_penalty"}, {frequency_penalty, 4, "frequency_penalty"},
                                    {presence_penalty, 4, "presence_penalty"}, {seed, 8, "seed"}}, "hyd_sample_tokens_rows: ");
    if (rc) return rc;
    const RowParams r{temperature, top_k, top_p, min_p, repetition_penalty, frequency_penalty, presence_penalty, seed};
    const bool neutral = penalties_neutral(p) && !repetition_penalty && !frequency_penalty && !presence_penalty;
    return launched(launch_sample_rows(a, c ? &ca : nullptr, r, neutral, p->dtype, static_cast<hipStream_t>(stream)), "sample_rows kernel launch");
}

int hyd_token_bitmap_build(const hyd_token_bitmap_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->groups < 0 || p->groups > 65535 || p->L < 0) return fail(HYD_ERR_BAD_ARG, "groups %d (0 to 65535), L %d", p->groups, p->L);
    if (p->n <= 0 || p->n > HYD_SAMPLE_FILTER_MAX_N) return fail(HYD_ERR_BAD_ARG, "n %d: 1 to %d", p->n, HYD_SAMPLE_FILTER_MAX_N);
    if (int rc = check_not_null({{p->ids, "ids"}, {p->bits, "bits"}})) return rc;
    if (p->id_stride < p->L) return fail(HYD_ERR_BAD_ARG, "id_stride %lld < L %d", (long long)p->id_stride, p->L);
    if (int rc = check_elem_align({{p->ids, 8, "ids"}, {p->lens, 8, "lens"}, {p->bits, 4, "bits"}})) return rc;
    BitmapArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = p->ids; a.lens = p->lens; a.bits = p->bits; a.id_stride = p->id_stride;
    a.groups = p->groups; a.L = p->L; a.n = p->n; a.words = (p->n + 31) / 32;
    return launched(launch_token_bitmap(a, static_cast<hipStream_t>(stream)), "token_bitmap kernel launch");
}

int hyd_token_logprobs(const hyd_token_logprob_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    int rc = check_logits_rows(p->dtype, p->rows, p->n, HYD_SAMPLE_FILTER_MAX_N);
    if (!rc) rc = check_not_null({{p->logits, "logits"}, {p->targets, "targets"}, {p->logprobs, "logprobs"}, {p->greedy, "greedy"}});
    if (rc) return rc;
    if (p->top_n < 0 || p->top_n > HYD_TOP_LOGPROBS_MAX) return fail(HYD_ERR_BAD_ARG, "top_n %d must be in [0, %d]", p->top_n, HYD_TOP_LOGPROBS_MAX);
    if (p->top_n > 0 && (!p->top_ids || !p->top_logprobs)) return fail(HYD_ERR_BAD_ARG, "top_n %d needs top_ids and top_logprobs (null)", p->top_n);
    if ((rc = check_row_stride(p->row_stride, p->n))) return rc;
    const size_t esz = logits_esz(p->dtype);
    rc = check_elem_align({{p->logits, esz, "logits"}, {p->targets, 8, "targets"}, {p->logprobs, 4, "logprobs"}, {p->top_ids, 8, "top_ids"}, {p->top_logprobs, 4, "top_logprobs"}});
    if (rc) return rc;
    TokenLogprobArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = p->logits; a.targets = p->targets; a.logprobs = p->logprobs; a.greedy = p->greedy;
    a.top_ids = p->top_ids; a.top_logprobs = p->top_logprobs;
    a.row_stride = p->row_stride; a.rows = p->rows; a.n = p->n; a.top_n = p->top_n;
    a.vec_ok = logits_vec_ok(p->logits, p->row_stride, 16 / (int)esz);
    return launched(launch_token_logprob(a, p->dtype, static_cast<hipStream_t>(stream)), "token_logprob kernel launch");
}

}  // extern "C"
