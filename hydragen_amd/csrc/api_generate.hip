// C ABI, the decode loop's device-side bookkeeping: stop conditions, and speculative decoding's draft lookup, automaton-forced
// drafts and draft acceptance.  The draft kernels take the validated public parameter blocks as they are.
#include "api_core.h"

using namespace hyd;

namespace {

// One spelling of each rule that several of these calls state.  The row state hyd_stop_update and the draft-accept calls advance has
// the EOS ids and three cursors in common (shared_len is optional); the arrays around them are listed by each call, in its own order.
int check_n_eos(int n) { return n < 0 || n > HYD_STOP_MAX_EOS ? fail(HYD_ERR_BAD_ARG, "n_eos %d: 0 to %d EOS ids", n, HYD_STOP_MAX_EOS) : HYD_OK; }
template <typename P>
int check_row_cursors(const P* p) { return check_not_null({{p->start_pos, "start_pos"}, {p->feed, "feed"}, {p->next_pos, "next_pos"}}); }
int check_draft_k(int K) { return K < 1 || K > 7 ? fail(HYD_ERR_BAD_ARG, "K = %d drafts per row, 1 to 7 are taken", K) : HYD_OK; }
int check_dfa_size(int n_states, int n) { return n_states <= 0 || n <= 0 ? fail(HYD_ERR_BAD_ARG, "n_states %d, n %d must be > 0", n_states, n) : HYD_OK; }

int check_draft_accept(const hyd_draft_accept_params* p) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->rows < 0) return fail(HYD_ERR_BAD_ARG, "rows %d", p->rows);
    if (p->T < 1 || p->T > 8) return fail(HYD_ERR_BAD_ARG, "T = %d tokens per row (K = %d drafts): 1 to 8 tokens are taken", p->T, p->T - 1);
    if (int rc = check_n_eos(p->n_eos)) return rc;
    if (p->max_new_tokens < 1 || p->max_new_tokens > p->out_stride)
        return fail(HYD_ERR_BAD_ARG, "max_new_tokens %d outside [1, out_stride = %lld]", p->max_new_tokens, (long long)p->out_stride);
    int rc = check_not_null({{p->fed, "fed"}, {p->sampled, "sampled"}, {p->out, "out"}, {p->length, "length"}, {p->reason, "reason"},
                             {p->stop_index, "stop_index"}, {p->accepted, "accepted"}, {p->live, "live"}});
    if (!rc) rc = check_row_cursors(p);
    if (!rc) rc = check_elem_align({{p->fed, 8, "fed"}, {p->sampled, 8, "sampled"}, {p->out, 8, "out"}, {p->start_pos, 8, "start_pos"},
                                    {p->shared_len, 8, "shared_len"}, {p->feed, 8, "feed"}, {p->next_pos, 8, "next_pos"}});
    if (!rc) rc = check_elem_align({{p->length, 4, "length"}, {p->reason, 4, "reason"}, {p->stop_index, 4, "stop_index"}, {p->accepted, 4, "accepted"},
                                    {p->live, 4, "live"}, {p->logprobs, 4, "logprobs"}, {p->out_logprobs, 4, "out_logprobs"}});
    return rc;
}

// hyd_stop_update, and with a row limit array hyd_stop_update_rows
int stop_update(const hyd_stop_params* p, const int32_t* max_len, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->rows < 0) return fail(HYD_ERR_BAD_ARG, "rows %d", p->rows);
    if (int rc = check_n_eos(p->n_eos)) return rc;
    if (p->n_stop < 0 || p->n_stop > HYD_STOP_MAX_SEQS) return fail(HYD_ERR_BAD_ARG, "n_stop %d: 0 to %d stop sequences", p->n_stop, HYD_STOP_MAX_SEQS);
    for (int k = 0; k < p->n_stop; ++k)
        if (p->stop_lens[k] < 1 || p->stop_lens[k] > HYD_STOP_MAX_LEN)
            return fail(HYD_ERR_BAD_ARG, "stop_lens[%d] = %d: a stop sequence holds 1 to %d tokens", k, p->stop_lens[k], HYD_STOP_MAX_LEN);
    if (p->t < 0 || p->t >= p->out_stride) return fail(HYD_ERR_BAD_ARG, "t %d outside [0, out_stride = %lld)", p->t, (long long)p->out_stride);
    int rc = check_not_null({{p->tok, "tok"}, {p->out, "out"}, {p->length, "length"}, {p->reason, "reason"}, {p->stop_index, "stop_index"}, {p->live, "live"}});
    if (!rc) rc = check_row_cursors(p);
    if (rc) return rc;
    if (p->n_stop > 0 && !p->stop_tokens) return fail(HYD_ERR_BAD_ARG, "n_stop %d needs stop_tokens (null)", p->n_stop);
    rc = check_elem_align({{p->tok, 8, "tok"}, {p->out, 8, "out"}, {p->stop_tokens, 8, "stop_tokens"}, {p->start_pos, 8, "start_pos"},
                           {p->shared_len, 8, "shared_len"}, {p->feed, 8, "feed"}, {p->next_pos, 8, "next_pos"}});
    if (!rc) rc = check_elem_align({{p->length, 4, "length"}, {p->reason, 4, "reason"}, {p->stop_index, 4, "stop_index"}, {p->live, 4, "live"}});
    if (!rc) rc = check_elem_align({{max_len, 4, "max_len"}});
    if (rc) return rc;
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
    a.max_len = max_len;
    return launched(launch_stop_update(a, static_cast<hipStream_t>(stream)), "stop_update kernel launch");
}

}  // namespace

extern "C" {

int hyd_stop_update(const hyd_stop_params* p, void* stream) { return stop_update(p, nullptr, stream); }

int hyd_stop_update_rows(const hyd_stop_params* p, const int32_t* max_len, void* stream) { return stop_update(p, max_len, stream); }

int hyd_draft_lookup(const hyd_draft_lookup_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->B < 0) return fail(HYD_ERR_BAD_ARG, "B %d", p->B);
    if (int rc = check_draft_k(p->K)) return rc;
    if (p->ngram_min < 1 || p->ngram_max < p->ngram_min || p->ngram_max > HYD_DRAFT_MAX_NGRAM)
        return fail(HYD_ERR_BAD_ARG, "ngram (%d, %d): 1 <= min <= max <= %d", p->ngram_min, p->ngram_max, HYD_DRAFT_MAX_NGRAM);
    if (p->n_segments < 1 || p->n_segments > HYD_DRAFT_MAX_SEGMENTS)
        return fail(HYD_ERR_BAD_ARG, "n_segments %d: 1 to %d segments", p->n_segments, HYD_DRAFT_MAX_SEGMENTS);
    if (int rc = check_not_null({{p->drafts, "drafts"}, {p->n_proposed, "n_proposed"}})) return rc;
    if (int rc = check_elem_align({{p->drafts, 8, "drafts"}, {p->n_proposed, 4, "n_proposed"}})) return rc;
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
    int rc = check_dfa_size(p->n_states, p->n);
    if (!rc) rc = check_allowed_stride(p->allowed_stride, p->n);
    if (!rc) rc = check_not_null({{p->allowed, "allowed"}, {p->forced, "forced"}});
    if (!rc) rc = check_elem_align({{p->allowed, 4, "allowed"}, {p->forced, 4, "forced"}});
    return rc ? rc : launched(launch_dfa_forced(*p, static_cast<hipStream_t>(stream)), "dfa_forced kernel launch");
}

int hyd_draft_constrain(const hyd_draft_constrain_params* p, void* stream) {
    if (!p) return fail(HYD_ERR_BAD_ARG, "null params");
    if (p->B < 0) return fail(HYD_ERR_BAD_ARG, "B %d", p->B);
    int rc = check_draft_k(p->K);
    if (!rc) rc = check_dfa_size(p->n_states, p->n);
    if (!rc) rc = check_next_stride(p->next_stride, p->n);
    if (rc) return rc;
    if (p->fed_stride < p->K + 1) return fail(HYD_ERR_BAD_ARG, "fed_stride %lld < K + 1 = %d", (long long)p->fed_stride, p->K + 1);
    rc = check_not_null({{p->state, "state"}, {p->fed, "fed"}, {p->forced, "forced"}, {p->next, "next"}, {p->step_state, "step_state"}, {p->n_forced, "n_forced"}});
    if (!rc) rc = check_elem_align({{p->state, 4, "state"}, {p->fed, 8, "fed"}, {p->n_proposed, 4, "n_proposed"}, {p->forced, 4, "forced"}, {p->next, 4, "next"},
                                    {p->step_state, 4, "step_state"}, {p->n_forced, 4, "n_forced"}});
    return rc ? rc : launched(launch_draft_constrain(*p, static_cast<hipStream_t>(stream)), "draft_constrain kernel launch");
}

int hyd_draft_accept(const hyd_draft_accept_params* p, void* stream) {
    const int rc = check_draft_accept(p);
    return rc ? rc : launched(launch_draft_accept(*p, static_cast<hipStream_t>(stream)), "draft_accept kernel launch");
}

int hyd_draft_accept_states(const hyd_draft_accept_params* p, const int32_t* step_state_after, int32_t* state, void* stream) {
    if (!step_state_after && !state) return hyd_draft_accept(p, stream);
    int rc = check_draft_accept(p);
    if (rc) return rc;
    if (!step_state_after || !state) return fail(HYD_ERR_BAD_ARG, "step_state_after and state go together: one of them is null");
    if ((rc = check_elem_align({{step_state_after, 4, "step_state_after"}, {state, 4, "state"}}))) return rc;
    return launched(launch_draft_accept_states(*p, step_state_after, state, static_cast<hipStream_t>(stream)), "draft_accept kernel launch");
}

int hyd_draft_accept_stop(const hyd_draft_accept_params* p, const hyd_stop_params* stop, const int32_t* step_state_after, int32_t* state,
                          int32_t* gen, int32_t* gen_len, int32_t gen_stride, void* stream) {
    int rc = check_draft_accept(p);
    if (rc) return rc;
    if ((step_state_after == nullptr) != (state == nullptr)) return fail(HYD_ERR_BAD_ARG, "step_state_after and state go together: one of them is null");
    if ((rc = check_elem_align({{step_state_after, 4, "step_state_after"}, {state, 4, "state"}}))) return rc;
    const int n_stop = stop ? stop->n_stop : 0;
    if (n_stop < 0 || n_stop > HYD_STOP_MAX_SEQS) return fail(HYD_ERR_BAD_ARG, "n_stop %d: 0 to %d stop sequences", n_stop, HYD_STOP_MAX_SEQS);
    if (n_stop > 0 && !stop->stop_tokens) return fail(HYD_ERR_BAD_ARG, "n_stop %d needs stop_tokens (null)", n_stop);
    for (int k = 0; k < n_stop; ++k)
        if (stop->stop_lens[k] < 1 || stop->stop_lens[k] > HYD_STOP_MAX_LEN)
            return fail(HYD_ERR_BAD_ARG, "stop_lens[%d] = %d: a stop sequence holds 1 to %d tokens", k, stop->stop_lens[k], HYD_STOP_MAX_LEN);
    if ((gen == nullptr) != (gen_len == nullptr)) return fail(HYD_ERR_BAD_ARG, "gen and gen_len go together (one of them is null)");
    if (gen_stride < 0 || gen_stride > HYD_SAMPLE_GEN_MAX) return fail(HYD_ERR_BAD_ARG, "gen_stride %d outside [0, %d]", gen_stride, HYD_SAMPLE_GEN_MAX);
    if ((rc = check_elem_align({{n_stop > 0 ? stop->stop_tokens : nullptr, 8, "stop_tokens"}, {gen, 4, "gen"}, {gen_len, 4, "gen_len"}}))) return rc;
    if (n_stop == 0 && !gen)  // nothing of this call's own is asked for: it IS the existing call
        return launched(state ? launch_draft_accept_states(*p, step_state_after, state, static_cast<hipStream_t>(stream))
                              : launch_draft_accept(*p, static_cast<hipStream_t>(stream)), "draft_accept kernel launch");
    DraftStopArgs s;
    memset(&s, 0, sizeof(s));
    s.stop_tokens = n_stop > 0 ? stop->stop_tokens : nullptr;
    s.gen = gen; s.gen_len = gen_len; s.gen_stride = gen_stride;
    for (int k = 0; k < n_stop; ++k) s.stop_lens[k] = stop->stop_lens[k];
    s.n_stop = n_stop; s.include_stop = (stop && stop->include_stop) ? 1 : 0;
    return launched(launch_draft_accept_stop(*p, s, step_state_after, state, static_cast<hipStream_t>(stream)), "draft_accept_stop kernel launch");
}

}  // extern "C"
