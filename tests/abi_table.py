"""A table of the C ABI's host-side contract: what the shapes-only queries answer and what the launch entry points refuse,
recorded once and compared exactly (tests/test_abi_table.py against tests/golden/abi_table.json).

    python tests/abi_table.py --write     record the table from the library that is built in the tree

The fixture is a recording of the library BEFORE a change to csrc/api_*.hip (the C ABI layer), not a product of the code under test: record it from
the parent commit, commit it as data, and let the changed library answer to it.

Four kinds of case.  A "query" never launches (plans, workspace sizes, support answers).  A "refusal" goes through a launch entry
point with made-up addresses and must come back with an error before anything is enqueued: its record is the return code and the
whole error string.  A "noop" goes through a launch entry point as well and must come back with HYD_OK before any HIP call (an empty
batch, an empty destination, a phase with nothing left to do): its record is the return code alone.  A "launch" is a call that is
ACCEPTED: where no device is present its first launch comes back as HYD_ERR_LAUNCH with "<what> failed: hip error N", and <what> names
the launcher the call reached -- its record is the return code and <what> (N belongs to the runtime, not to the project).  Launch cases
run only where no device is present: on one they would run kernels on made-up addresses.  --write records nothing when a
refusal is accepted (HYD_OK) or tries to launch (HYD_ERR_LAUNCH), when a noop does not answer HYD_OK, or when a launch case does not
answer HYD_ERR_LAUNCH.
"""
import ctypes as C
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

from hydragen_amd import _lib  # noqa: E402

FIXTURE = REPO / "tests" / "golden" / "abi_table.json"
HYD_OK, HYD_ERR_LAUNCH = 0, -4
PTR = 0x10000  # an aligned address that is never dereferenced: every refusal comes before the first launch
ODD = PTR + 1  # misaligned for every element size
MIS8 = PTR + 8  # aligned to its element, not to 16 bytes
NAN, INF = float("nan"), float("inf")
MAX_N = _lib.SAMPLE_FILTER_MAX_N


def _fill(obj, kw):
    """setattr along dotted paths: "suffix.q", "levels.0.k", "stop_lens.3"."""
    for path, v in kw.items():
        *head, last = path.split(".")
        o = obj
        for name in head:
            o = o[int(name)] if name.isdigit() else getattr(o, name)
        if last.isdigit():
            o[int(last)] = v
        else:
            setattr(o, last, v)
    return obj


# ---- parameter blocks: each builder gives a call that WOULD launch with ptrs=True; a case breaks one or two fields of it ----------
def prefix(ptrs=False, **kw):
    p = _lib.PrefixParams()
    p.dtype, p.B, p.nq, p.Hq, p.Hkv, p.D, p.sb, p.kv_len = 1, 4, 1, 8, 8, 128, 1, 512
    if ptrs:
        p.q = p.k = p.v = p.out = p.workspace = PTR
        p.workspace_bytes = 1 << 40
    return _fill(p, kw)


def suffix(**kw):
    s = _lib.SuffixParams()
    s.dtype, s.B, s.nq, s.Hq, s.Hkv, s.D, s.kv_len = 1, 4, 1, 8, 8, 128, 16
    s.q = s.k = s.v = s.out = PTR
    _fill(s, {k: kw.pop(k) for k in list(kw) if k in ("B", "nq", "Hq", "Hkv", "D", "kv_len")})
    s.k_head_stride = s.v_head_stride = s.D
    s.k_tok_stride = s.v_tok_stride = s.Hkv * s.D
    s.k_batch_stride = s.v_batch_stride = max(s.kv_len, 1) * s.Hkv * s.D
    return _fill(s, kw)


def decode(levels=((1, 64),), ptrs=False, **kw):
    """levels: (sb, kv_len) or (sb, kv_len, token stride); the token stride defaults to the unique tensors' Hkv * D."""
    d = _lib.DecodeParams()
    shape = {k: kw.pop(k) for k in list(kw) if k in ("B", "nq", "Hq", "Hkv", "D", "kv_len")}
    d.suffix = suffix(**shape)
    if not ptrs:
        d.suffix.q = d.suffix.k = d.suffix.v = d.suffix.out = None
    s = d.suffix
    d.n_levels = len(levels)
    for i, lv in enumerate(levels):
        sb, n = lv[:2]
        L = d.levels[i]
        L.sb, L.kv_len = sb, n
        L.k_head_stride = L.v_head_stride = s.D
        L.k_tok_stride = L.v_tok_stride = lv[2] if len(lv) > 2 else s.Hkv * s.D
        L.k_group_stride = L.v_group_stride = n * L.k_tok_stride
        if ptrs:
            L.k = L.v = PTR
    if ptrs:
        d.workspace, d.workspace_bytes = PTR, 1 << 40
    return _fill(d, kw)


def kvq(kv_dtype=_lib.HYD_FP8_E4M3, flags=0, **kw):
    q = _lib.KvQuant()
    q.kv_dtype, q.flags = kv_dtype, flags
    return _fill(q, kw)


def rope(**kw):
    p = _lib.RopeParams()
    p.dtype, p.B, p.Hq, p.Hkv, p.D, p.cache_len, p.max_pos = 1, 4, 8, 8, 128, 64, 128
    p.q = p.k = p.v = p.q_out = p.k_cache = p.v_cache = p.cos = p.sin = p.position_ids = p.seq_lens = PTR
    p.q_batch_stride = p.k_batch_stride = p.v_batch_stride = 1024
    p.kc_head_stride = p.vc_head_stride = 128
    p.kc_tok_stride = p.vc_tok_stride = 1024
    p.kc_batch_stride = p.vc_batch_stride = 64 * 1024
    p.pos_stride, p.cs_stride = 1, 128
    return _fill(p, kw)


def rmsnorm(**kw):
    p = _lib.AddRmsnormParams()
    p.x = p.weight = p.norm_out = PTR
    p.x_row_stride = p.residual_row_stride = p.sum_row_stride = p.norm_row_stride = 64
    p.rows, p.n, p.dtype, p.eps = 4, 64, 1, 1e-5
    return _fill(p, kw)


def swiglu(**kw):
    p = _lib.SwigluParams()
    p.gate = p.up = p.out = PTR
    p.gate_row_stride = p.up_row_stride = p.out_row_stride = 64
    p.rows, p.n, p.dtype = 4, 64, 1
    return _fill(p, kw)


def _logits_row(p, kw):
    p.logits = p.out = PTR
    p.row_stride, p.rows, p.n, p.dtype, p.temperature = 64, 4, 64, 1, 1.0
    return _fill(p, kw)


def sample(**kw):
    return _logits_row(_lib.SampleParams(), kw)


def sample_filter(**kw):
    p = _lib.SampleFilterParams()
    p.top_p = 1.0
    return _logits_row(p, kw)


def sample_penalty(**kw):
    p = _lib.SamplePenaltyParams()
    p.top_p, p.repetition_penalty = 1.0, 1.0
    return _logits_row(p, kw)


def bitmap(**kw):
    p = _lib.TokenBitmapParams()
    p.ids = p.bits = PTR
    p.id_stride, p.groups, p.L, p.n = 8, 2, 8, 64
    return _fill(p, kw)


def token_logprob(**kw):
    p = _lib.TokenLogprobParams()
    p.logits = p.targets = p.logprobs = p.greedy = PTR
    p.dtype, p.n, p.rows, p.row_stride = 1, 64, 4, 64
    return _fill(p, kw)


def stop(**kw):
    p = _lib.StopParams()
    p.tok = p.out = p.length = p.reason = p.stop_index = p.live = p.start_pos = p.feed = p.next_pos = PTR
    p.out_stride, p.rows, p.t = 8, 4, 0
    return _fill(p, kw)


def rope_multi(**kw):
    p = _lib.RopeMultiParams()
    p.dtype, p.B, p.T, p.Hq, p.Hkv, p.D, p.cache_len, p.max_pos = 1, 4, 2, 8, 8, 128, 64, 128
    p.q = p.k = p.v = p.q_out = p.k_cache = p.v_cache = p.cos = p.sin = p.position_ids = p.seq_lens = PTR
    p.q_tok_stride = p.k_tok_stride = p.v_tok_stride = 1024
    p.q_batch_stride = p.k_batch_stride = p.v_batch_stride = 2048
    p.kc_head_stride = p.vc_head_stride = 128
    p.kc_tok_stride = p.vc_tok_stride = 1024
    p.kc_batch_stride = p.vc_batch_stride = 64 * 1024
    p.pos_stride, p.cs_stride = 2, 128
    return _fill(p, kw)


def token_dfa(**kw):
    c = _lib.TokenDfa()
    c.allowed = c.next = c.state = PTR
    c.allowed_stride, c.next_stride, c.n_states = 2, 64, 4   # (sample_penalty's n = 64: two bitmap words per state)
    return _fill(c, kw)


def draft_lookup(**kw):
    p = _lib.DraftLookupParams()
    p.drafts = p.n_proposed = PTR
    p.drafts_stride, p.n_segments, p.B, p.K, p.ngram_min, p.ngram_max = 3, 2, 4, 3, 1, 3
    for g in p.segments:   # (all of them, so that a case may raise n_segments)
        g.ids, g.row_stride, g.len, g.div = PTR, 16, 16, 1
    return _fill(p, kw)


def dfa_forced(**kw):
    p = _lib.DfaForcedParams()
    p.allowed = p.forced = PTR
    p.allowed_stride, p.n_states, p.n = 2, 4, 64
    return _fill(p, kw)


def draft_constrain(**kw):
    p = _lib.DraftConstrainParams()
    p.state = p.fed = p.forced = p.next = p.step_state = p.n_forced = PTR
    p.fed_stride, p.next_stride, p.B, p.K, p.n_states, p.n = 4, 64, 4, 3, 4, 64
    return _fill(p, kw)


def draft_accept(**kw):
    p = _lib.DraftAcceptParams()
    p.fed = p.sampled = p.out = p.length = p.reason = p.stop_index = p.accepted = p.live = p.start_pos = p.feed = p.next_pos = PTR
    p.out_stride, p.rows, p.T, p.max_new_tokens = 8, 4, 4, 8
    return _fill(p, kw)


def _kv_unique(p, kw):
    """The unique segment of hyd_kv_promote / hyd_kv_gather_paths: the fields the two blocks share by name."""
    p.k_src = p.v_src = p.k_dst = p.v_dst = p.rows = p.lens = PTR
    p.k_head_stride = p.v_head_stride = 128
    p.k_tok_stride = p.v_tok_stride = 1024
    p.k_batch_stride = p.v_batch_stride = 64 * 1024
    p.src_dtype, p.dst_dtype, p.n, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst, p.capacity = 1, 1, 4, 4, 64, 8, 128, 128, 256
    return _fill(p, kw)


def kv_promote(**kw):
    p = _lib.KvPromoteParams()
    p.cu = PTR
    return _kv_unique(p, kw)


def kv_gather(**kw):
    p = _lib.KvGatherParams()
    p.cu_dst, p.n_levels = PTR, 2
    for j in range(_lib.HYD_MAX_LEVELS):   # (all of them, so that a case may raise n_levels)
        p.level_k[j] = p.level_v[j] = p.level_cu[j] = PTR
        p.level_s[j], p.level_cap[j], p.level_div[j] = 1, 64, 4
    return _kv_unique(p, kw)


def kv_absmax(**kw):
    p = _lib.KvAbsmaxParams()
    p.k = p.v = p.amax = PTR
    p.k_head_stride = p.v_head_stride = 128
    p.k_row_stride = p.v_row_stride = 1024
    p.k_outer_stride = p.v_outer_stride = 64 * 1024
    p.dtype, p.Hkv, p.d, p.n_outer, p.n_rows = 1, 8, 128, 4, 64
    return _fill(p, kw)


def kv_scales(**kw):
    p = _lib.KvScalesParams()
    p.amax = p.k_scale = p.v_scale = PTR
    p.Hkv, p.c = 8, 1.0 / 448.0
    return _fill(p, kw)


W8_SPLIT = dict(M=4, N=64, K=4096)   # a shape whose plan splits K: hyd_linear_w8_workspace_bytes(4, 64, 4096) > 0


def linear_w8(**kw):
    p = _lib.LinearW8Params()
    p.x = p.w8 = p.scale = p.y = p.workspace = PTR
    p.workspace_bytes = 1 << 40
    p.M, p.N, p.K, p.dtype = 4, 64, 256, 1
    _fill(p, {k: kw.pop(k) for k in list(kw) if k in ("M", "N", "K")})
    p.x_row_stride, p.y_row_stride = p.K, p.N
    return _fill(p, kw)


def weight_widen(**kw):
    p = _lib.WeightWidenParams()
    p.w8 = p.scale = p.out = PTR
    p.out_row_stride, p.N, p.K, p.dtype = 256, 64, 256, 1
    return _fill(p, kw)


# ---- runners: one per kind of record ----------------------------------------------------------------------------------------
def _err(lib):
    return lib.hyd_last_error_string().decode()


def _q_prefix(lib, kw):
    p = prefix(**kw)
    ns, grid, sl = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = lib.hyd_prefix_plan(C.byref(p), C.byref(ns), C.byref(grid), C.byref(sl))
    rec = {"rc": rc, "num_splits": ns.value, "grid": grid.value, "split_len": sl.value,
           "workspace_bytes": lib.hyd_prefix_workspace_bytes(C.byref(p))}
    if rc:
        rec["error"] = _err(lib)
    return rec


def _q_decode(lib, kw):
    rec = {}
    for f32 in (0, 1):
        d = decode(f32_partials=f32, **kw)
        rec[f"workspace_bytes_f32_partials_{f32}"] = lib.hyd_decode_workspace_bytes(C.byref(d))
    d = decode(**kw)
    rec["two_stream_ok"] = lib.hyd_decode_two_stream_ok(C.byref(d))
    rec["kv_quant_supported"] = lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(kvq()))
    rec["kv_quant_supported_gqa"] = lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(kvq(flags=_lib.HYD_KVQ_GQA)))
    return rec


def _q_decode_kvq(lib, kw):
    """hyd_decode_kv_quant_supported under every combination of hyd_kv_quant.flags (the causal tail reads HYD_KVQ_CAUSAL)."""
    d = decode(**kw)
    return {f"supported_flags_{f}": lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(kvq(flags=f))) for f in (0, 1, 2, 3)}


def _q_workspace(lib, kw):
    sb = [lv[0] for lv in kw["levels"]]
    ln = [lv[1] for lv in kw["levels"]]
    n = kw.get("n_levels", len(sb))
    arr = lambda xs: (C.c_int32 * max(len(xs), 1))(*xs)  # noqa: E731
    return {"bytes": lib.hyd_workspace_bytes(kw["B"], kw.get("nq", 1), kw["Hq"], kw["Hkv"], kw["D"], n, arr(sb), arr(ln))}


def _q_kvq(lib, kw):
    kw = dict(kw)
    kv_dtype = kw.pop("kv_dtype", _lib.HYD_FP8_E4M3)
    s = suffix(**kw)
    return {"supported": lib.hyd_kv_quant_supported(C.byref(s), C.byref(kvq(kv_dtype))),
            "supported_gqa": lib.hyd_kv_quant_supported(C.byref(s), C.byref(kvq(kv_dtype, _lib.HYD_KVQ_GQA))),
            "supported_null_kq": lib.hyd_kv_quant_supported(C.byref(s), None)}


def _q_null(lib, kw):
    return {"prefix_workspace_bytes": lib.hyd_prefix_workspace_bytes(None), "decode_workspace_bytes": lib.hyd_decode_workspace_bytes(None),
            "two_stream_ok": lib.hyd_decode_two_stream_ok(None), "kv_quant_supported": lib.hyd_kv_quant_supported(None, None),
            "decode_kv_quant_supported": lib.hyd_decode_kv_quant_supported(None, None)}


def _q_block(lib, kw):
    return {"bytes": lib.hyd_allreduce_block_bytes(kw["world"], kw["max_bytes"])}


def _q_narrow(lib, kw):
    """hyd_narrow_kv_supported as hydragen_amd/flash.py asks it: contiguous [B, kv_len, Hkv, kv_dim] caches."""
    kw = dict(kw)
    if kw.pop("null", False):
        return {"supported": lib.hyd_narrow_kv_supported(None)}
    s = suffix(**kw)
    d = s.kv_dim or s.D
    s.k_head_stride = s.v_head_stride = d
    s.k_tok_stride = s.v_tok_stride = s.Hkv * d
    s.k_batch_stride = s.v_batch_stride = max(s.kv_len, 1) * s.Hkv * d
    return {"supported": lib.hyd_narrow_kv_supported(C.byref(s))}


def _q_w8_workspace(lib, kw):
    return {"bytes": lib.hyd_linear_w8_workspace_bytes(kw["M"], kw["N"], kw["K"])}


def _refusal(lib, rc):
    return {"rc": rc, "error": _err(lib) if rc else ""}


def _params_runner(fn, build, with_kq=False):
    def run(lib, kw):
        kw = dict(kw)
        null = kw.pop("null", False)
        kq = kw.pop("kq", None)
        p = None if null else C.byref(build(**kw))
        f = getattr(lib, fn)
        if with_kq:
            return _refusal(lib, f(p, None if kq is None else C.byref(kvq(**kq)), None))
        return _refusal(lib, f(p, None))
    return run


def _r_combine(lib, kw):
    n = kw.get("n", 2)
    m = max(min(n, 65), 1)
    outs = (C.c_void_p * m)(*[PTR] * m)
    lses = (C.c_void_p * m)(*[PTR] * m)
    for i in kw.get("null_out", ()):
        outs[i] = None
    for i in kw.get("null_lse", ()):
        lses[i] = None
    rc = lib.hyd_combine_lse(None if kw.get("no_outs") else outs, None if kw.get("no_lses") else lses, n, kw.get("rows", 4),
                             kw.get("D", 64), kw.get("dtype", 1), kw.get("out", PTR), None, None)
    return _refusal(lib, rc)


def _r_allreduce(lib, kw):
    kw = dict(kw)
    if kw.pop("null", False):
        return _refusal(lib, lib.hyd_allreduce_sum(None, None))
    blocks = (C.c_void_p * 8)(*[PTR] * 8)
    for i, v in kw.pop("block", {}).items():
        blocks[i] = v
    p = _lib.AllReduceParams()
    p.blocks = None if kw.pop("no_blocks", False) else blocks
    p.in_ = p.out = PTR
    p.count, p.max_bytes, p.dtype, p.rank, p.world = 64, 1 << 20, 1, 0, 2
    _fill(p, kw)
    return _refusal(lib, lib.hyd_allreduce_sum(C.byref(p), None))


def _r_constrained(lib, kw):
    """hyd_sample_tokens_constrained: "c.<field>" breaks the hyd_token_dfa, no_dfa passes none (the penalised sampler's call)."""
    kw = dict(kw)
    null, no_dfa = kw.pop("null", False), kw.pop("no_dfa", False)
    c = token_dfa(**{k[2:]: kw.pop(k) for k in list(kw) if k.startswith("c.")})
    p = None if null else C.byref(sample_penalty(**kw))
    return _refusal(lib, lib.hyd_sample_tokens_constrained(p, None if no_dfa else C.byref(c), None))


def _r_accept_states(lib, kw):
    kw = dict(kw)
    null, after, state = kw.pop("null", False), kw.pop("step_state_after", PTR), kw.pop("state", PTR)
    p = None if null else C.byref(draft_accept(**kw))
    return _refusal(lib, lib.hyd_draft_accept_states(p, after, state, None))


_FAILED = " failed: hip error "


def _launch(rec):
    """A refusal runner's answer -> the record of a launch case: the code and the name of the launch that was reached."""
    what, sep, _ = rec["error"].partition(_FAILED)
    if rec["rc"] != HYD_ERR_LAUNCH or not sep:
        return rec  # not a launch: the whole answer, which no recorded launch equals
    return {"rc": rec["rc"], "what": what}


def device_present():
    import torch

    return torch.cuda.is_available()


QUERIES = {"prefix": _q_prefix, "decode": _q_decode, "decode_kvq": _q_decode_kvq, "workspace": _q_workspace, "kv_quant": _q_kvq, "null": _q_null,
           "allreduce_block": _q_block, "narrow_kv": _q_narrow, "linear_w8_workspace": _q_w8_workspace}
REFUSALS = {
    "hyd_prefix_attn_fwd": _params_runner("hyd_prefix_attn_fwd", lambda **kw: prefix(ptrs=True, **kw)),
    "hyd_suffix_attn_fwd": _params_runner("hyd_suffix_attn_fwd", suffix),
    "hyd_suffix_attn_fwd_kvq": _params_runner("hyd_suffix_attn_fwd_kvq", suffix, with_kq=True),
    "hyd_decode_attn_fused": _params_runner("hyd_decode_attn_fused", lambda **kw: decode(ptrs=True, **kw)),
    "hyd_decode_attn_fused_kvq": _params_runner("hyd_decode_attn_fused_kvq", lambda **kw: decode(ptrs=True, **kw), with_kq=True),
    "hyd_rope_append_decode": _params_runner("hyd_rope_append_decode", rope),
    "hyd_rope_append_decode_kvq": _params_runner("hyd_rope_append_decode_kvq", rope, with_kq=True),
    "hyd_add_rmsnorm": _params_runner("hyd_add_rmsnorm", rmsnorm),
    "hyd_swiglu": _params_runner("hyd_swiglu", swiglu),
    "hyd_sample_tokens": _params_runner("hyd_sample_tokens", sample),
    "hyd_sample_tokens_filtered": _params_runner("hyd_sample_tokens_filtered", sample_filter),
    "hyd_sample_tokens_penalized": _params_runner("hyd_sample_tokens_penalized", sample_penalty),
    "hyd_token_bitmap_build": _params_runner("hyd_token_bitmap_build", bitmap),
    "hyd_token_logprobs": _params_runner("hyd_token_logprobs", token_logprob),
    "hyd_stop_update": _params_runner("hyd_stop_update", stop),
    "hyd_combine_lse": _r_combine,
    "hyd_allreduce_sum": _r_allreduce,
    "hyd_suffix_attn_causal_fwd": _params_runner("hyd_suffix_attn_causal_fwd", lambda **kw: suffix(**{"nq": 2, **kw})),
    "hyd_suffix_attn_causal_fwd_kvq": _params_runner("hyd_suffix_attn_causal_fwd_kvq", lambda **kw: suffix(**{"nq": 2, **kw}), with_kq=True),
    "hyd_rope_append_multi": _params_runner("hyd_rope_append_multi", rope_multi),
    "hyd_sample_tokens_constrained": _r_constrained,
    "hyd_draft_lookup": _params_runner("hyd_draft_lookup", draft_lookup),
    "hyd_dfa_forced_tokens": _params_runner("hyd_dfa_forced_tokens", dfa_forced),
    "hyd_draft_constrain": _params_runner("hyd_draft_constrain", draft_constrain),
    "hyd_draft_accept": _params_runner("hyd_draft_accept", draft_accept),
    "hyd_draft_accept_states": _r_accept_states,
    "hyd_kv_promote": _params_runner("hyd_kv_promote", kv_promote),
    "hyd_kv_gather_paths": _params_runner("hyd_kv_gather_paths", kv_gather),
    "hyd_kv_absmax": _params_runner("hyd_kv_absmax", kv_absmax),
    "hyd_kv_scales_from_absmax": _params_runner("hyd_kv_scales_from_absmax", kv_scales),
    "hyd_linear_w8": _params_runner("hyd_linear_w8", linear_w8),
    "hyd_weight_widen": _params_runner("hyd_weight_widen", weight_widen),
}

# ---- the cases: (kind, entry, arguments) ------------------------------------------------------------------------------------
_Q, _R, _N, _L = [], [], [], []


def q(entry, **kw):
    _Q.append((entry, kw))


def r(entry, **kw):
    _R.append((entry, kw))


def noop(entry, **kw):
    """A call that returns HYD_OK before any HIP call (through the entry's refusal runner); its record is the return code alone."""
    _N.append((entry, kw))


def launch(entry, **kw):
    """A call that is accepted (through the entry's refusal runner): without a device its record is HYD_ERR_LAUNCH and the launch reached."""
    _L.append((entry, kw))


def chain(entry, steps, pairs=True, **base):
    """steps: one breaking dict per check, in the order of the checks; a list of dicts where one check (one message) reads several
    fields.  Every dict alone, and every two neighbouring checks together: the earlier one answers, so swapping two adjacent checks
    changes a record.  (Neighbours that can only be broken through the same field are not paired.)"""
    steps = [s if isinstance(s, list) else [s] for s in steps]
    for i, alts in enumerate(steps):
        for s in alts:
            r(entry, **base, **s)
        if pairs and i + 1 < len(steps):
            both = [(a, b) for a in reversed(alts) for b in steps[i + 1] if not set(a) & set(b)]
            if both:
                r(entry, **base, **both[0][0], **both[0][1])


# the prefix planner (hyd_prefix_plan + hyd_prefix_workspace_bytes)
for n in (0, 1, 255, 256, 257, 512, 1024):
    q("prefix", kv_len=n)
q("prefix", B=129, Hq=128, Hkv=128)            # units128 = 256: 128-row workgroups, two row blocks
q("prefix", B=129, Hq=129, Hkv=129)            # units128 = 258: 256-row workgroups, one row block
q("prefix", B=1, Hq=256, Hkv=256)              # units128 = 256
q("prefix", B=1, Hq=257, Hkv=257)              # units128 = 257
q("prefix", B=129, Hq=129, Hkv=129, D=256)     # D = 256 never takes 256 rows
q("prefix", B=129, Hq=129, Hkv=129, D=64)
q("prefix", B=4, kv_len=1024)                  # max_by_len wins
q("prefix", B=64, Hq=32, Hkv=8, kv_len=4096)   # by_cost wins
q("prefix", B=64, Hq=32, Hkv=8, kv_len=16384)
q("prefix", B=64, Hq=32, Hkv=8, kv_len=16384, D=64)
q("prefix", B=64, Hq=32, Hkv=8, kv_len=16384, D=256)
q("prefix", B=1, Hq=1, Hkv=1, kv_len=8192)     # want and by_cost beyond the cap of 32
q("prefix", B=16, Hq=16, Hkv=16, kv_len=2048)  # units = kNumCU / 2 ...
q("prefix", B=129, Hq=16, Hkv=16, kv_len=2048, sb=1)
q("prefix", B=8, sb=8, Hq=17, Hkv=17, kv_len=2048)  # ... and just above: unsplit
for ns in (1, 2, 7, 32, 33, 1000):
    q("prefix", kv_len=4096, num_splits=ns)
q("prefix", kv_len=100, num_splits=4)
q("prefix", B=12, sb=3, kv_len=700)
q("prefix", B=12, nq=3, Hq=8, Hkv=2, kv_len=700, causal=1)
q("prefix", B=40, cu_seqlens_q=PTR, max_q_len=24, sb=3, kv_len=4096)   # packed queries: one split
q("prefix", B=40, cu_seqlens_q=PTR, max_q_len=24, sb=3, kv_len=4096, num_splits=8)
q("prefix", B=40, cu_seqlens_q=PTR, max_q_len=24, sb=3, nq=2)
q("prefix", B=40, cu_seqlens_q=PTR, max_q_len=0, sb=3)
q("prefix", B=40, cu_seqlens_k=PTR, sb=4, kv_len=3000)
q("prefix", kv_len=2048, num_splits=1, k_tok_stride=1 << 20, v_tok_stride=1024)     # 2 GiB per split: cut into 4
q("prefix", kv_len=2048, num_splits=1, k_tok_stride=1024, v_tok_stride=1 << 20)
q("prefix", kv_len=16384, k_tok_stride=1 << 20, v_tok_stride=1 << 20)               # 32 x 512 keys: still fits
q("prefix", kv_len=16385, k_tok_stride=1 << 20, v_tok_stride=1 << 20)               # 33 splits: refused
q("prefix", B=40, cu_seqlens_q=PTR, max_q_len=24, sb=3, kv_len=2048, k_tok_stride=1 << 20)  # packed queries cannot be cut
q("prefix", k_tok_stride=1 << 22, v_tok_stride=8)    # max_rows = 0
q("prefix", k_tok_stride=(1 << 21) - 8)              # max_rows just above / below 128 ...
q("prefix", k_tok_stride=1 << 21)
q("prefix", k_tok_stride=1677721)
q("prefix", k_tok_stride=1677722)
q("prefix", B=65536, sb=65536, Hq=65536, Hkv=65536)  # grid too large
for bad in (dict(D=96), dict(dtype=2), dict(dtype=3), dict(B=10, sb=3), dict(Hq=8, Hkv=5), dict(B=0), dict(nq=0), dict(Hkv=0),
            dict(sb=0), dict(sb=-1), dict(kv_len=-1), dict(softmax_scale=-1.0), dict(softmax_scale=NAN), dict(softmax_scale=2.0e4),
            dict(softmax_scale=0.25), dict(D=96, dtype=2), dict(sb=0, softmax_scale=-1.0), dict(kv_len=-1, sb=0)):
    q("prefix", **bad)
q("null")

# the decode planner (hyd_decode_workspace_bytes at f32_partials 0 / 1, hyd_decode_two_stream_ok, hyd_decode_kv_quant_supported)
for n_levels in (-1, 0, 9):
    q("decode", n_levels=n_levels)
    q("decode", n_levels=n_levels, kv_len=0)
for B in (64, 65):      # level_is_small: 64 / 65 query rows per (group, kv head)
    for P in (1024, 1025):  # ... and 1024 / 1025 keys
        for D in (64, 128, 256):
            q("decode", B=B, Hq=2, Hkv=2, D=D, levels=((1, P),))
q("decode", B=16, Hq=16, Hkv=4, levels=((1, 1024),))   # 64 rows through the group factor
q("decode", B=17, Hq=16, Hkv=4, levels=((1, 1024),))
q("decode", B=16, Hq=2, Hkv=2, levels=((1, 1024, 1 << 20),))   # a small level's span stays below 2 GiB ...
q("decode", B=16, Hq=2, Hkv=2, levels=((1, 1024, 1 << 21),))   # ... or it is no small level (and here no level at all)
q("decode", B=16, Hq=2, Hkv=2, levels=((4, 300),), **{"levels.0.cu_seqlens_k": PTR})
for S in (0, 16):       # the prefix-only form plans with the default cap, every other form with the levels' shared budget
    q("decode", B=4, kv_len=S, levels=((1, 1024),))
    q("decode", B=4, kv_len=S, levels=((1, 4096),))
    q("decode", B=1, Hq=1, Hkv=1, kv_len=S, levels=((1, 8192),))
    q("decode", B=64, Hq=8, Hkv=1, kv_len=S, levels=((1, 16384),))
    q("decode", B=64, Hq=8, Hkv=1, kv_len=S, levels=((1, 16384), (2, 16384), (4, 16384)))
    q("decode", B=1, Hq=1, Hkv=1, kv_len=S, levels=((1, 8192),) * 3)
    q("decode", B=1, Hq=1, Hkv=1, kv_len=S, levels=((1, 8192),) * 8)
    q("decode", B=96, Hq=8, Hkv=2, kv_len=S, levels=((1, 2048), (4, 96)))        # one split level + one small level
    q("decode", B=32, Hq=8, Hkv=8, kv_len=S, levels=((1, 300), (2, 200), (8, 77)))
    q("decode", B=33, nq=3, Hq=3, Hkv=1, D=64, kv_len=S, levels=((1, 257),))     # odd sizes: the 256-byte padding shows
    q("decode", B=33, nq=3, Hq=3, Hkv=1, D=64, kv_len=S, levels=((1, 4099), (3, 1300), (11, 129)))
    q("decode", B=4, kv_len=S, levels=((1, 0),))
    q("decode", B=4, kv_len=S, levels=((1, 64), (3, 64)))      # a level that does not plan: the query answers 0
    q("decode", B=4, kv_len=S, levels=((3, 1024),))
q("decode", kv_len=-1)
q("decode", D=96)
# the one-launch rule: B * Hkv * (P + S) of 8192 / 8193, equal / unequal token strides, with and without the flag and an LSE
for S in (7168, 7169):
    for sls in (0, 1):
        q("decode", B=1, Hq=4, Hkv=1, kv_len=S, levels=((1, 1024),), single_launch_small=sls)
    q("decode", B=1, Hq=4, Hkv=1, kv_len=S, levels=((1, 1024, 256),), single_launch_small=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=33, levels=((1, 96),), single_launch_small=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1, **{"suffix.lse": PTR})
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1, phase=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((4, 96),), single_launch_small=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((3, 96),), single_launch_small=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 48), (2, 48)), single_launch_small=1)
q("decode", B=8, Hq=32, Hkv=8, kv_len=32, levels=((2, 96),), single_launch_small=1, **{"levels.0.cu_seqlens_k": PTR})
q("decode", B=8, Hq=32, Hkv=32, kv_len=32, levels=((1, 96),), single_launch_small=1)   # Hq == Hkv ignores the flag
q("decode", B=8, Hq=16, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1)    # 2-row units: not native
q("decode", B=8, Hq=32, Hkv=8, D=256, kv_len=32, levels=((1, 96),), single_launch_small=1)
for phase in (0, 1, 2, 3, 4):
    q("decode", B=96, Hq=8, Hkv=2, kv_len=16, levels=((1, 2048),), phase=phase)

for lv in ((), ((1, 1024),), ((1, 1024), (32, 64)), ((1, 4096), (2, 300), (4, 64)), ((1, 8192),) * 8, ((1, 8192),) * 9, ((3, 64),)):
    q("workspace", B=64, Hq=8, Hkv=8, D=128, levels=lv)
q("workspace", B=64, Hq=8, Hkv=8, D=128, levels=(), n_levels=-1)
q("workspace", B=33, nq=3, Hq=3, Hkv=1, D=64, levels=((1, 4099), (3, 1300), (11, 129)))
q("workspace", B=64, Hq=8, Hkv=8, D=96, levels=((1, 1024),))

for shape in (dict(Hq=32, Hkv=8), dict(Hq=12, Hkv=4), dict(Hq=4, Hkv=2), dict(Hq=8, Hkv=8), dict(Hq=8, Hkv=8, nq=2), dict(Hq=2, Hkv=2),
              dict(Hq=4, Hkv=4), dict(Hq=4, Hkv=4, D=64), dict(Hq=8, Hkv=8, D=64), dict(Hq=2, Hkv=2, D=256), dict(Hq=32, Hkv=8, D=96),
              dict(Hq=8, Hkv=1, D=256), dict(Hq=8, Hkv=1, D=256, B=2048), dict(Hq=8, Hkv=1, D=256, kv_len=200),
              dict(Hq=32, Hkv=8, dtype=0), dict(Hq=32, Hkv=8, dtype=2), dict(Hq=32, Hkv=8, B=0), dict(Hq=32, Hkv=8, kv_dtype=1),
              dict(Hq=4, Hkv=2, kv_dtype=1), dict(Hq=32, Hkv=8, kv_dtype=0), dict(Hq=32, Hkv=8, kv_dtype=7),
              dict(Hq=32, Hkv=8, kv_len=1 << 20)):
    q("kv_quant", **shape)

for world, max_bytes in ((0, 1024), (1, 1024), (2, 1), (2, 1000), (8, 1 << 20), (8, (1 << 20) + 1), (9, 1024), (-1, 1024), (4, 0)):
    q("allreduce_block", world=world, max_bytes=max_bytes)

# ---- refusals ------------------------------------------------------------------------------------------------------------
_STRIDES6 = ("k_{}_stride", "v_{}_stride")

# hyd_prefix_attn_fwd
r("hyd_prefix_attn_fwd", null=True)
for bad in (dict(D=96), dict(dtype=2), dict(B=10, sb=3), dict(sb=0), dict(kv_len=-1), dict(softmax_scale=-1.0), dict(k_tok_stride=1 << 22),
            dict(kv_len=16385, k_tok_stride=1 << 20, v_tok_stride=1 << 20), dict(cu_seqlens_q=PTR, nq=2), dict(cu_seqlens_q=PTR),
            dict(q=None), dict(q=MIS8), dict(k=None), dict(k=MIS8), dict(v=None), dict(v=ODD), dict(out=None), dict(out=MIS8),
            dict(kv_len=0), dict(kv_len=0, out=None), dict(q=None, D=96), dict(k=None, q=MIS8), dict(k_group_stride=4, q=None),
            dict(kv_len=1024, workspace=None), dict(kv_len=1024, workspace_bytes=1000), dict(kv_len=1024, workspace_bytes=4096),
            dict(kv_len=4096, B=3, Hq=3, Hkv=1, D=64, workspace_bytes=0), dict(kv_len=1024, workspace_bytes=0, out=None)):
    r("hyd_prefix_attn_fwd", **bad)
for g in ("group", "tok", "head"):
    for t in _STRIDES6:
        r("hyd_prefix_attn_fwd", **{t.format(g): 12})

# hyd_suffix_attn_fwd and its _kvq twin
_SUFFIX_BAD = (dict(D=96), dict(dtype=2), dict(B=0), dict(Hq=8, Hkv=3), dict(softmax_scale=-0.5), dict(softmax_scale=INF), dict(kv_len=-1),
               dict(q=None), dict(q=MIS8), dict(out=None), dict(out=ODD), dict(k=None), dict(k=MIS8), dict(v=None), dict(v=MIS8),
               dict(n_partials=-1), dict(n_partials=9), dict(kv_len=0), dict(kv_len=0, n_partials=9), dict(kv_len=0, k=None),
               dict(D=96, q=None), dict(q=None, out=None), dict(k=MIS8, n_partials=-1),
               dict(n_partials=1), dict(n_partials=2, **{"partials.0.out": PTR, "partials.0.lse": PTR, "partials.0.count": 1}),
               dict(n_partials=1, **{"partials.0.out": PTR, "partials.0.lse": PTR, "partials.0.count": 0}),
               dict(n_partials=1, **{"partials.0.out": PTR, "partials.0.count": 1}),
               dict(kv_len=1 << 21, k_tok_stride=1024), dict(kv_len=1 << 21, v_tok_stride=512), dict(kv_len=1 << 20, k_tok_stride=1024),
               dict(Hq=4 * 65535 + 1, Hkv=4 * 65535 + 1), dict(nq=8 * 65535 + 1), dict(kv_len=1 << 21, k_tok_stride=1024, nq=8 * 65535 + 1))
for bad in _SUFFIX_BAD:
    r("hyd_suffix_attn_fwd", **bad)
for g in ("batch", "tok", "head"):
    for t in _STRIDES6:
        r("hyd_suffix_attn_fwd", **{t.format(g): 4})
_MANY = {f"partials.{i}.{f}": v for i in range(8) for f, v in (("out", PTR), ("lse", PTR), ("count", 9))}
r("hyd_suffix_attn_fwd", n_partials=8, **_MANY)                    # 72 slices: more than the epilogue merges
r("hyd_suffix_attn_fwd", n_partials=8, kv_len=1 << 21, k_tok_stride=1024, **_MANY)
r("hyd_suffix_attn_fwd_kvq", null=True)
r("hyd_suffix_attn_fwd_kvq", null=True, kq=dict(kv_dtype=7))
for kq in (None, dict()):
    for bad in _SUFFIX_BAD:
        if kq is None or bad != dict(kv_len=1 << 20, k_tok_stride=1024):  # (2^30 bytes of fp8: taken)
            r("hyd_suffix_attn_fwd_kvq", kq=kq, **bad)
for bad in (dict(), dict(D=96), dict(q=None), dict(n_partials=9), dict(kv_len=0)):
    r("hyd_suffix_attn_fwd_kvq", kq=dict(kv_dtype=7), **bad)
    r("hyd_suffix_attn_fwd_kvq", kq=dict(kv_dtype=0), **bad)
    r("hyd_suffix_attn_fwd_kvq", kq=dict(k_scale=PTR + 2), **bad)
    r("hyd_suffix_attn_fwd_kvq", kq=dict(v_scale=PTR + 1), **bad)
for shape in (dict(Hq=4, Hkv=2), dict(Hq=2, Hkv=2), dict(Hq=8, Hkv=8, nq=2), dict(Hq=4, Hkv=4, D=64), dict(Hq=8, Hkv=1, D=256),
              dict(Hq=32, Hkv=8), dict(Hq=4, Hkv=2, kv_len=1 << 21, k_tok_stride=1024)):
    r("hyd_suffix_attn_fwd_kvq", kq=dict(), **shape)                # without HYD_KVQ_GQA
    if shape["Hq"] // shape["Hkv"] * shape.get("nq", 1) < 3:
        r("hyd_suffix_attn_fwd_kvq", kq=dict(flags=1), **shape)
r("hyd_suffix_attn_fwd_kvq", kq=dict(), kv_len=1 << 20, k_tok_stride=2048)   # fp8 spans count bytes: 2^31 is refused ...
r("hyd_suffix_attn_fwd_kvq", kq=dict(flags=1), Hq=32, Hkv=8, kv_len=1 << 20, k_tok_stride=2048)
r("hyd_suffix_attn_fwd", kv_len=1 << 20, k_tok_stride=2048)                  # ... as for 16-bit caches, which count two per element

# hyd_decode_attn_fused and its _kvq twin
_DECODE_BAD = (dict(n_levels=-1), dict(n_levels=9), dict(phase=-1), dict(phase=5), dict(phase=7, n_levels=9), dict(shared_max_workgroups=-1),
               dict(f32_partials=2), dict(f32_partials=-1), dict(f32_partials=2, shared_max_workgroups=-1, phase=9),
               dict(D=96), dict(**{"suffix.dtype": 2}), dict(B=0), dict(Hq=8, Hkv=3), dict(**{"suffix.softmax_scale": -1.0}), dict(kv_len=-1),
               dict(**{"suffix.q": None}), dict(**{"suffix.q": MIS8}), dict(**{"suffix.out": None}), dict(**{"suffix.out": MIS8}),
               dict(**{"suffix.k": None}), dict(**{"suffix.k": MIS8}), dict(**{"suffix.v": None}), dict(**{"suffix.v": ODD}),
               dict(**{"suffix.k_tok_stride": 4}), dict(**{"suffix.v_batch_stride": 4}), dict(**{"suffix.q": None}, f32_partials=2),
               dict(levels=(), kv_len=0), dict(levels=(), kv_len=0, phase=3), dict(levels=(), phase=3), dict(levels=(), phase=4),
               dict(kv_len=0, phase=3), dict(kv_len=0, phase=4), dict(kv_len=0, phase=4, levels=((1, 64), (2, 64))),
               # the prefix-only form
               dict(kv_len=0, levels=((3, 64),)), dict(kv_len=0, levels=((0, 64),)), dict(kv_len=0, levels=((1, 0),)),
               dict(kv_len=0, levels=((1, 64, 1 << 22),)), dict(kv_len=0, **{"levels.0.k": None}), dict(kv_len=0, **{"levels.0.v": MIS8}),
               dict(kv_len=0, **{"levels.0.k_head_stride": 4}), dict(kv_len=0, levels=((1, 0),), **{"levels.0.k": None}),
               dict(kv_len=0, levels=((1, 1024),), workspace=None), dict(kv_len=0, levels=((1, 1024),), workspace_bytes=4096),
               dict(kv_len=0, levels=((1, 1024),), workspace_bytes=0, f32_partials=1),
               dict(kv_len=0, B=1, Hq=1, Hkv=1, levels=((1, 8192),), workspace_bytes=0),
               dict(kv_len=0, B=1, Hq=1, Hkv=1, levels=((1, 8192),), workspace_bytes=0, phase=1),
               # levels that do not plan, in level order
               dict(levels=((3, 64),)), dict(levels=((1, 64), (3, 64))), dict(levels=((1, 64), (1, 0))), dict(levels=((1, 0), (3, 64))),
               dict(levels=((1, 64), (2, 64, 1 << 22))), dict(levels=((1, 64), (2, 64)), **{"levels.1.k": None}),
               dict(levels=((1, 64), (2, 64)), **{"levels.1.v": MIS8, "levels.0.v_tok_stride": 12}),
               dict(levels=((1, 64), (2, 64)), **{"levels.1.k_group_stride": 4}), dict(levels=((1, 0),), **{"levels.0.k": None}),
               dict(levels=((1, 16385, 1 << 20),)))
for bad in _DECODE_BAD:
    r("hyd_decode_attn_fused", **bad)
# the workspace each form asks for: in-order and two-stream phases, 16-bit and fp32 partials, small / unsplit / split levels
_WS_SHAPES = (dict(B=96, Hq=8, Hkv=2, levels=((1, 2048), (4, 96))), dict(B=33, nq=3, Hq=3, Hkv=1, D=64, levels=((1, 4099), (3, 1300), (11, 129))),
              dict(B=4, levels=((1, 64),)), dict(B=65, Hq=2, Hkv=2, levels=((1, 64),)), dict(B=1, Hq=1, Hkv=1, levels=((1, 8192),) * 8),
              dict(B=1, Hq=4, Hkv=1, kv_len=7169, levels=((1, 1024),), single_launch_small=1),
              dict(B=32, Hq=8, Hkv=8, kv_len=0, levels=((1, 300), (2, 200), (8, 77))))
for shape in _WS_SHAPES:
    for phase in (0, 1, 2, 3, 4):
        for f32 in (0, 1):
            r("hyd_decode_attn_fused", workspace_bytes=255, phase=phase, f32_partials=f32, **shape)
r("hyd_decode_attn_fused", workspace=None, **_WS_SHAPES[0])
# more partials than one merge takes: two levels of 32 slices + the unique partial of the two-stream form
r("hyd_decode_attn_fused", B=1, Hq=1, Hkv=1, levels=((1, 8192),) * 2, phase=3)
r("hyd_decode_attn_fused", B=1, Hq=1, Hkv=1, levels=((1, 8192),) * 2, phase=4)
r("hyd_decode_attn_fused", B=1, Hq=1, Hkv=1, levels=((1, 8192),) * 8, phase=4, workspace_bytes=0)
r("hyd_decode_attn_fused", B=1, Hq=1, Hkv=1, levels=((1, 8192),) * 2, phase=2, workspace_bytes=0)
# what the unique pass refuses after the levels are carved (HYD_PHASE_UNIQUE / UNIQUE_PARTIAL launch nothing before it)
for phase in (2, 3):
    r("hyd_decode_attn_fused", phase=phase, kv_len=1 << 20, **{"suffix.k_tok_stride": 1024})
    r("hyd_decode_attn_fused", phase=phase, Hq=4 * 65535 + 1, Hkv=4 * 65535 + 1)
    r("hyd_decode_attn_fused_kvq", kq=dict(), phase=phase, kv_len=1 << 20, **{"suffix.k_tok_stride": 2048})
r("hyd_decode_attn_fused_kvq", null=True)
r("hyd_decode_attn_fused_kvq", null=True, kq=dict())
for kq in (dict(kv_dtype=1),):
    for bad in _DECODE_BAD:
        r("hyd_decode_attn_fused_kvq", kq=kq, **bad)
for bad in (dict(), dict(D=96), dict(phase=7), dict(n_levels=9), dict(**{"suffix.q": None})):
    r("hyd_decode_attn_fused_kvq", kq=dict(kv_dtype=7), **bad)
    r("hyd_decode_attn_fused_kvq", kq=dict(k_scale=PTR + 2), **bad)
for phase in (0, 1, 2, 3, 4, 5):   # the fp8 shapes are validated for every phase
    r("hyd_decode_attn_fused_kvq", kq=dict(), phase=phase, Hq=4, Hkv=2)
    r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), phase=phase, Hq=4, Hkv=2)
    r("hyd_decode_attn_fused_kvq", kq=dict(), phase=phase, Hq=32, Hkv=8)
    if phase in (0, 5):  # only HYD_PHASE_ALL has a one-launch form
        r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), phase=phase, B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1)
r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), B=1, Hq=4, Hkv=1, kv_len=7168, levels=((1, 1024),), single_launch_small=1)
r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), B=1, Hq=4, Hkv=1, kv_len=7169, levels=((1, 1024),), single_launch_small=1, workspace_bytes=0)
r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), B=1, Hq=4, Hkv=1, kv_len=7168, levels=((1, 1024, 256),), single_launch_small=1, workspace_bytes=0)
r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), B=8, Hq=32, Hkv=8, kv_len=32, levels=((3, 96),), single_launch_small=1)
r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1, n_levels=9)
for bad in (dict(n_levels=9), dict(phase=7), dict(kv_len=0, levels=((3, 64),)), dict(levels=((1, 64), (3, 64))), dict(workspace_bytes=0),
            dict(kv_len=0, workspace_bytes=0, levels=((1, 1024),)), dict(kv_len=0, levels=(), phase=0), dict(Hq=4, Hkv=2, kv_len=0, levels=((1, 0),))):
    r("hyd_decode_attn_fused_kvq", kq=dict(), **bad)
    r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), Hq=32 if "Hq" not in bad else bad["Hq"], **{k: v for k, v in bad.items() if k != "Hq"})

# hyd_rope_append_decode and its _kvq twin
_ROPE_PTRS = ("q", "k", "v", "q_out", "k_cache", "v_cache", "cos", "sin")
_ROPE_STRIDES = ("q_batch_stride", "k_batch_stride", "v_batch_stride", "kc_batch_stride", "kc_tok_stride", "kc_head_stride",
                 "vc_batch_stride", "vc_tok_stride", "vc_head_stride")
_ROPE_BAD = ([dict(D=96), dict(dtype=2), dict(B=0), dict(Hq=8, Hkv=3), dict(position_ids=None), dict(seq_lens=None), dict(cs_stride=6),
              dict(cache_len=0), dict(max_pos=0), dict(max_pos=0, cache_len=0), dict(D=96, q=None), dict(sin=None, q_batch_stride=4),
              dict(position_ids=None, kc_tok_stride=4)]
             + [{n: None} for n in _ROPE_PTRS] + [{n: MIS8} for n in _ROPE_PTRS] + [{n: 4} for n in _ROPE_STRIDES])
r("hyd_rope_append_decode", null=True)
r("hyd_rope_append_decode_kvq", null=True)
r("hyd_rope_append_decode_kvq", null=True, kq=dict(kv_dtype=7))
for bad in _ROPE_BAD:
    r("hyd_rope_append_decode", **bad)
    r("hyd_rope_append_decode_kvq", kq=dict(), **bad)
for bad in (dict(), dict(D=96), dict(q=None), dict(B=0)):   # a shape error is reported before a hyd_kv_quant error
    r("hyd_rope_append_decode_kvq", kq=dict(kv_dtype=7), **bad)
    r("hyd_rope_append_decode_kvq", kq=dict(v_scale=PTR + 2), **bad)
r("hyd_rope_append_decode_kvq", kq=None, q=None)
r("hyd_rope_append_decode_kvq", kq=dict(kv_dtype=1), q=None)

# the layer glue
for bad in ([dict(dtype=2), dict(rows=-1), dict(rows=1 << 31), dict(n=0), dict(n=12), dict(n=16392), dict(x=None), dict(weight=None),
             dict(norm_out=None), dict(x=MIS8), dict(weight=MIS8), dict(norm_out=MIS8), dict(x_row_stride=4), dict(norm_row_stride=4),
             dict(residual=MIS8), dict(residual=PTR, residual_row_stride=4), dict(residual=PTR, sum_out=MIS8),
             dict(residual=PTR, sum_out=PTR, sum_row_stride=4), dict(dtype=2, n=12), dict(n=12, x=None), dict(x=None, rows=-1),
             dict(x=MIS8, norm_row_stride=4), dict(residual=MIS8, x_row_stride=4)]):
    r("hyd_add_rmsnorm", **bad)
r("hyd_add_rmsnorm", null=True)
for bad in ([dict(dtype=2), dict(rows=-1), dict(n=0), dict(n=12), dict(rows=(1 << 40) + 1, n=8 << 20), dict(gate=None), dict(up=None), dict(out=None),
             dict(gate=MIS8), dict(up=MIS8), dict(out=MIS8), dict(gate_row_stride=4), dict(up_row_stride=4), dict(out_row_stride=4),
             dict(dtype=2, n=12), dict(n=12, gate=None), dict(up=None, gate=MIS8), dict(out=MIS8, gate_row_stride=4)]):
    r("hyd_swiglu", **bad)
r("hyd_swiglu", null=True)

# the logits entry points
_ROW_BAD = [dict(dtype=3), dict(dtype=-1), dict(rows=-1), dict(n=0), dict(logits=None), dict(out=None), dict(temperature=-1.0),
            dict(temperature=NAN), dict(row_stride=63), dict(logits=ODD), dict(logits=PTR + 2, dtype=2), dict(out=PTR + 4),
            dict(dtype=3, rows=-1), dict(rows=-1, logits=None), dict(logits=None, temperature=-1.0), dict(temperature=-1.0, row_stride=63),
            dict(row_stride=63, logits=ODD)]
_FILTER_BAD = _ROW_BAD + [dict(n=MAX_N + 1, row_stride=MAX_N + 1), dict(n=MAX_N + 1, logits=None), dict(top_k=-1), dict(top_p=0.0),
                          dict(top_p=1.5), dict(top_p=NAN), dict(min_p=-0.5), dict(min_p=1.5), dict(min_p=NAN), dict(logprobs=PTR + 2),
                          dict(kept=PTR + 1), dict(temperature=-1.0, top_k=-1), dict(top_k=-1, top_p=0.0), dict(top_p=0.0, min_p=2.0),
                          dict(min_p=2.0, row_stride=63), dict(row_stride=63, kept=PTR + 1)]
_PENALTY_BAD = _FILTER_BAD + [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=INF), dict(repetition_penalty=NAN),
    dict(frequency_penalty=INF), dict(presence_penalty=NAN), dict(n_context=-1), dict(n_context=10), dict(n_context=1),
    dict(n_context=2, **{"context.0.bits": PTR, "context.0.rows_per_group": 1, "context.1.bits": PTR}),
    dict(n_context=1, **{"context.0.bits": PTR + 2, "context.0.rows_per_group": 1}), dict(gen=PTR), dict(gen_len=PTR), dict(gen_stride=-1),
    dict(gen_stride=2049), dict(append_out=1), dict(n_bias=-1), dict(n_bias=1025), dict(n_bias=1), dict(n_bias=1, bias_ids=PTR),
    dict(gen=PTR + 2, gen_len=PTR), dict(gen=PTR, gen_len=PTR + 2), dict(n_bias=1, bias_ids=PTR + 4, bias_values=PTR),
    dict(n_bias=1, bias_ids=PTR, bias_values=PTR + 2), dict(row_stride=63, repetition_penalty=0.0), dict(repetition_penalty=0.0, frequency_penalty=INF),
    dict(presence_penalty=INF, n_context=-1), dict(n_context=1, gen=PTR), dict(gen=PTR, gen_stride=-1), dict(gen_stride=2049, append_out=1),
    dict(append_out=1, n_bias=-1), dict(n_bias=1, logits=ODD), dict(kept=PTR + 1, gen=PTR + 2, gen_len=PTR)]
for entry, bads in (("hyd_sample_tokens", _ROW_BAD), ("hyd_sample_tokens_filtered", _FILTER_BAD), ("hyd_sample_tokens_penalized", _PENALTY_BAD)):
    r(entry, null=True)
    for bad in bads:
        r(entry, **bad)
r("hyd_token_logprobs", null=True)
for bad in (dict(dtype=3), dict(rows=-1), dict(rows=(1 << 31) + 1), dict(n=0), dict(n=MAX_N + 1, row_stride=MAX_N + 1), dict(logits=None),
            dict(targets=None), dict(logprobs=None), dict(greedy=None), dict(top_n=-1), dict(top_n=21), dict(top_n=2), dict(top_n=2, top_ids=PTR),
            dict(row_stride=63), dict(logits=ODD), dict(logits=PTR + 2, dtype=2), dict(targets=PTR + 4), dict(logprobs=PTR + 2),
            dict(top_ids=PTR + 4), dict(top_logprobs=PTR + 2), dict(dtype=3, rows=-1), dict(rows=-1, n=MAX_N + 1), dict(n=MAX_N + 1, logits=None),
            dict(greedy=None, top_n=-1), dict(top_n=2, row_stride=63), dict(row_stride=63, logits=ODD)):
    r("hyd_token_logprobs", **bad)
r("hyd_token_bitmap_build", null=True)
for bad in (dict(groups=-1), dict(groups=65536), dict(L=-1), dict(n=0), dict(n=MAX_N + 1), dict(ids=None), dict(bits=None), dict(id_stride=7),
            dict(ids=PTR + 4), dict(lens=PTR + 4), dict(bits=PTR + 2), dict(groups=-1, n=0), dict(n=0, ids=None), dict(bits=None, id_stride=7),
            dict(id_stride=7, ids=PTR + 4)):
    r("hyd_token_bitmap_build", **bad)
r("hyd_stop_update", null=True)
_STOP_PTRS8 = ("tok", "out", "stop_tokens", "start_pos", "shared_len", "feed", "next_pos")
_STOP_PTRS4 = ("length", "reason", "stop_index", "live")
for bad in ([dict(rows=-1), dict(n_eos=-1), dict(n_eos=17), dict(n_stop=-1), dict(n_stop=33), dict(n_stop=1), dict(n_stop=2, **{"stop_lens.0": 3, "stop_lens.1": 17}),
             dict(t=-1), dict(t=8), dict(n_stop=1, **{"stop_lens.0": 3}), dict(rows=-1, n_eos=17), dict(n_eos=17, n_stop=33), dict(n_stop=1, t=-1),
             dict(t=8, tok=None), dict(tok=None, feed=None), dict(feed=None, n_stop=1, **{"stop_lens.0": 3}),
             dict(n_stop=1, tok=PTR + 4, **{"stop_lens.0": 3}), dict(tok=PTR + 4, live=PTR + 2), dict(rows=0, live=PTR + 2)]
            + [{n: None} for n in _STOP_PTRS8 + _STOP_PTRS4 if n not in ("stop_tokens", "shared_len")]
            + [{n: PTR + 4} for n in _STOP_PTRS8] + [{n: PTR + 2} for n in _STOP_PTRS4]):
    r("hyd_stop_update", **bad)

# hyd_combine_lse and hyd_allreduce_sum
for bad in (dict(no_outs=True), dict(no_lses=True), dict(out=None), dict(n=0), dict(n=-1), dict(n=65), dict(rows=-1), dict(D=0), dict(dtype=3),
            dict(dtype=-1), dict(null_out=(1,)), dict(null_lse=(0,)), dict(n=64, null_lse=(63,)), dict(no_outs=True, n=0), dict(n=0, rows=-1),
            dict(rows=-1, dtype=3), dict(dtype=3, null_out=(0,))):
    r("hyd_combine_lse", **bad)
r("hyd_allreduce_sum", null=True)
for bad in (dict(no_blocks=True), dict(world=0), dict(world=9), dict(rank=-1), dict(rank=2), dict(dtype=3), dict(count=-1), dict(timeout_log2_polls=5),
            dict(timeout_log2_polls=32), dict(timeout_log2_polls=-1), dict(count=(1 << 19) + 1), dict(count=(1 << 18) + 1, dtype=2), dict(in_=None),
            dict(in_=MIS8), dict(out=None), dict(out=MIS8), dict(block={0: None}), dict(block={1: MIS8}), dict(world=9, rank=-1), dict(rank=2, dtype=3),
            dict(dtype=3, count=-1), dict(count=-1, timeout_log2_polls=5), dict(timeout_log2_polls=5, count=(1 << 19) + 1),
            dict(count=(1 << 19) + 1, in_=None), dict(in_=None, block={0: None}), dict(world=1, block={0: None})):
    r("hyd_allreduce_sum", **bad)


def _ptrs16(*names):
    """null, then aligned to the element but not to 16 bytes, for each pointer in turn"""
    return [{n: v} for n in names for v in (None, MIS8)]


# hyd_suffix_attn_causal_fwd (the builder's nq is 2: two rows per unit, which the causal kernel takes at every head count)
r("hyd_suffix_attn_causal_fwd", null=True)
chain("hyd_suffix_attn_causal_fwd",
      [dict(dtype=2), dict(D=96), dict(B=0), dict(Hq=8, Hkv=3), dict(softmax_scale=-0.5), dict(kv_dim=8), dict(kv_len=-1)]
      + _ptrs16("q", "out", "k", "v") + [{t.format(g): 4} for t in _STRIDES6 for g in ("batch", "tok", "head")]
      + [dict(nq=1), dict(nq=9), dict(kv_dim=96), dict(n_partials=-1), dict(n_partials=9), dict(kv_len=0), dict(n_partials=1),
         dict(kv_len=1 << 21, k_tok_stride=1024), dict(Hq=4 * 65535 + 1, Hkv=4 * 65535 + 1)])
for bad in (dict(kv_dim=136), dict(kv_dim=24), dict(softmax_scale=INF), dict(kv_len=0, k=None), dict(kv_len=0, kv_dim=96, n_partials=9),
            dict(kv_len=1 << 21, v_tok_stride=512), dict(Hq=65536, Hkv=1, nq=8), dict(Hq=65536, Hkv=65536, nq=3),
            dict(Hq=4 * 65535 + 1, Hkv=4 * 65535 + 1, nq=3), dict(Hq=65536, Hkv=65536, nq=3, kv_len=1 << 21, k_tok_stride=1024),
            dict(n_partials=1, **{"partials.0.out": PTR, "partials.0.lse": PTR, "partials.0.count": 0}),
            dict(n_partials=1, nq=3, Hq=65536, Hkv=65536)):
    r("hyd_suffix_attn_causal_fwd", **bad)
r("hyd_suffix_attn_causal_fwd", n_partials=8, **_MANY)
# (the causal tail's fp8 refusal is out of this entry point's reach -- it passes no hyd_kv_quant; the decode call reaches it)
for bad in (dict(), dict(nq=9), dict(**{"suffix.kv_dim": 96}), dict(phase=2)):
    r("hyd_decode_attn_fused_kvq", kq=dict(flags=1), causal_tail=1, Hq=32, **{"nq": 2, **bad})   # (8-row grouped-query units: native fp8 shapes)
r("hyd_decode_attn_fused", causal_tail=2)
r("hyd_decode_attn_fused", causal_tail=1)
r("hyd_decode_attn_fused", causal_tail=1, nq=2, **{"suffix.kv_dim": 96})
r("hyd_decode_attn_fused", causal_tail=1, nq=3, Hq=65536, Hkv=65536)

# hyd_rope_append_multi
_ROPE_MULTI_STRIDES = ("q_batch_stride", "k_batch_stride", "v_batch_stride", "q_tok_stride", "k_tok_stride", "v_tok_stride") + _ROPE_STRIDES[3:]
r("hyd_rope_append_multi", null=True)
chain("hyd_rope_append_multi",
      [dict(T=1), dict(T=9), dict(dtype=2), dict(D=96), dict(B=0), dict(Hq=8, Hkv=3)] + _ptrs16(*_ROPE_PTRS)
      + [[dict(position_ids=None), dict(seq_lens=None)], [dict(position_ids=PTR + 4), dict(shared_len=PTR + 4), dict(seq_lens=PTR + 2)]]
      + [{n: 4} for n in _ROPE_MULTI_STRIDES] + [dict(cs_stride=6), dict(cache_len=0), dict(max_pos=0)])
r("hyd_rope_append_multi", sin=MIS8, seq_lens=None)

# hyd_sample_tokens_constrained: without an automaton the penalised sampler's call; with one, every check of that call, then its own
r("hyd_sample_tokens_constrained", null=True)
r("hyd_sample_tokens_constrained", null=True, no_dfa=True)
r("hyd_sample_tokens_constrained", null=True, **{"c.allowed": None})
for bad in (dict(dtype=3), dict(top_p=0.0), dict(n_bias=1), dict(gen=PTR + 2, gen_len=PTR)):
    r("hyd_sample_tokens_constrained", no_dfa=True, **bad)
for bad in (dict(dtype=3), dict(rows=-1), dict(n=MAX_N + 1, row_stride=MAX_N + 1), dict(logits=None), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0),
            dict(min_p=1.5), dict(row_stride=63), dict(repetition_penalty=0.0), dict(frequency_penalty=INF), dict(n_context=10), dict(n_context=1),
            dict(n_context=2, **{"context.0.bits": PTR, "context.0.rows_per_group": 1, "context.1.bits": PTR}),
            dict(n_context=1, **{"context.0.bits": PTR + 2, "context.0.rows_per_group": 1}), dict(gen=PTR), dict(gen_stride=-1), dict(gen_stride=2049),
            dict(append_out=1), dict(n_bias=1025), dict(n_bias=1), dict(kept=PTR + 1), dict(gen=PTR, gen_len=PTR + 2)):   # (each is in _PENALTY_BAD)
    r("hyd_sample_tokens_constrained", **bad)
_DFA_CHAIN = [[{"c.allowed": None}, {"c.next": None}, {"c.state": None}], {"c.n_states": 0}, {"c.allowed_stride": 1}, {"c.next_stride": 63},
              [{"c.allowed": PTR + 2}, {"c.next": PTR + 2}, {"c.state": PTR + 2}]]
chain("hyd_sample_tokens_constrained", _DFA_CHAIN)
r("hyd_sample_tokens_constrained", n_bias=1, bias_ids=PTR, bias_values=PTR + 2, **{"c.allowed": None})   # the sampler's last check first
r("hyd_sample_tokens_constrained", n=65, row_stride=72, **{"c.allowed_stride": 2, "c.next_stride": 64})   # three words, 65 entries
r("hyd_sample_tokens_constrained", n=65, row_stride=72, **{"c.allowed_stride": 3, "c.next_stride": 64})
r("hyd_sample_tokens_constrained", **{"c.n_states": -1, "c.state": None})

# hyd_draft_lookup, with its per-segment loop (the first segment, the last of the two in use, the last there can be)
r("hyd_draft_lookup", null=True)


def _segment(i):
    g = f"segments.{i}."
    return [{g + "div": 0}, {g + "len": -1}, {g + "ids": None}, [{g + "ids": PTR + 4}, {g + "lens_i64": PTR + 4}, {g + "lens_i32": PTR + 2}]]


chain("hyd_draft_lookup",
      [dict(B=-1), dict(K=0), dict(K=8), dict(ngram_min=0), dict(ngram_max=0), dict(ngram_max=9), dict(n_segments=0), dict(n_segments=11),
       [dict(drafts=None), dict(n_proposed=None)], [dict(drafts=PTR + 4), dict(n_proposed=PTR + 2)], dict(drafts_stride=2)]
      + [s for i in (0, 1) for s in _segment(i)])
chain("hyd_draft_lookup", _segment(9), pairs=False, n_segments=10)
r("hyd_draft_lookup", **{"segments.0.ids": None, "segments.0.len": 0, "segments.1.len": -1})   # no ids and no length: taken
r("hyd_draft_lookup", **{"segments.2.div": 0, "segments.1.len": -1})                            # a segment past n_segments is not read
r("hyd_draft_lookup", K=4)                                                                      # drafts_stride 3 < K

# hyd_dfa_forced_tokens and hyd_draft_constrain
r("hyd_dfa_forced_tokens", null=True)
chain("hyd_dfa_forced_tokens", [[dict(n_states=0), dict(n=0)], dict(allowed_stride=1), [dict(allowed=None), dict(forced=None)],
                                [dict(allowed=PTR + 2), dict(forced=PTR + 2)]])
r("hyd_dfa_forced_tokens", n=65, allowed_stride=2)
r("hyd_dfa_forced_tokens", n_states=-1, allowed=None)
r("hyd_draft_constrain", null=True)
chain("hyd_draft_constrain",
      [dict(B=-1), [dict(K=0), dict(K=8)], [dict(n_states=0), dict(n=0)], dict(next_stride=63), dict(fed_stride=3),
       [{n: None} for n in ("state", "fed", "forced", "next", "step_state", "n_forced")],
       [dict(fed=PTR + 4)] + [{n: PTR + 2} for n in ("state", "n_proposed", "forced", "next", "step_state", "n_forced")]])
r("hyd_draft_constrain", K=4)   # fed_stride 4 < K + 1

# hyd_draft_accept and hyd_draft_accept_states (the same row-state block; the second adds the automaton's two arrays)
_ACCEPT_CHAIN = [dict(rows=-1), [dict(T=0), dict(T=9)], [dict(n_eos=-1), dict(n_eos=17)], [dict(max_new_tokens=0), dict(max_new_tokens=9)],
                 [{n: None} for n in ("fed", "sampled", "out", "length", "reason", "stop_index", "accepted", "live")],
                 [{n: None} for n in ("start_pos", "feed", "next_pos")],
                 [{n: PTR + 4} for n in ("fed", "sampled", "out", "start_pos", "shared_len", "feed", "next_pos")],
                 [{n: PTR + 2} for n in ("length", "reason", "stop_index", "accepted", "live", "logprobs", "out_logprobs")]]
r("hyd_draft_accept", null=True)
chain("hyd_draft_accept", _ACCEPT_CHAIN)
r("hyd_draft_accept_states", null=True)
r("hyd_draft_accept_states", null=True, step_state_after=None, state=None)
chain("hyd_draft_accept_states", _ACCEPT_CHAIN, pairs=False)   # (the order of these is pinned through hyd_draft_accept)
chain("hyd_draft_accept_states", [dict(out_logprobs=PTR + 2, live=PTR + 2), [dict(state=None), dict(step_state_after=None)],
                                  [dict(step_state_after=PTR + 2), dict(state=PTR + 2)]])
for bad in (dict(rows=-1), dict(live=None), dict(next_pos=PTR + 4), dict(out_logprobs=PTR + 2)):   # neither array: hyd_draft_accept's call
    r("hyd_draft_accept_states", step_state_after=None, state=None, **bad)

# hyd_kv_promote and hyd_kv_gather_paths: the unique segment they share, then the path's levels
_KV_SHAPE = [[dict(dst_dtype=2), dict(dst_dtype=3)], dict(src_dtype=2), dict(src_dtype=0), dict(n=0)]
_KV_SIZES = [dict(Hkv=0), [dict(B=0), dict(src_rows=0), dict(capacity=-1)], [dict(d_src=0), dict(d_src=12)], dict(d_dst=64), dict(d_dst=192),
             [dict(max_len=-1), dict(max_len=65)]]


def _kv_tail(cu):
    return ([dict(n=65536)] + _ptrs16("k_src", "v_src", "k_dst", "v_dst") + [[dict(rows=None), dict(lens=None), {cu: None}]]
            + [[{n: PTR + 2} for n in ("rows", "lens", cu, "k_scale", "v_scale")]]
            + [{t.format(g): 4} for t in _STRIDES6 for g in ("batch", "tok", "head")] + [[dict(k_head_stride=64), dict(v_head_stride=64)]])


r("hyd_kv_promote", null=True)
chain("hyd_kv_promote", _KV_SHAPE + _KV_SIZES + _kv_tail("cu") + [dict(src_rows=1 << 24)])
r("hyd_kv_promote", src_dtype=3, dst_dtype=3)
r("hyd_kv_promote", src_dtype=3, k_scale=PTR + 2)
r("hyd_kv_promote", d_src=96, d_dst=120)
r("hyd_kv_promote", max_len=64, src_rows=1 << 24, Hkv=1 << 21)           # max_len, not src_rows, bounds the sequence


def _level(j):
    return [{f"level_k.{j}": None}, {f"level_k.{j}": MIS8}, {f"level_v.{j}": None}, {f"level_v.{j}": MIS8},
            [{f"level_cu.{j}": None}, {f"level_cu.{j}": PTR + 2}], {f"level_div.{j}": 0}, [{f"level_s.{j}": 0}, {f"level_cap.{j}": -1}]]


r("hyd_kv_gather_paths", null=True)
chain("hyd_kv_gather_paths",
      _KV_SHAPE + [[dict(n_levels=-1), dict(n_levels=9)]] + _KV_SIZES + [[dict(max_path=-1), dict(max_path=257)]] + _kv_tail("cu_dst")
      + _level(0) + _level(1) + [dict(src_rows=1 << 24), dict(capacity=1 << 24)])
chain("hyd_kv_gather_paths", _level(7), pairs=False, n_levels=8)
r("hyd_kv_gather_paths", n_levels=8, src_rows=1 << 24, **{"level_cap.7": -1})
r("hyd_kv_gather_paths", **{"level_k.2": None, "level_cap.1": -1})       # a level past n_levels is not read
r("hyd_kv_gather_paths", n_levels=0, **{"level_k.0": None}, src_rows=1 << 24)
r("hyd_kv_gather_paths", max_path=64, src_rows=32, capacity=1 << 24, Hkv=1 << 21)    # max_path, not capacity, bounds the path
r("hyd_kv_gather_paths", capacity=0, src_rows=1 << 24)
r("hyd_kv_gather_paths", capacity=0, max_path=1)
noop("hyd_kv_gather_paths", capacity=0)
noop("hyd_kv_gather_paths", capacity=0, n_levels=0)

# hyd_kv_absmax and hyd_kv_scales_from_absmax
r("hyd_kv_absmax", null=True)
chain("hyd_kv_absmax",
      [dict(dtype=2), dict(Hkv=0), [dict(d=4), dict(d=264), dict(d=12)], [dict(n_outer=-1), dict(n_rows=-1)], dict(amax=None), dict(k=None, v=None),
       dict(k=MIS8), dict(v=MIS8), [dict(amax=PTR + 2), dict(row_lens=PTR + 2)]]
      + [{f"{t}_{g}_stride": 4} for t in "kv" for g in ("outer", "row", "head")]
      + [dict(n_rows=(1 << 30) + 1), dict(Hkv=(1 << 19) + 1, d=256), dict(n_rows=1 << 30, n_outer=64)])
r("hyd_kv_absmax", Hkv=1 << 19, d=256)                                   # 2^24 vectors per row: 65536 column blocks
r("hyd_kv_absmax", k=None, k_outer_stride=4, v_head_stride=4)            # an absent tensor's strides are not read
r("hyd_kv_absmax", v=None, v_outer_stride=4, k_head_stride=4)
r("hyd_kv_absmax", n_outer=0, n_rows=(1 << 30) + 1)                      # refused before the empty call returns
r("hyd_kv_absmax", n_rows=0, Hkv=(1 << 19) + 1, d=256)
for empty in (dict(n_outer=0), dict(n_rows=0), dict(n_outer=0, n_rows=0), dict(n_rows=0, k=None)):
    noop("hyd_kv_absmax", **empty)
r("hyd_kv_scales_from_absmax", null=True)
chain("hyd_kv_scales_from_absmax", [[{n: None} for n in ("amax", "k_scale", "v_scale")], [{n: PTR + 2} for n in ("amax", "k_scale", "v_scale")],
                                    dict(Hkv=0), [dict(c=0.0), dict(c=-1.0), dict(c=INF), dict(c=NAN)]])

# hyd_linear_w8 (with the workspace of a plan that splits K) and hyd_weight_widen
r("hyd_linear_w8", null=True)
chain("hyd_linear_w8",
      [dict(M=0), dict(dtype=2), [dict(N=0), dict(K=0)], dict(K=24)] + _ptrs16("w8") + [dict(scale=None), dict(scale=PTR + 2)] + _ptrs16("x", "y")
      + [dict(x_row_stride=4), dict(y_row_stride=4), [dict(x_row_stride=248), dict(y_row_stride=56)]])
r("hyd_linear_w8", M=1 << 30, N=1 << 30, K=16)
r("hyd_linear_w8", M=1 << 30, N=1 << 30, K=16, y_row_stride=56)
r("hyd_linear_w8", M=1 << 30, N=1 << 30, K=4096, workspace=None)
chain("hyd_linear_w8", [dict(y_row_stride=56), dict(workspace=None), dict(workspace_bytes=16), dict(workspace=MIS8)], **W8_SPLIT)
r("hyd_linear_w8", workspace=None, workspace_bytes=0, **W8_SPLIT)
r("hyd_weight_widen", null=True)
chain("hyd_weight_widen", [dict(dtype=2), [dict(N=0), dict(K=0)], dict(K=12)] + _ptrs16("w8") + [dict(scale=None), dict(scale=PTR + 2)]
      + _ptrs16("out") + [dict(out_row_stride=4), dict(out_row_stride=248)])

# hyd_narrow_kv_supported over the head dims and shapes of tests/test_narrow_head_dim_gpu.py: (kv_dim, Hkv, rows) of nine sequences, the
# 2052-sequence call, the few-unit and no-copy calls, the operator sizes (B, longest unique cache) at 80 / 96 / 192 on 8 heads
_PAD_D = {48: 64, 80: 128, 96: 128, 112: 128, 160: 256, 192: 256}
_NARROW = ([(9, 1, H, d, rows) for d, H, rows in ((96, 4, 40), (96, 8, 40), (96, 12, 40), (96, 20, 40), (96, 4, 16), (80, 8, 40), (112, 8, 40),
                                                 (48, 8, 40), (48, 16, 40), (160, 2, 40), (160, 6, 40), (192, 2, 40), (192, 6, 40))]
           + [(2052, 1, 4, 96, 32), (3, 1, 8, 96, 80), (3, 1, 8, 96, 1040), (64, 1, 32, 96, 512)]
           + [(B, 1, 8, d, S) for d in (80, 96, 192) for B, S in ((4, 4), (8, 6), (4, 5), (8, 8))])
for i, (B, nq, H, d, S) in enumerate(_NARROW):
    for dtype in ((0, 1) if i < 2 else (1,)):   # (the answer does not look at which of the two 16-bit dtypes it is)
        q("narrow_kv", dtype=dtype, B=B, nq=nq, Hq=H, Hkv=H, D=_PAD_D[d], kv_dim=d, kv_len=S)
for shape in (dict(kv_dim=0), dict(kv_dim=128), dict(kv_dim=8), dict(kv_dim=24), dict(kv_dim=136), dict(kv_dim=96, kv_len=0), dict(kv_dim=96, kv_len=-1),
              dict(kv_dim=0, kv_len=-1), dict(kv_dim=96, nq=2), dict(kv_dim=96, Hq=16), dict(kv_dim=96, Hq=6, Hkv=6), dict(kv_dim=96, dtype=2),
              dict(kv_dim=48, D=96), dict(kv_dim=96, B=0), dict(kv_dim=96, kv_len=1 << 21), dict(kv_dim=96, Hq=4 * 65535 + 4, Hkv=4 * 65535 + 4)):
    q("narrow_kv", **shape)
q("narrow_kv", null=True)
for M in (-1, 0, 1, 16, 17, 33, 65):         # (every row-tile class of the plan, and a non-positive size in each place)
    for N in (0, 30, 4096):
        for K in (0, 128, 4096, 16384):
            q("linear_w8_workspace", M=M, N=N, K=K)

# calls that return HYD_OK before any HIP call
noop("hyd_stop_update", rows=0)
noop("hyd_allreduce_sum", count=0)
noop("hyd_allreduce_sum", count=0, in_=None, out=None)
noop("hyd_decode_attn_fused", kv_len=0, phase=_lib.HYD_PHASE_UNIQUE)

# ---- the unique pass: which launch an accepted call reaches, on each side of every seam between two suffix kernels -----------------
_ONE = {"n_partials": 1, "partials.0.out": PTR, "partials.0.lse": PTR, "partials.0.count": 1}
_GQ = dict(Hq=32, Hkv=8)
_ALL, _UNIQUE, _PARTIAL, _MERGE = _lib.HYD_PHASE_ALL, _lib.HYD_PHASE_UNIQUE, _lib.HYD_PHASE_UNIQUE_PARTIAL, _lib.HYD_PHASE_MERGE
_GQA, _CAUSAL = _lib.HYD_KVQ_GQA, _lib.HYD_KVQ_CAUSAL
# 16-bit caches: one-row units, 2-row units, grouped-query units, the other head dims, narrow rows
_SHAPES16 = (dict(), dict(Hq=16, Hkv=8), _GQ, dict(D=64), dict(D=256), dict(D=256, **_GQ), dict(kv_dim=96), dict(kv_dim=96, Hq=4, Hkv=4))
# fp8 caches: (hyd_kv_quant, shape) -- one-row units with and without HYD_KVQ_GQA, grouped-query units with it
_SHAPES8 = ((dict(), dict()), (dict(flags=_GQA), dict()), (dict(flags=_GQA), _GQ), (dict(flags=_GQA | _CAUSAL), _GQ), (dict(), dict(D=64)),
            (dict(flags=_GQA), dict(D=256, **_GQ)))
# the causal tail: 2-row units, grouped-query units, the most query tokens, head dim 256
_SHAPES_CAUSAL = (dict(), _GQ, dict(nq=8), dict(nq=8, **_GQ), dict(D=256), dict(D=64))
_SAME_DTYPE = dict(kv_dtype=1)   # a hyd_kv_quant that names the q dtype: 16-bit caches through the _kvq entry points

for shape in _SHAPES16:
    launch("hyd_suffix_attn_fwd", **shape)
launch("hyd_suffix_attn_fwd", kv_len=0, **_ONE)       # merge-only
launch("hyd_suffix_attn_fwd", **_ONE)
launch("hyd_suffix_attn_fwd_kvq", kq=None)
launch("hyd_suffix_attn_fwd_kvq", kq=_SAME_DTYPE, **_GQ)
for kq, shape in _SHAPES8:
    launch("hyd_suffix_attn_fwd_kvq", kq=kq, **shape)
launch("hyd_suffix_attn_fwd_kvq", kq=dict(), **_ONE)
launch("hyd_suffix_attn_fwd_kvq", kq=dict(), kv_len=0, **_ONE)                 # no unique key to read
launch("hyd_suffix_attn_fwd_kvq", kq=dict(flags=_GQA), kv_len=0, **_GQ, **_ONE)
r("hyd_suffix_attn_fwd_kvq", kq=dict(), kv_len=0, Hq=4, Hkv=2, **_ONE)

for shape in _SHAPES_CAUSAL:
    launch("hyd_suffix_attn_causal_fwd", **shape)
    launch("hyd_suffix_attn_causal_fwd_kvq", kq=_SAME_DTYPE, **shape)
launch("hyd_suffix_attn_causal_fwd", kv_len=0, **_ONE)
launch("hyd_suffix_attn_causal_fwd_kvq", kq=None)
for flags in (_CAUSAL, _GQA | _CAUSAL):
    for shape in (dict(), _GQ, dict(nq=8, **_GQ), dict(D=256, **_GQ)):   # (the fp8 causal kernel also takes the 2-row units)
        launch("hyd_suffix_attn_causal_fwd_kvq", kq=dict(flags=flags), **shape)
launch("hyd_suffix_attn_causal_fwd_kvq", kq=dict(flags=_GQA | _CAUSAL), kv_len=0, **_ONE)   # no unique key: the 16-bit call
r("hyd_suffix_attn_causal_fwd_kvq", null=True)
# fp8 caches and no HYD_KVQ_CAUSAL: this entry point answers for the causal tail, on shapes the fp8 kernels take and on others alike ...
for kq in (dict(), dict(flags=_GQA)):
    for shape in (_GQ, dict(), dict(nq=9), dict(kv_len=0, **_ONE)):
        r("hyd_suffix_attn_causal_fwd_kvq", kq=kq, **shape)
r("hyd_suffix_attn_causal_fwd_kvq", kq=dict(flags=_GQA | _CAUSAL), kv_dim=96)
r("hyd_suffix_attn_causal_fwd_kvq", kq=dict(flags=_GQA | _CAUSAL), Hq=8, Hkv=1, D=256, kv_len=200)   # head dim 256 on few units
# ... the decode call for the fp8 shapes first (2-row units are not native without the causal kernel)
for kq in (dict(), dict(flags=_GQA)):
    r("hyd_decode_attn_fused_kvq", kq=kq, causal_tail=1, nq=2)
r("hyd_decode_attn_fused_kvq", kq=dict(), causal_tail=1, nq=2, **_GQ)
r("hyd_decode_attn_fused_kvq", kq=dict(flags=_GQA | _CAUSAL), causal_tail=1, nq=2, Hq=8, Hkv=1, D=256, kv_len=200)

# the decode call: every route with the unique pass as the first launch (HYD_PHASE_UNIQUE), then the other phases and forms
_ONE_LAUNCH = dict(B=8, Hq=32, Hkv=8, kv_len=32, levels=((1, 96),), single_launch_small=1)
_NOT_ONE_LAUNCH = (dict(kv_len=33), {"suffix.lse": PTR}, dict(levels=((1, 96, 512),)), dict(single_launch_small=0), dict(phase=_UNIQUE))
_DECODE_FORMS = (dict(phase=_PARTIAL), dict(phase=_MERGE), dict(phase=_ALL), dict(phase=_ALL, levels=((1, 4096),)),
                 dict(phase=_ALL, B=96, Hq=8, Hkv=2, levels=((1, 2048), (4, 96))), dict(kv_len=0), dict(kv_len=0, levels=((1, 4096),)),
                 dict(kv_len=0, phase=_UNIQUE, levels=((1, 64), (2, 64))), dict(kv_len=0, phase=_ALL, levels=((1, 64), (2, 64))),
                 dict(phase=_UNIQUE, levels=()), dict(phase=_ALL, levels=()))
for entry, kq in (("hyd_decode_attn_fused", {}), ("hyd_decode_attn_fused_kvq", dict(kq=_SAME_DTYPE))):
    for shape in _SHAPES16:
        launch(entry, phase=_UNIQUE, **kq, **{("suffix.kv_dim" if k == "kv_dim" else k): v for k, v in shape.items()})
    for form in _DECODE_FORMS:
        launch(entry, **kq, **form)
    launch(entry, **kq, **_ONE_LAUNCH)
    for near in _NOT_ONE_LAUNCH:
        launch(entry, **kq, **{**_ONE_LAUNCH, **near})
    launch(entry, **kq, **_ONE_LAUNCH, causal_tail=1, nq=2)   # (the walk over both segments has no per-row key limit)
    for shape in _SHAPES_CAUSAL:
        launch(entry, phase=_UNIQUE, causal_tail=1, **kq, **{"nq": 2, **shape})
    launch(entry, phase=_PARTIAL, causal_tail=1, nq=2, **kq)
    launch(entry, phase=_UNIQUE, causal_tail=1, nq=2, kv_len=0, levels=((1, 64), (2, 64)), **kq)
r("hyd_decode_attn_fused", **{**_ONE_LAUNCH, "levels": ((3, 96),)})
for kq, shape in _SHAPES8:
    launch("hyd_decode_attn_fused_kvq", kq=kq, phase=_UNIQUE, **shape)
for form in _DECODE_FORMS:
    launch("hyd_decode_attn_fused_kvq", kq=dict(), **{**form, "Hq": 8, "Hkv": 8})
    launch("hyd_decode_attn_fused_kvq", kq=dict(flags=_GQA), **{**_GQ, **form})
for near in _NOT_ONE_LAUNCH[:3] + _NOT_ONE_LAUNCH[4:]:
    launch("hyd_decode_attn_fused_kvq", kq=dict(flags=_GQA), **{**_ONE_LAUNCH, **near})
r("hyd_decode_attn_fused_kvq", kq=dict(), **_ONE_LAUNCH)                     # without HYD_KVQ_GQA these shapes are not native ...
launch("hyd_decode_attn_fused_kvq", kq=dict(), **{**_ONE_LAUNCH, "Hq": 8})   # ... and Hq == Hkv shapes ignore single_launch_small
for flags in (_CAUSAL, _GQA | _CAUSAL):
    for shape in (dict(), _GQ, dict(nq=8, **_GQ), dict(D=256, **_GQ)):
        launch("hyd_decode_attn_fused_kvq", kq=dict(flags=flags), phase=_UNIQUE, causal_tail=1, **{"nq": 2, **shape})
launch("hyd_decode_attn_fused_kvq", kq=dict(flags=_GQA | _CAUSAL), phase=_PARTIAL, causal_tail=1, nq=2, **_GQ)
launch("hyd_decode_attn_fused_kvq", kq=dict(flags=_GQA | _CAUSAL), causal_tail=1, nq=2, **_ONE_LAUNCH)
launch("hyd_decode_attn_fused_kvq", kq=dict(), phase=_UNIQUE, causal_tail=1, nq=2, kv_len=0, levels=((1, 64), (2, 64)))

# hyd_decode_kv_quant_supported under every hyd_kv_quant.flags: the causal tail's answer follows the launch's own rules
for ct in (0, 1, 2):
    for shape in (dict(), _GQ, dict(nq=2), dict(nq=2, **_GQ), dict(nq=8, **_GQ), dict(nq=9, **_GQ), dict(nq=2, D=256), dict(nq=2, D=64),
                  dict(nq=2, Hq=8, Hkv=1, D=256, kv_len=200), dict(nq=2, kv_len=0), dict(nq=2, kv_len=-1), {"nq": 2, "suffix.kv_dim": 96},
                  {"suffix.kv_dim": 96}, dict(nq=2, D=96), dict(nq=2, n_levels=9), dict(nq=2, kv_len=1 << 21), dict(nq=2, Hq=8, Hkv=3),
                  dict(nq=2, **_ONE_LAUNCH), _ONE_LAUNCH):
        q("decode_kvq", causal_tail=ct, **shape)


def _case_id(kind, entry, kw):
    return f"{kind}:{entry}:" + json.dumps(kw, sort_keys=True, default=str)


QUERY_CASES = [(_case_id("query", e, kw), e, kw) for e, kw in _Q]
REFUSAL_CASES = [(_case_id("refusal", e, kw), e, kw) for e, kw in _R]
NOOP_CASES = [(_case_id("noop", e, kw), e, kw) for e, kw in _N]
LAUNCH_CASES = [(_case_id("launch", e, kw), e, kw) for e, kw in _L]
_ids = [c[0] for c in QUERY_CASES + REFUSAL_CASES + NOOP_CASES + LAUNCH_CASES]
assert len(set(_ids)) == len(_ids), sorted(i for i in set(_ids) if _ids.count(i) > 1)


def run_case(case):
    """One case through ctypes -> a plain record (ints and strings only)."""
    cid, entry, kw = case
    lib = _lib.load()
    if cid.startswith("query:"):
        return QUERIES[entry](lib, kw)
    if cid.startswith("launch:"):
        assert not device_present(), "launch cases run where no device is present only: they would launch on made-up addresses"
        return _launch(REFUSALS[entry](lib, kw))
    rec = REFUSALS[entry](lib, kw)
    return {"rc": rec["rc"]} if cid.startswith("noop:") else rec  # (the error string is not cleared on success)


def load_fixture():
    return json.loads(FIXTURE.read_text())


def write():
    if device_present():
        raise SystemExit("record the table where no device is present: a launch case would run a kernel on made-up addresses")
    table = {}
    for case in QUERY_CASES:
        table[case[0]] = run_case(case)
    wrong = []
    for case in REFUSAL_CASES:
        rec = run_case(case)
        if rec["rc"] in (HYD_OK, HYD_ERR_LAUNCH):
            wrong.append(f"{case[0]}: the library answers {rec['rc']} ({rec['error']!r}): not a refusal")
        table[case[0]] = rec
    for case in NOOP_CASES:
        rec = run_case(case)
        if rec["rc"] != HYD_OK:
            wrong.append(f"{case[0]}: the library answers {rec['rc']} ({_err(_lib.load())!r}): not a call that returns HYD_OK")
        table[case[0]] = rec
    for case in LAUNCH_CASES:
        rec = run_case(case)
        if set(rec) != {"rc", "what"}:
            wrong.append(f"{case[0]}: the library answers {rec['rc']} ({rec['error']!r}): not a launch that fails for want of a device")
        table[case[0]] = rec
    if wrong:
        raise SystemExit("\n".join(wrong) + "\nnothing recorded")
    FIXTURE.write_text(json.dumps(table, indent=0, sort_keys=True) + "\n")
    print(f"{FIXTURE}: {len(QUERY_CASES)} queries, {len(REFUSAL_CASES)} refusals, {len(NOOP_CASES)} no-ops, {len(LAUNCH_CASES)} launches")


if __name__ == "__main__":
    if "--write" not in sys.argv:
        raise SystemExit(__doc__)
    write()
