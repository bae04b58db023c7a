"""The decode half of `HydragenLlamaForCausalLM.generate()` (llama.py): the argument checks, the first draw from the prefill logits
and the three step loops -- plain, device-side stop conditions (stopping.py), speculative drafts (speculative.py) -- as functions
that take the model.  The model keeps generate() itself, the prompt levels, the caches and the switches that tests and tools set
on it.  What the stop loop and the draft loop have in common is stated once: `_row_origin`, `_RunningPoll`, `_stopped_result`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor, nn

from . import flash as _flash
from . import layer_ops, sampling, scoring, speculative, stopping
from .tp import check_collectives


def per_row_sampling(temperature, top_k=None, top_p=None, min_p=None, penalties=None, seed=None) -> bool:
    """A sampling value is given per row, or the rows draw with seeds of their own (sampling.sample_route's per_row)."""
    return (seed is not None or any(sampling.is_per_row(v) for v in (temperature, top_k, top_p, min_p))
            or (penalties is not None and penalties.per_row()))


def draw_tokens(route: sampling.SampleRoute, logits, temperature, num_samples=1, top_p=None, top_k=None, min_p=None,
                return_logprobs=False, penalties=None, constraint=None, seed=None, offset=0, drafts=None):
    """Run one draw along `route` (sampling.sample_route's table): (tokens [B, num_samples], their fp32 log-probs
    [B, num_samples] or, for a draw in torch that needs none, None).  The other arguments are sample_from_logits'.
    drafts = fed int64 [B, T]: the rows are the B * T logits rows of a speculative step; a PENALIZED route then draws through
    hyd_sample_tokens_penalized_drafts, which counts the drafts in front of each position (the draft loop takes no other
    penalised route)."""
    x, n = logits, num_samples
    if drafts is not None and penalties is not None and penalties.active():
        if route.draw != sampling.PENALIZED or route.torch_penalties or per_row_sampling(temperature, top_k, top_p, min_p, penalties, seed):
            raise NotImplementedError("penalties in a speculative step are drawn by hyd_sample_tokens_penalized_drafts alone: scalar "
                                      "values, no constraint, fused_penalties on")
        tok, lp = layer_ops.sample_tokens(x if x.stride(-1) == 1 else x.contiguous(), temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                                          return_logprobs=True, penalties=penalties, drafts=drafts)
        return tok.reshape(-1, 1), lp.reshape(-1, 1)
    if per_row_sampling(temperature, top_k, top_p, min_p, penalties, seed):
        # the per_row routes: one launch over one row per sample (the values and seeds are the batch rows'), rows a kernel cannot
        # take as they are made contiguous; CPU rows: the definition in torch (layer_ops.sample_tokens routes both)
        x = x.repeat_interleave(n, 0) if n > 1 else x if x.stride(-1) == 1 else x.contiguous()
        tok, lp = layer_ops.sample_tokens(
            x, temperature, None if seed is None else (0, offset), top_k=top_k, top_p=top_p, min_p=min_p, return_logprobs=True,
            penalties=penalties, constraint=(*constraint, True) if constraint is not None else None, seed=seed)
        return tok.reshape(-1, num_samples), lp.reshape(-1, num_samples)
    if route.torch_penalties:  # the definition, float64 through [B, V] tables
        x = penalties.apply(x, n).float()
    if route.torch_mask:
        x, n = sampling.constrain_logits(x.repeat_interleave(n, 0), *constraint), 1
    if route.draw in (sampling.PLAIN, sampling.TORCH):
        src = x
        # (a top_p of 1.0 is no cut to the kernels, but in torch it still passes through apply_top_p, as in the reference)
        if route.torch_cuts or top_p is not None:
            x = sampling.filter_logits(x, top_k, top_p, min_p) if top_k or min_p else sampling.apply_top_p(x, top_p)
        if route.draw == sampling.PLAIN:
            # argmax(logits / T + Gumbel noise) draws exactly from softmax(logits / T) -- what the softmax + torch.multinomial
            # chain below draws, in one pass over the logits instead of ~12 launches over [B, vocab]
            tok = layer_ops.sample_tokens(x, temperature)
        elif temperature == 0:
            assert x.ndim == 2
            tok = x.argmax(dim=-1, keepdim=True).repeat_interleave(n, dim=-1)
        else:
            tok = torch.multinomial(nn.functional.softmax(x / temperature, dim=-1), num_samples=n, replacement=True)
        lp = torch.log_softmax(src.float(), dim=-1).gather(-1, tok) if return_logprobs or route.torch_mask else None
    else:
        # one launch (CPU rows: its definition in torch): mask, penalties, cuts, draw, log-prob, the append and the state update
        tok, lp = layer_ops.sample_tokens(
            x, temperature, top_k=top_k, top_p=top_p, min_p=min_p, return_logprobs=True,
            penalties=None if route.draw == sampling.FILTERED else penalties,
            constraint=(*constraint, True) if route.draw == sampling.CONSTRAINED else None)
    if route.torch_mask:  # a row drew something iff its log-prob is a number
        dfa, state = constraint
        state.copy_(sampling.advance_state(dfa, state, tok, ~torch.isnan(lp.reshape(-1))))
    if route.torch_penalties and penalties.append and num_samples == 1:
        penalties.push(tok)
    return tok.reshape(-1, num_samples), None if lp is None else lp.reshape(-1, num_samples)


@dataclass
class _Draft:
    """generate()'s speculative-decoding arguments: _check_draft sets the fields down to `only_forced`, generate() the rest."""
    k: int                                     # drafts fed per row and step (draft_tokens)
    given: Optional[Tensor]                    # the caller's drafts [batch, max_new_tokens], or None: proposed per step
    ngram: tuple                               # (min, max) n-gram lengths of the prompt lookup
    only_forced: bool                          # draft="constraint": propose the tokens the automaton forces and nothing else
    segments: Optional[list] = None            # the lookup's context: the prompt levels given to this call, outermost first
    stats: bool = False                        # return a speculative.DraftStats as the last value


@dataclass
class _DecodeCall:
    """What the decode half of one generate() call shares between decode and its three step loops.  check_arguments sets the
    fields down to `draft`, before any launch; decode sets `state`, `route`, `pen`, `raw` and `graphed` before the steps; decode,
    _step and keep() fill the lists."""
    sample: dict                               # sample_from_logits' arguments but the logits and num_samples
    fan: int
    max_new_tokens: int
    top_n: int = 0
    logits: Optional[list] = None              # kept per step, if they are returned: [B, V] each
    logprobs: Optional[list] = None            # [B, 1] each
    top: Optional[tuple] = None                # (ids, log-probs) lists of [B, 1, top_n] each
    eos: Optional[int] = None                  # an int eos_token_id: the plain loop's own exit
    overrides: Optional[Tensor] = None         # token_overrides: what is fed instead of the draws
    stop: Optional[stopping.StopSpec] = None   # stop conditions decided on the device: the stop loop or the draft loop
    finish: bool = False                       # return a stopping.Finish
    penalty_args: Optional[tuple] = None       # (repetition, presence, frequency, logit_bias, one of the first three is on), if any is on
    constraint_args: Optional[tuple] = None    # (dfa, the given start states or None, return the final states)
    draft: Optional[_Draft] = None             # speculative decoding
    rows: Optional[dict] = None                # per-row arguments as the caller gave them, host-checked: sampling values, "seed", "limits"
    max_len: Optional[Tensor] = None           # per-row max_new_tokens: int32 [batch] on the model's device (the stop loop)
    seeded: bool = False                       # seed=: the draw of output position t uses offset t and the rows' seeds
    state: Optional[Tensor] = None             # the automaton states, if they are returned
    route: Optional[sampling.SampleRoute] = None  # of the steps' draws (the first draw, which may fan out, has its own)
    pen: Optional[layer_ops.Penalties] = None  # the penalties, if they keep a list of generated tokens (a bias alone does not)
    raw: bool = False                          # the steps' logits stay in the lm_head's dtype
    graphed: bool = False

    def keep(self, logits, tok, lp):
        """Record a step's returned log-probs and alternatives."""
        if self.logprobs is not None:
            self.logprobs.append(lp)
        if self.top is not None:  # the same logits the sampler read; the sampled token's log-prob stays the sampler's
            for kept, t in zip(self.top, layer_ops.token_logprobs(logits, tok[:, 0], self.top_n)[2:]):
                kept.append(t[:, None])

    def result(self, tokens, past=None, finish=None):
        """generate()'s (tokens[, logits][, logprobs][, top_ids, top_logprobs][, finish][, state]), or the tokens alone.
        past [B, width] bool (the stop path): what was kept is trimmed to the tokens' width and blanked at or past a row's
        length."""
        width = None if past is None else tokens.shape[1]
        ret = (tokens,) if self.logits is None else (tokens, self.logits[:width])
        for kept, blank in zip((self.logprobs,) + (self.top or ()), (0.0, -1, float("-inf"))):
            if kept is not None:
                t = torch.cat(kept, dim=1)
                ret += (t if past is None else t[:, :width].masked_fill(past if t.ndim == 2 else past[:, :, None], blank),)
        ret += tuple(x for x in (finish, self.state) if x is not None)
        return ret if len(ret) > 1 else tokens


def check_arguments(model, *, input_ids, starting_logits, num_return_sequences, max_new_tokens, temperature, top_p, top_k, min_p, eos_token_id,
                    return_logits, disable_hydragen, disable_attention, disable_hierarchy, token_overrides, return_logprobs,
                    top_logprobs, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, stop, pad_token_id,
                    include_stop, return_finish, constraint, constraint_state, return_constraint_state, draft_tokens, draft,
                    ngram, return_draft_stats, seed=None) -> _DecodeCall:
    """generate()'s arguments but the prompt levels, checked on the host before any launch -> the call's _DecodeCall."""
    vocab, on_gpu = model.vocab_size, model.lm_head.weight.is_cuda
    # per-row arguments: lists / 1-d tensors become host lists here (checked element by element); decode() repeats them per
    # sample and uploads them once
    rows = {}
    given = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, repetition_penalty=repetition_penalty,
                 presence_penalty=presence_penalty, frequency_penalty=frequency_penalty)
    for name, v in given.items():
        if sampling.is_per_row(v):
            vals = sampling.row_values(v.cpu() if isinstance(v, Tensor) else v, None, name)
            if not vals:
                raise ValueError(f"{name}: an empty list of per-row values")
            if all(x == vals[0] for x in vals) and not (name == "temperature" and vals[0] is None):
                given[name] = vals[0]  # every row equal: the scalar, and exactly the scalar call's launches
            else:
                rows[name] = vals
    if seed is not None:
        rows["seed"] = [int(v) for v in sampling.row_values(seed.cpu() if isinstance(seed, Tensor) else seed, None, "seed")]
    if sampling.is_per_row(max_new_tokens):
        limits = sampling.row_values(max_new_tokens.cpu() if isinstance(max_new_tokens, Tensor) else max_new_tokens, None, "max_new_tokens")
        if not limits or any(isinstance(v, bool) or int(v) != v or v < 1 for v in limits):
            raise ValueError(f"max_new_tokens per row: integers >= 1, got {limits}")
        rows["limits"] = [int(v) for v in limits]
        max_new_tokens = max(rows["limits"])
    if rows and (draft_tokens or token_overrides is not None):
        raise NotImplementedError("per-row sampling values, seed= and a per-row max_new_tokens cannot be combined with draft_tokens or "
                                  "token_overrides: the draft loop draws several positions per step with one offset, and teacher "
                                  f"forcing draws nothing (per row here: {', '.join(rows)})")
    if "temperature" in rows:
        if any(t is None or not t >= 0 for t in rows["temperature"]):
            raise ValueError(f"temperature must be non-negative for every row, {rows['temperature']} is invalid")
    temperature, top_k, top_p, min_p, repetition_penalty, presence_penalty, frequency_penalty = (
        rows.get(name, v) for name, v in dict(given, temperature=0.0 if "temperature" in rows else given["temperature"]).items())
    penalties = (repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
    if constraint is None and (constraint_state is not None or return_constraint_state):
        raise ValueError("constraint_state / return_constraint_state need constraint=")
    if constraint is not None:
        if token_overrides is not None:
            raise ValueError("constraint cannot be combined with token_overrides (teacher forcing draws nothing to constrain)")
        sampling.check_constraint(constraint, vocab)
        if constraint.next.device != model.lm_head.weight.device:
            constraint = constraint.to(model.lm_head.weight.device)
    spec_draft = None
    if draft_tokens:
        spec_draft = _check_draft(
            model, draft_tokens, draft, ngram, max_new_tokens,
            {"repetition / presence / frequency penalties or logit_bias together with constraint=":
                 sampling.penalties_active(*penalties) and constraint is not None,
             "stop together with constraint=": stop is not None and constraint is not None,
             "token_overrides": token_overrides is not None,
             "top_logprobs": bool(top_logprobs), "return_logits": return_logits, "disable_hydragen": disable_hydragen,
             "disable_attention": disable_attention, "disable_hierarchy": disable_hierarchy},
            n_given=0 if input_ids is None else 1 if isinstance(input_ids, Tensor) else len(input_ids),
            constrained=constraint is not None,
            gpu_only={"repetition / presence / frequency penalties or logit_bias": sampling.penalties_active(*penalties),
                      "stop": stop is not None})
        spec_draft.stats = return_draft_stats
        if eos_token_id is not None and not isinstance(eos_token_id, (list, tuple, Tensor)):
            eos_token_id = [eos_token_id]
    elif return_draft_stats:
        raise ValueError("return_draft_stats needs draft_tokens")
    stop_spec = None
    if isinstance(eos_token_id, (list, tuple)) or stop is not None or pad_token_id is not None or return_finish or spec_draft or "limits" in rows:
        if token_overrides is not None:
            raise ValueError("token_overrides (teacher forcing) has nothing to stop: it cannot be combined with a list of EOS ids, "
                             "stop, pad_token_id or return_finish")
        if "limits" in rows and eos_token_id is not None and not isinstance(eos_token_id, (list, tuple, Tensor)):
            eos_token_id = [eos_token_id]  # (the device-side stop path takes lists)
        stop_spec = stopping.check_stop(eos_token_id, stop, pad_token_id, include_stop, vocab)
        if not on_gpu and "limits" not in rows:  # (per-row limits on a CPU model: the stop loop on the torch definition)
            raise ValueError("stop conditions are decided by a HIP kernel (hyd_stop_update): the model must be on the GPU; "
                             "stopping.truncate_reference applies the same rules to CPU tokens")
        eos_token_id = None
    if (input_ids is None) == (starting_logits is None):
        raise ValueError("pass exactly one of input_ids and starting_logits")
    if "temperature" not in rows and temperature < 0:
        raise ValueError(f"temperature must be non-negative, {temperature} is invalid")
    sampling.check_filters(top_k, top_p, min_p)
    top_n = scoring.check_top_n(top_logprobs)
    if top_n and not return_logprobs:
        raise ValueError("top_logprobs needs return_logprobs=True")
    sampling.check_penalties(*penalties, vocab)
    # only the three penalties read the generated tokens; a bias / ban list alone needs no list and has no length limit
    counted = sampling.penalties_active(*penalties[:3])
    if counted and max_new_tokens > sampling.GEN_MAX:
        raise ValueError(f"repetition / presence / frequency penalties count up to {sampling.GEN_MAX} generated tokens per "
                         f"sequence, max_new_tokens is {max_new_tokens}")
    return _DecodeCall(
        sample=dict(temperature=temperature, top_p=top_p, top_k=top_k, min_p=min_p, return_logprobs=return_logprobs),
        fan=num_return_sequences, max_new_tokens=max_new_tokens, top_n=top_n, logits=[] if return_logits else None, logprobs=[] if return_logprobs else None,
        top=([], []) if top_n else None, eos=eos_token_id, overrides=token_overrides, stop=stop_spec, finish=return_finish,
        penalty_args=(*penalties, counted) if sampling.penalties_active(*penalties) else None,
        constraint_args=None if constraint is None else (constraint, constraint_state, return_constraint_state), draft=spec_draft,
        rows=rows or None, seeded=seed is not None)


def _check_draft(model, draft_tokens, draft, ngram, max_new_tokens, refused: dict, n_given: int = 0, constrained: bool = False,
                 gpu_only: Optional[dict] = None) -> _Draft:
    """generate()'s draft arguments, checked before any launch.  n_given: the prompt levels given to the call (each is a
    segment of the lookup's table, beside the generated tokens); constrained: the call has a constraint= (what
    draft="constraint" proposes from); gpu_only: what a speculative step carries in HIP kernels alone (stop sequences in
    hyd_draft_accept_stop, penalties in hyd_sample_tokens_penalized_drafts)."""
    k = speculative.check_draft_tokens(draft_tokens)
    for what, on in refused.items():
        if on:
            raise NotImplementedError(f"draft_tokens cannot be combined with {what}: a speculative step draws and accepts "
                                      "several tokens per row in launches that do not carry it")
    for what, on in (gpu_only or {}).items():
        if on and not model.lm_head.weight.is_cuda:
            raise NotImplementedError(f"draft_tokens with {what} is not implemented for a model on the CPU: a speculative step judges "
                                      "and counts the several tokens it emits per row in HIP kernels (speculative.accept_stop_reference "
                                      "/ sampling.draft_row_lists_reference state the rules in torch)")
    given = None
    only_forced = isinstance(draft, str) and draft == "constraint"
    if isinstance(draft, Tensor):
        if draft.ndim != 2 or draft.shape[1] != max_new_tokens or draft.is_floating_point() or draft.dtype == torch.bool:
            raise ValueError(f"draft: an int tensor [batch, max_new_tokens = {max_new_tokens}], got {tuple(draft.shape)} {draft.dtype}")
        given = draft
    elif only_forced:
        if not constrained:
            raise ValueError("draft='constraint' proposes the tokens the automaton forces: it needs constraint=")
    elif not isinstance(draft, str) or draft != "prompt_lookup":
        raise ValueError(f"draft = {draft!r}: 'prompt_lookup', 'constraint' or an int tensor [batch, max_new_tokens]")
    elif n_given + 1 > speculative.MAX_SEGMENTS:
        raise ValueError(f"draft='prompt_lookup' searches {n_given} given levels and the generated tokens: at most "
                         f"{speculative.MAX_SEGMENTS} segments (hyd_draft_lookup)")
    ngram = speculative.check_ngram(ngram)
    attn = model.model.layers[0].self_attn
    if attn.kv_cache.narrow or attn.head_dim not in (64, 128, 256):
        raise NotImplementedError("draft_tokens with a head dim other than 64 / 128 / 256: the multi-token preamble and the causal-tail "
                                  "suffix pass take caches of those head dims only")
    if attn.kv_cache.fp8 and not model.lm_head.weight.is_cuda:
        raise NotImplementedError("draft_tokens with fp8 unique caches is not implemented for a model on the CPU: the multi-token "
                                  "preamble quantizes and the causal-tail suffix pass widens the cache rows in HIP kernels")
    if constrained and not model.lm_head.weight.is_cuda:
        raise NotImplementedError("draft_tokens with constraint= is not implemented for a model on the CPU: the drafts are walked "
                                  "through the automaton and accepted with their states by HIP kernels (speculative."
                                  "constrain_drafts_reference / accept_states_reference state the rules in torch)")
    if not model.lm_head.weight.is_cuda:
        raise ValueError("draft_tokens: drafts are proposed, verified and accepted by HIP kernels, the model must be on the GPU "
                         "(speculative.prompt_lookup_reference / accept_reference state the rules in torch)")
    return _Draft(k=k, given=given, ngram=ngram, only_forced=only_forced)


def _penalties(model, batch, unique, fan, max_new_tokens, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, counted):
    """The call's layer_ops.Penalties: the used shared levels' bitmaps (one row per shared sequence, read by its
    batch / sb rows: the same token set whether the keys sit in shared or -- disable_hydragen -- unique caches), the unique
    prompts' bitmap shared by the samples of a leaf, and -- `counted`: a penalty that reads them is on -- an empty
    [batch, max_new_tokens] list of generated tokens."""
    if len(model.shared_bitmaps) != model.get_num_used_shared_caches():
        raise RuntimeError(f"{model.get_num_used_shared_caches()} shared levels in use but {len(model.shared_bitmaps)} recorded token "
                           "sets: a level was added or dropped behind append_shared / truncate_shared_caches")
    context = [(bits, batch // bits.shape[0]) for bits in model.shared_bitmaps]
    if unique is not None:
        context.append((layer_ops.token_bitmap(unique[0].long(), unique[1].to(unique[0].device), model.vocab_size), fan))
    if len(context) > sampling.MAX_CONTEXT:
        raise ValueError(f"{len(context)} prompt levels: penalties take up to {sampling.MAX_CONTEXT}")
    dev = model.lm_head.weight.device
    return layer_ops.Penalties(
        repetition_penalty, presence_penalty, frequency_penalty, sampling.normalize_logit_bias(logit_bias, dev), context,
        gen=torch.zeros((batch, max_new_tokens), dtype=torch.int32, device=dev) if counted else None,
        gen_len=torch.zeros((batch,), dtype=torch.int32, device=dev) if counted else None)


def _upload_rows(model, call: _DecodeCall, leaf_batch, fan):
    """The call's per-row arguments, [leaf batch] (repeated per sample) or [batch] -- constraint_state's rule --, uploaded once:
    they live on the model's device for the whole call (fp32 / int32 arrays as hyd_sample_tokens_rows reads them, the seeds as
    int64 bit patterns, the limits as int32)."""
    dev, batch = model.lm_head.weight.device, leaf_batch * fan
    dtypes = {name: (dtype, off) for name, dtype, off in layer_ops.ROW_FIELDS}
    dtypes.update(seed=(torch.int64, 0), limits=(torch.int32, 1))
    for name, vals in call.rows.items():
        if len(vals) == 1:
            vals = vals * batch
        if len(vals) not in (leaf_batch, batch):
            raise ValueError(f"{'max_new_tokens' if name == 'limits' else name} holds {len(vals)} per-row values: {leaf_batch} "
                             f"(one per prompt, repeated for num_return_sequences) or {batch}")
        if len(vals) != batch:
            vals = [v for v in vals for _ in range(fan)]
        arr = layer_ops.row_array(vals, batch, dev, *dtypes[name], name)
        if name == "limits":
            call.max_len = arr
        elif name in ("repetition_penalty", "presence_penalty", "frequency_penalty"):
            if call.penalty_args is None:  # (a list of values that are all off)
                continue
            slot = dict(repetition_penalty=0, presence_penalty=1, frequency_penalty=2)[name]
            call.penalty_args = tuple(arr if i == slot else v for i, v in enumerate(call.penalty_args))
        else:
            call.sample[name] = arr


def _constraint_state(model, constraint_state, leaf_batch, fan):
    """The call's automaton states, int32 [batch] on the device: the given start states ([leaf batch], repeated per sample, or
    [batch]), default 0."""
    dev = model.lm_head.weight.device
    batch = leaf_batch * fan
    if constraint_state is None:
        return torch.zeros((batch,), dtype=torch.int32, device=dev)
    st = torch.as_tensor(constraint_state)
    if st.ndim != 1 or st.dtype.is_floating_point or st.dtype == torch.bool or st.shape[0] not in (leaf_batch, batch):
        raise ValueError(f"constraint_state must hold {leaf_batch} or {batch} integer states, got {tuple(st.shape)} {st.dtype}")
    st = st.to(device=dev, dtype=torch.int32)
    return (st.repeat_interleave(fan, 0) if st.shape[0] != batch else st.clone()).contiguous()


def decode(model, call: _DecodeCall, prefill_logits, shared, unique):
    """Everything of a generate() call behind its prefills: prefill_logits [leaf batch, V] of the innermost level, shared / unique
    the prompt levels given to the call (model._prompt_levels).  -> generate()'s return value."""
    from .llama import AttentionMode

    samp, fan = call.sample, call.fan
    leaf_batch = prefill_logits.shape[0]
    if call.rows is not None:
        _upload_rows(model, call, leaf_batch, fan)
    if call.penalty_args is not None:
        samp["penalties"] = _penalties(model, leaf_batch * fan, unique, fan, call.max_new_tokens, *call.penalty_args)
    if call.constraint_args is not None:
        dfa, given, returned = call.constraint_args
        state = _constraint_state(model, given, leaf_batch, fan)
        samp["constraint"] = (dfa, state)
        call.state = state if returned else None
    if call.draft is not None:
        # the logical context of the lookup: the levels given to THIS call, outermost first, then the rows' own prompts
        # (moved to the model's device: hyd_draft_lookup reads them there every step, whatever device the caller's ids are on)
        dev = model.lm_head.weight.device
        call.draft.segments = [speculative.Segment(ids.to(dev).long(), None if lens is None else lens.to(dev).long())
                               for ids, lens in shared + ([unique] if unique is not None else [])]
    overrides = call.overrides
    pen = samp.get("penalties")
    if pen is not None and pen.gen is not None:  # (a bias alone keeps no list of generated tokens)
        # the list of generated tokens follows what is FED: the sampler appends its own draws unless overrides replace them
        # (or the first token fans out: one row of logits, `fan` rows of tokens)
        # (a speculative step draws several positions per row and keeps some of them: there the sampler never appends, the
        # accept writes the list -- the first token included, which enters through an accept of one token)
        call.pen = pen
        pen.append = overrides is None and fan == 1 and call.draft is None
    first = model.sample_from_logits(prefill_logits, num_samples=fan, **samp)
    if call.logprobs is not None:
        first, lp = first
        call.logprobs.append(lp.reshape(-1, 1))
    if call.top is not None:
        # the alternatives do not depend on the drawn token: once over the leaf_batch prefill rows, repeated per sample
        rows = prefill_logits if prefill_logits.stride(-1) == 1 else prefill_logits.contiguous()
        none = torch.full((rows.shape[0],), -1, dtype=torch.int64, device=rows.device)
        for kept, t in zip(call.top, layer_ops.token_logprobs(rows, none, call.top_n)[2:]):
            kept.append(t.repeat_interleave(fan, 0)[:, None])
    first = first.reshape(-1, 1)
    if call.logits is not None:
        call.logits.append(prefill_logits.repeat_interleave(fan, 0))
    start = model.get_shared_cache_len(first.shape[0])[:, None]
    if unique is not None:
        start = start + unique[1].long().repeat_interleave(fan, 0)[:, None]
    model._check_room(start, call.max_new_tokens, extra=call.draft.k if call.draft else 0)
    feed = first if overrides is None else overrides[:, 0:1]
    if call.pen is not None and not pen.append and call.draft is None:
        pen.push(feed)
        pen.append = overrides is None
    model.set_mode(AttentionMode.DECODE)
    # calibrated fp8 scales: a call without unique prompts first writes the unique cache in its first decode step (the fused
    # preamble does not pass through update_per_completion_kvs): the scales are written here, once, outside any captured graph
    model._scale_windows("close_scale_window")
    # 16-bit logits straight into the sampler unless the caller wants them (fp32, as the reference returns them) or
    # the cuts run in torch
    call.graphed = model.graphed_model is not None
    call.route = model.sample_route(prefill_logits.is_cuda, True, **samp)  # (a step's logits are rows of the lm_head's output)
    call.raw = call.logits is None and (model.fused_sampling_filters or not sampling.filters_active(
        samp["top_k"], samp["top_p"], samp["min_p"]))
    # Ragged unique prompts: hand the longest sequences to the chip first.  Every length grows by one per step, so the order of
    # this generation's first step is the order of all of them (C2 heads, lengths 1..128 at random: suffix pass 184 -> 169 us).
    order = None
    if unique is not None:
        lens0 = unique[1].repeat_interleave(fan, 0)
        if model.schedule_longest_first and lens0.numel() > 1 and bool((lens0 != lens0[0]).any()):
            order = model.seq_order_buf[: lens0.numel()]
            order.copy_(_flash.longest_first(lens0))
    with _flash.seq_order(order, check=False):
        if call.draft is not None:
            return _decode_steps_draft(model, call, first, start)
        if call.stop is not None:
            return _decode_steps_stop(model, call, first, start)
        return _decode_steps(model, call, first, feed, start)


def _step(model, call: _DecodeCall, input_ids, position_ids, t=0):
    """One decode step along the call's route: (logits [B, V], tokens [B, 1], log-probs or None).  t: the output position the
    step draws (the offset of a seeded draw)."""
    logits = model(input_ids=input_ids, position_ids=position_ids, use_graph=call.graphed, raw_logits=call.raw)[:, -1]
    if call.logits is not None:
        call.logits.append(logits)
    return (logits,) + draw_tokens(call.route, logits, **call.sample, **(dict(offset=t) if call.seeded else {}))


def _decode_steps(model, call: _DecodeCall, first, feed, start):
    eos, overrides = call.eos, call.overrides
    done = (first == eos) if eos is not None else None
    tokens = [first]
    for step in range(call.max_new_tokens - 1):
        logits, nxt, lp = _step(model, call, feed, start + step, step + 1)
        if done is not None:
            done = done | (nxt == eos)
            if bool(done.all()):
                break
        tokens.append(nxt)
        call.keep(logits, nxt, lp)
        feed = nxt if overrides is None else overrides[:, step + 1 : step + 2]
        if call.pen is not None and not call.pen.append and feed.shape[1]:
            call.pen.push(feed)
    check_collectives()  # no-op without the direct xGMI all-reduce; raises if a rank ever gave up on a peer
    return call.result(torch.cat(tokens, dim=-1))


# ---- what the stop loop and the draft loop share ------------------------------------------------------------------------------
def _row_origin(model, start):
    """(retire, shared_len [B] or None, start_pos [B]) of a loop whose state kernel hands back the rows' next positions.  retire:
    finished rows leave the unique K/V stream -- model.stop_retire, None meaning whenever every layer uses the fused decode
    preamble: a retired row is fed position shared_len - 1, cache index -1, which the fused preamble skips and the torch scatter
    of update_per_completion_kvs would not."""
    fused = all(l.self_attn.use_fused_decode for l in model.model.layers)
    retire = fused if model.stop_retire is None else bool(model.stop_retire)
    if retire and not fused:
        raise ValueError("stop_retire needs the fused decode preamble (use_fused_decode) in every layer")
    shared_len = None if model.model.get_disable_hydragen() else model.get_shared_cache_len(start.shape[0]).contiguous()
    return retire, shared_len, start.reshape(-1).long().contiguous()


class _RunningPoll:
    """The count of running rows, without draining the launch queue: the copy started after step c is waited for after step
    c + 1 has been enqueued, so the device always has a step of work queued behind what the host waits for, and an exit is
    noticed at most stop_poll_steps steps late.  (Only looking at events that happen to be complete would let the host run ahead
    by the whole launch queue before it notices anything.)"""

    def __init__(self, model, max_new_tokens):
        self.period, self.max_new_tokens = max(1, int(model.stop_poll_steps)), max_new_tokens
        # (page-locked once per model, not once per call: every slot is written by its copy before it is read, and no copy
        # is left in flight when a generation returns)
        need = max_new_tokens // self.period + 1
        self.polled = getattr(model, "_stop_polled", None)
        if self.polled is None or self.polled.numel() < need:
            self.polled = model._stop_polled = torch.empty((max(need, 512),), dtype=torch.int32).pin_memory()
        self.pending = None  # (slot, event) of the copy started at the previous step

    def none_running(self) -> bool:
        """Wait for the copy started at the previous step, if one was: whether it read 0 running rows."""
        if self.pending is None:
            return False
        slot, ev = self.pending
        ev.synchronize()
        self.pending = None
        return int(self.polled[slot]) == 0

    def start(self, live, count, slot):
        """After state-kernel call number slot + 1 has written live[slot]: start a non-blocking copy of it if the caller's
        `count` is a multiple of the period and a step is still to come.  (The loops count from different phases: the stop
        loop passes the calls made, the draft loop the forwards run -- one less.)"""
        if count % self.period == 0 and slot + 1 < self.max_new_tokens:
            at = count // self.period
            self.polled[at : at + 1].copy_(live[slot : slot + 1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.pending = (at, ev)


def _stopped_result(call: _DecodeCall, out, length, reason, stop_index):
    """The tail of both loops: the kept columns of the output matrix `out` and what was recorded beside them."""
    check_collectives()
    width = int(length.max().item()) if out.shape[0] else 0  # (the one synchronisation of the generation)
    past = torch.arange(width, device=out.device)[None, :] >= length[:, None]
    return call.result(out[:, :width], past, stopping.Finish(length, reason, stop_index) if call.finish else None)


def _decode_steps_stop(model, call: _DecodeCall, first, start):
    """_decode_steps with the stop conditions of call.stop decided by hyd_stop_update after every sampling launch: the kernel
    writes the output matrix, keeps lengths and finish reasons, and hands back the token and the position to feed next."""
    # (penalties: decode has switched the sampler's own append on -- nothing is overridden here -- so the list of generated
    # tokens follows the draws; what a finished row draws goes nowhere else)
    dev, spec = first.device, call.stop
    retire, shared_len, start_pos = _row_origin(model, start)
    out, length, reason, stop_index, live = stopping.new_state(first.shape[0], call.max_new_tokens, spec, dev)
    stop_tokens = spec.stop_table(dev)[0] if spec.stops else None
    poll = _RunningPoll(model, call.max_new_tokens) if dev.type == "cuda" else None  # (CPU rows: live is read as it is)

    def update(tok, t):
        return layer_ops.stop_update(tok, t, spec, out, length, reason, stop_index, live, start_pos, shared_len, retire, stop_tokens,
                                     max_len=call.max_len)

    feed, pos = update(first, 0)
    steps = 1  # columns of `out` written
    for step in range(call.max_new_tokens - 1):
        logits, nxt, lp = _step(model, call, feed[:, None], pos[:, None], steps)
        call.keep(logits, nxt, lp)
        feed, pos = update(nxt, steps)
        steps += 1
        if poll is None:
            if int(live[steps - 1]) == 0:
                break
            continue
        if poll.none_running():
            break
        poll.start(live, steps, steps - 1)
    return _stopped_result(call, out, length, reason, stop_index)


def _decode_steps_draft(model, call: _DecodeCall, first, start):
    """The decode loop with draft_tokens = K: per step the drafts (hyd_draft_lookup, or a gather from the given ones), ONE
    forward over [B, K + 1] with all its logits, one draw per logits row along the call's route, then hyd_draft_accept, which
    keeps the output matrix, the lengths and the finish reasons and hands back each row's next token and position.  The host
    polls the running-row count through the stop loop's _RunningPoll."""
    dev, B = first.device, first.shape[0]
    d, spec = call.draft, call.stop
    K, mx = d.k, call.max_new_tokens
    T = K + 1
    retire, shared_len, start_pos = _row_origin(model, start)
    want_lp = call.logprobs is not None
    out, length, reason, stop_index, out_lp = speculative.new_state(B, mx, spec.pad, dev, want_lp)
    live = torch.zeros((mx,), dtype=torch.int32, device=dev)
    eos = spec.eos
    # stop sequences and the penalties' token lists ride on the accept (hyd_draft_accept_stop): it judges every emitted token and
    # is the one place that knows which draws became output.  Without either the calls are hyd_draft_accept(_states) as before.
    extra = {}
    if spec.stops:
        extra.update(stop=spec, stop_tokens=spec.stop_table(dev)[0])
    pen = call.pen
    if pen is not None:
        extra.update(gen=pen.gen, gen_len=pen.gen_len)
    penalised = call.sample.get("penalties") is not None and call.sample["penalties"].active()
    if penalised and (call.route.draw != sampling.PENALIZED or call.route.torch_penalties):
        raise NotImplementedError("draft_tokens with penalties or logit_bias needs the fused penalty kernel (fused_penalties): the "
                                  "draws of a speculative step count the drafts in front of them inside hyd_sample_tokens_penalized_drafts")

    def accept(fed, sampled, lp, slot, states=None):
        return speculative.draft_accept(fed, sampled, out, length, reason, stop_index, live[slot : slot + 1], start_pos, shared_len,
                                        eos, spec.pad, mx, retire, lp, out_lp if lp is not None else None, states, **extra)

    # constraint=: the rows' automaton states (already advanced by the first draw) and, per step, the state behind every fed
    # token -- the sampler's state array over the step's B * T logits rows, advanced in place, then read by the accept
    dfa, state = call.sample.get("constraint") or (None, None)
    sample = call.sample
    if dfa is not None:
        step_state = torch.empty((B, T), dtype=torch.int32, device=dev)
        n_forced = torch.empty((B,), dtype=torch.int32, device=dev)
        forced = torch.zeros((B,), dtype=torch.int64, device=dev)
        sample = dict(call.sample, constraint=(dfa, step_state.view(-1)))
        dfa.forced  # (made once per automaton, before the loop)

    # the first token, drawn from the prefill logits, enters like a step of one token
    first = first.reshape(B, 1).long()
    feed, pos, _ = accept(first, first, call.logprobs[0].reshape(B, 1).float() if want_lp else None, 0)
    given = d.given
    if given is not None:
        if given.shape[0] != B:
            raise ValueError(f"draft holds {given.shape[0]} rows for a batch of {B}")
        given = given.to(dev).long()
    segments = d.segments + [speculative.Segment(out, length)]
    cols = torch.arange(K, device=dev)[None, :]
    offs = torch.arange(T, device=dev)[None, :]
    fed = torch.full((B, T), spec.pad, dtype=torch.int64, device=dev)
    proposed = torch.zeros((B,), dtype=torch.int64, device=dev)
    accepted = torch.zeros((B,), dtype=torch.int64, device=dev)
    poll = _RunningPoll(model, mx)
    steps = 0
    for step in range(1, mx):
        fed[:, 0] = feed
        # a draft counts as proposed when accepting it can add a token: the one for output position p lets the draw for p + 1
        # out, so a row with `length` tokens has room for max_new_tokens - 1 - length of them (0 for a finished row)
        room = (mx - 1 - length).clamp_(min=0) * (reason == 0)
        n_prop = None
        if given is not None:
            fed[:, 1:] = given.gather(1, (length.long()[:, None] + cols).clamp_(max=mx - 1))
            if dfa is not None:
                n_prop = torch.full((B,), K, dtype=torch.int32, device=dev)
        elif d.only_forced:
            n_prop = torch.zeros((B,), dtype=torch.int32, device=dev)
        else:
            _, n_prop = speculative.draft_lookup(segments, B, K, d.ngram, out=fed[:, 1:])
        compare, states = fed, None
        if dfa is not None:
            # forced states replace drafts, a draft the automaton rejects ends the row's proposal (hyd_draft_constrain)
            speculative.constrain_drafts(dfa, state, fed, n_prop, d.only_forced, step_state, n_forced)
            forced += torch.minimum(n_forced, room)
            states = (step_state, state)
            if d.only_forced:
                # behind the end of the forced chain the columns hold whatever an earlier step left and their draws are
                # unconstrained: the accept compares them with a value no token equals, so none of those draws is kept
                compare = torch.where(offs <= n_prop[:, None], fed, torch.full_like(fed, -1))
        proposed += room.clamp(max=K) if n_prop is None else torch.minimum(n_prop, room)
        logits = model(input_ids=fed, position_ids=pos[:, None] + offs, use_graph=call.graphed, full_logits=True, raw_logits=call.raw)
        tok, lp = draw_tokens(call.route, logits.reshape(B * T, -1), **sample, **(dict(drafts=fed) if penalised else {}))
        feed, pos, acc = accept(compare, tok.reshape(B, T), lp.reshape(B, T).float() if want_lp else None, step, states)
        accepted += acc
        steps += 1
        if poll.none_running():
            break
        poll.start(live, steps, step)
    if want_lp:
        call.logprobs = [out_lp]
    ret = _stopped_result(call, out, length, reason, stop_index)
    if d.stats:
        ret = (ret if isinstance(ret, tuple) else (ret,)) + (speculative.DraftStats(steps, proposed, accepted, forced if dfa is not None else None),)
    return ret
