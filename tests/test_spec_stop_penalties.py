"""-m "not gpu": speculative decoding with stop sequences, penalties and logit bias -- the C surface (hyd_draft_accept_stop,
hyd_sample_tokens_penalized_drafts: exports, unchanged structs, refusals before any launch) and the torch definitions
(speculative.accept_stop_reference against one-token stopping.stop_update_reference steps over whole generations,
sampling.draft_row_lists_reference)."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, sampling, speculative, stopping
from tests import spec_stop_cases as cases

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "hydragen_hip.h").read_text()


# ---- exports and ABI ---------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_declared_and_listed_with_the_issue_signatures():
    flat = re.sub(r"\s+", " ", HEADER)
    assert ("HYD_API int hyd_draft_accept_stop(const hyd_draft_accept_params* p, const hyd_stop_params* stop, const int32_t* step_state_after, "
            "int32_t* state, int32_t* gen, int32_t* gen_len, int32_t gen_stride, void* stream);") in flat
    assert "HYD_API int hyd_sample_tokens_penalized_drafts(const hyd_sample_penalty_params* p, const int64_t* fed, int32_t T, void* stream);" in flat
    ptr = C.c_void_p
    assert _lib.EXPORTS["hyd_draft_accept_stop"] == (C.c_int, [C.POINTER(_lib.DraftAcceptParams), C.POINTER(_lib.StopParams), ptr, ptr, ptr, ptr,
                                                              C.c_int32, ptr])
    assert _lib.EXPORTS["hyd_sample_tokens_penalized_drafts"] == (C.c_int, [C.POINTER(_lib.SamplePenaltyParams), ptr, C.c_int32, ptr])
    lib = _lib.load()  # (load() resolves every listed name: a hidden symbol fails here)
    assert lib.hyd_version() == 500 and _lib.ABI_VERSION == 500


def test_no_struct_changed_its_size():
    """The new calls take existing structs and plain arguments: every struct the header declares has the size its mirror has, and
    the three these calls read have the sizes they had before (8-byte pointers)."""
    names = re.findall(r"^\} (hyd_\w+);", HEADER, flags=re.M)
    assert len(names) >= 20
    src = '#include "hydragen_hip.h"\n#include <stdio.h>\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        sizes = dict(line.split() for line in subprocess.check_output([str(Path(d) / "s")]).decode().splitlines())
    mirrors = {"hyd_draft_accept_params": _lib.DraftAcceptParams, "hyd_stop_params": _lib.StopParams, "hyd_sample_penalty_params": _lib.SamplePenaltyParams}
    for name, m in mirrors.items():
        assert int(sizes[name]) == C.sizeof(m), name
    assert {n: int(sizes[n]) for n in ("hyd_draft_accept_params", "hyd_stop_params", "hyd_sample_penalty_params")} == PINNED_SIZES


PINNED_SIZES = {"hyd_draft_accept_params": 280, "hyd_stop_params": 384, "hyd_sample_penalty_params": 304}


# ---- refusals, before any launch and without a device ------------------------------------------------------------------------------
def _accept(**kw):
    p = _lib.DraftAcceptParams()
    for i, name in enumerate(("fed", "sampled", "out", "start_pos", "feed", "next_pos")):
        setattr(p, name, 0x10000 + 0x1000 * i)
    for i, name in enumerate(("length", "reason", "stop_index", "accepted", "live")):
        setattr(p, name, 0x20000 + 0x1000 * i)
    p.out_stride, p.rows, p.T, p.n_eos, p.max_new_tokens = 32, 4, 4, 1, 32
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _stop(n_stop=2, lens=(2, 16), stop_tokens=0x30000):
    s = _lib.StopParams()
    s.n_stop, s.stop_tokens = n_stop, stop_tokens
    for k, n in enumerate(lens):
        s.stop_lens[k] = n
    return s


GEN = dict(gen=0x40000, gen_len=0x41000, gen_stride=64)


@pytest.mark.parametrize("p, stop, rest, frag", [
    (dict(fed=0), _stop(), {}, "is null"), (dict(T=9), _stop(), {}, "1 to 8 tokens"), (dict(T=0), _stop(), {}, "1 to 8 tokens"),
    (dict(rows=-1), _stop(), {}, "rows -1"), (dict(n_eos=17), _stop(), {}, "n_eos"), (dict(max_new_tokens=33), _stop(), {}, "max_new_tokens"),
    (dict(out=0x10004), _stop(), {}, "not aligned"), (dict(length=0x20002), _stop(), {}, "not aligned"),
    ({}, _stop(), dict(after=0x50000), "go together"), ({}, _stop(), dict(state=0x50000), "go together"),
    ({}, _stop(), dict(after=0x50002, state=0x51000), "not aligned"),
    ({}, _stop(n_stop=-1), {}, "n_stop -1"), ({}, _stop(n_stop=_lib.STOP_MAX_SEQS + 1), {}, "n_stop 33"),
    ({}, _stop(stop_tokens=None), {}, "needs stop_tokens"), ({}, _stop(lens=(0, 3)), {}, "stop_lens[0] = 0"),
    ({}, _stop(lens=(2, 17)), {}, "stop_lens[1] = 17"), ({}, _stop(stop_tokens=0x30004), {}, "not aligned"),
    ({}, None, dict(gen=0x40000), "gen and gen_len go together"), ({}, None, dict(gen_len=0x41000), "gen and gen_len go together"),
    ({}, None, dict(GEN, gen_stride=-1), "gen_stride -1"), ({}, None, dict(GEN, gen_stride=_lib.SAMPLE_GEN_MAX + 1), "gen_stride 2049"),
    ({}, _stop(), dict(GEN, gen=0x40002), "not aligned"), ({}, None, dict(GEN, gen_len=0x41002), "not aligned"),
])
def test_draft_accept_stop_refusals_come_with_their_message_before_any_launch(p, stop, rest, frag):
    lib = _lib.load()
    rc = lib.hyd_draft_accept_stop(C.byref(_accept(**p)), None if stop is None else C.byref(stop), rest.get("after"), rest.get("state"),
                                   rest.get("gen"), rest.get("gen_len"), rest.get("gen_stride", 0), None)
    assert rc == -1 and frag in lib.hyd_last_error_string().decode(), lib.hyd_last_error_string().decode()


def test_draft_accept_stop_null_params_and_zero_rows():
    lib = _lib.load()
    assert lib.hyd_draft_accept_stop(None, None, None, None, None, None, 0, None) == -1 and "null params" in lib.hyd_last_error_string().decode()
    assert lib.hyd_draft_accept_stop(C.byref(_accept(rows=0)), C.byref(_stop()), None, None, GEN["gen"], GEN["gen_len"], 64, None) == 0  # no launch


def _penalty(**kw):
    p = _lib.SamplePenaltyParams()
    p.logits, p.out, p.row_stride, p.rows, p.n, p.dtype = 0x10000, 0x20000, 1024, 8, 1024, 1
    p.temperature, p.top_p, p.repetition_penalty = 1.0, 1.0, 1.2
    p.gen, p.gen_len, p.gen_stride = 0x30000, 0x31000, 64
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, fed, T, code, frag", [
    (dict(logits=0), 0x40000, 4, -1, "is null"), (dict(repetition_penalty=0.0), 0x40000, 4, -1, "repetition_penalty"),
    (dict(top_p=0.0), 0x40000, 4, -1, "top_p"), (dict(gen_len=0), 0x40000, 4, -1, "gen and gen_len"),
    (dict(gen_stride=_lib.SAMPLE_GEN_MAX + 1), 0x40000, 4, -2, "gen_stride"), (dict(dtype=7), 0x40000, 4, -2, "dtype"),
    (dict(n_bias=3), 0x40000, 4, -1, "n_bias"), (dict(n_context=1), 0x40000, 4, -1, "context[0]"),
    ({}, 0x40000, 0, -1, "T = 0"), ({}, 0x40000, 9, -1, "T = 9"), ({}, 0x40000, 3, -1, "not a multiple of T = 3"),
    (dict(append_out=1), 0x40000, 4, -1, "append_out"), ({}, None, 4, -1, "gen needs fed"), ({}, 0x40004, 4, -1, "not aligned"),
])
def test_penalized_drafts_refusals_come_with_their_message_before_any_launch(kw, fed, T, code, frag):
    lib = _lib.load()
    assert lib.hyd_sample_tokens_penalized_drafts(C.byref(_penalty(**kw)), fed, T, None) == code
    assert frag in lib.hyd_last_error_string().decode(), lib.hyd_last_error_string().decode()
    assert lib.hyd_sample_tokens_penalized_drafts(None, fed, T, None) == -1


# ---- accept_stop_reference against the sequential form -----------------------------------------------------------------------------
def sequential_accept(spec, max_new, counts=None):
    """The accepted draws of every running row, fed one at a time through stopping.stop_update_reference (one row, t = the row's
    column); lists, log-probs, states and the next step's token and position by their plain rules.  counts: a dict that
    receives the kinds of rows this step saw (module docstring of the test below), judged here on the sequential form."""
    def accept(fed, sampled, lp, after, st):
        rows, T = fed.shape
        feed = torch.full((rows,), spec.pad, dtype=torch.int64)
        pos = torch.empty((rows,), dtype=torch.int64)
        acc = torch.zeros((rows,), dtype=torch.int32)
        live = 0
        scratch = torch.zeros((max_new,), dtype=torch.int32)
        for b in range(rows):
            if int(st.reason[b]) == 0 and int(st.length[b]) < max_new:
                n = 0
                while n < T - 1 and int(fed[b, n + 1]) == int(sampled[b, n]):
                    n += 1
                e = 0
                for i in range(min(n + 1, max_new - int(st.length[b]))):
                    t = int(st.length[b])
                    assert t == int(st.length[b])
                    f, _ = stopping.stop_update_reference(sampled[b: b + 1, i], t, spec, st.out[b: b + 1], st.length[b: b + 1], st.reason[b: b + 1],
                                                          st.stop_index[b: b + 1], scratch, st.start_pos[b: b + 1], st.shared_len[b: b + 1], True)
                    st.out_lp[b, t] = lp[b, i]
                    if int(st.gen_len[b]) < st.gen.shape[1]:
                        st.gen[b, int(st.gen_len[b])] = int(sampled[b, i])
                    st.gen_len[b] += 1
                    e += 1
                    if int(st.reason[b]) != 0:
                        break
                st.state[b] = after[b, e - 1]
                acc[b] = e - 1
                feed[b] = f[0]
            running = int(st.reason[b]) == 0 and int(st.length[b]) < max_new
            live += running
            if not running:
                feed[b] = spec.pad
            pos[b] = int(st.start_pos[b]) + int(st.length[b]) - 1 if running else int(st.shared_len[b]) - 1
        return feed, pos, acc, live
    return accept


def hits(seq, c, spec):
    """(is EOS, [k of the stop sequences that end at column c of seq])"""
    return seq[c] in spec.eos, [k for k, s in enumerate(spec.stops) if c + 1 >= len(s) and seq[c + 1 - len(s): c + 1] == list(s)]


def count_kinds(records, steps, spec, max_new, kinds):
    """The kinds of rows the issue lists, counted on the reference's own records."""
    before = cases.new_state(cases.ROWS, max_new).snapshot()
    for rec, (fed, sampled, _, _) in zip(records, steps):
        T = fed.shape[1]
        for b in range(cases.ROWS):
            l0, r0 = int(before["length"][b]), int(before["reason"][b])
            if r0 != 0 or l0 >= max_new:
                continue
            n = 0
            while n < T - 1 and int(fed[b, n + 1]) == int(sampled[b, n]):
                n += 1
            room = max_new - l0
            e0, e, r = min(n + 1, room), int(rec["accepted"][b]) + 1, int(rec["reason"][b])
            full = before["out"][b, :l0].tolist() + sampled[b].tolist()  # the row's output and EVERY draw of the step
            if r == 2:
                k = int(rec["stop_index"][b])
                kinds["first"] += e == 1 and e0 > 1
                kinds["middle"] += 1 < e < e0
                kinds["last"] += e == e0 and e0 > 1
                kinds["earlier step"] += len(spec.stops[k]) > e
                kinds["two sequences"] += len(hits(full, l0 + e - 1, spec)[1]) >= 2
            if r == 1:
                kinds["eos and stop"] += len(hits(full, l0 + e - 1, spec)[1]) >= 1
            if r == 0:
                assert e == e0
                kinds["only rejected"] += any(any(map(bool, hits(full, l0 + i, spec))) for i in range(n + 1, T))
                kinds["room cut"] += room < n + 1 and any(map(bool, hits(full, l0 + room, spec)))
            for i in range(e):  # a tail of the first columns that equals a stop's tail, the stop reaching in front of column 0
                c = l0 + i
                kinds["front of column 0"] += any(c + 1 < len(s) and full[: c + 1] == list(s)[len(s) - c - 1:] for s in spec.stops)
        before = rec
    for r in before["reason"].tolist():
        kinds[f"reason {r}"] += 1


KINDS = ("first", "middle", "last", "earlier step", "only rejected", "eos and stop", "two sequences", "front of column 0", "room cut",
         "reason 0", "reason 1", "reason 2")


@pytest.mark.parametrize("include_stop", [False, True])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_accept_stop_reference_equals_one_token_stop_updates_over_whole_generations(K, include_stop):
    """130 rows, drafts right with probability 0.6, EOS [5], five stop sequences, vocabulary 6 / max_new_tokens 24 and vocabulary
    16 / max_new_tokens 10: after EVERY step every buffer of the torch definition equals the sequential form's.  Each kind of row
    the rules distinguish occurs at least once over the two ranges (K = 1 has no middle token)."""
    spec = cases.spec(include_stop)
    kinds = dict.fromkeys(KINDS, 0)
    for name, (vocab, max_new) in cases.RANGES.items():
        steps = cases.step_inputs(K, vocab, max_new, seed=100 * K + ord(name))
        ref = cases.run(cases.reference_accept(spec, max_new), steps, max_new)
        seq = cases.run(sequential_accept(spec, max_new), steps, max_new)
        for s, (a, b) in enumerate(zip(ref, seq)):
            for key in a:
                same = a[key] == b[key] if key == "live" else torch.equal(a[key], b[key])
                assert same, (name, "step", s, key)
        assert ref[-1]["live"] == 0
        count_kinds(ref, steps, spec, max_new, kinds)
    print(K, include_stop, kinds)
    for kind, n in kinds.items():
        assert n >= 1 or (K == 1 and kind == "middle"), (kind, kinds)


# ---- hand-written cases ------------------------------------------------------------------------------------------------------------
def one_step(out_row, fed, sampled, max_new=12, eos=(5,), stops=((4, 1), (1,), (2, 5), (0, 2, 3), (3, 3)), include_stop=False, pad=-1):
    """One row with `out_row` already emitted -> (out row, length, reason, stop_index, accepted, feed, next_pos, live, gen list)."""
    spec = stopping.StopSpec(eos=tuple(eos), stops=tuple(tuple(s) for s in stops), pad=pad, include_stop=include_stop)
    out = torch.full((1, max_new), pad, dtype=torch.int64)
    out[0, : len(out_row)] = torch.tensor(out_row, dtype=torch.int64)
    length, reason, index = torch.tensor([len(out_row)], dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.full((1,), -1, dtype=torch.int32)
    gen, gen_len = torch.zeros((1, 32), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    feed, pos, acc, live = speculative.accept_stop_reference(
        torch.tensor([fed]), torch.tensor([sampled]), out, length, reason, index, torch.tensor([100]), torch.tensor([7]), spec.eos, pad, max_new,
        stop=spec, gen=gen, gen_len=gen_len)
    return (out[0, : max(int(length), 0)].tolist(), int(length), int(reason), int(index), int(acc), int(feed), int(pos), live,
            gen[0, : int(gen_len)].tolist())


def test_hand_written_cases_one_kind_each():
    P = -1
    # a match on the first / a middle / the last token of a three-token run; what lies behind the cut is never written
    assert one_step([0], [9, 4, 3, 3], [4, 3, 3, 0], stops=[(4,)])[:5] == ([0], 1, 2, 0, 0)
    assert one_step([0], [9, 4, 3, 2], [4, 3, 2, 0], stops=[(4, 3)])[:5] == ([0], 1, 2, 0, 1)
    assert one_step([0], [9, 4, 3, 2], [4, 3, 2, 0], stops=[(3, 2)], include_stop=True)[:5] == ([0, 4, 3, 2], 4, 2, 0, 2)
    got = one_step([0], [9, 4, 3, 2], [4, 3, 2, 0], stops=[(4, 3)])
    assert got[5:8] == (P, 6, 0) and got[8] == [4, 3]  # finished: fed pad at shared_len - 1; the judged tokens reach the list, trimmed or not
    # a match that began in an earlier step trims columns that step wrote: the length falls below what it was
    assert one_step([2, 0, 2], [9, 3], [3, 4])[:5] == ([2], 1, 2, 3, 0)
    assert one_step([2, 0, 2], [9, 3], [3, 4], include_stop=True)[:5] == ([2, 0, 2, 3], 4, 2, 3, 0)
    # only a REJECTED draw would complete a match or be the EOS: the row goes on
    assert one_step([0], [9, 2, 0], [4, 1, 5])[:8] == ([0, 4], 2, 0, -1, 0, 4, 101, 1)
    # EOS and a stop sequence on the same token: reason 1 wins, the token is kept
    assert one_step([0], [9, 2], [2, 5])[:5] == ([0, 2, 5], 3, 1, 0, 1)
    # two sequences on the same token: the lowest k wins, and trims its own length
    assert one_step([0], [9, 4], [4, 1])[:5] == ([0], 1, 2, 0, 1)
    assert one_step([0], [9, 4], [4, 1], stops=[(1,), (4, 1)])[:5] == ([0, 4], 2, 2, 0, 1)
    # a tail in the first columns that equals a stop's tail in front of column 0 is no match
    assert one_step([], [9, 2, 3], [2, 3, 0], stops=[(0, 2, 3)])[:5] == ([2, 3, 0], 3, 0, -1, 2)
    # max_new_tokens cuts the run in front of a token that would have stopped it: reason stays 0, the row is not running
    assert one_step([0, 0], [9, 4, 1], [4, 1, 0], max_new=3)[:8] == ([0, 0, 4], 3, 0, -1, 0, P, 6, 0)
    # T = 1: the first token of a generation
    assert one_step([], [9], [1])[:5] == ([], 0, 2, 1, 0)
    assert one_step([], [9], [5])[:5] == ([5], 1, 1, 0, 0)
    assert one_step([], [9], [4])[:8] == ([4], 1, 0, -1, 0, 4, 100, 1)
    # without stop sequences and lists the rules are accept_reference's
    args = lambda: (torch.tensor([[9, 4, 1]]), torch.tensor([[4, 1, 5]]), torch.full((1, 8), P), torch.zeros(1, dtype=torch.int32),
                    torch.zeros(1, dtype=torch.int32), torch.full((1,), -1, dtype=torch.int32), torch.tensor([3]), None, (5,), P, 8)
    a, b = args(), args()
    ra, rb = speculative.accept_reference(*a), speculative.accept_stop_reference(*b)
    assert all(torch.equal(x, y) for x, y in zip(a[2:6], b[2:6])) and all(torch.equal(x, y) for x, y in zip(ra[:3], rb[:3])) and ra[3] == rb[3]


def test_a_sixteen_token_stop_sequence_spanning_three_steps():
    stop = tuple(range(10, 26))
    out, fed = [7], 9
    for chunk in (list(stop[:6]), list(stop[6:12])):
        got = one_step(out, [fed] + chunk[:5], chunk, max_new=40, stops=[stop])
        out = out + chunk
        assert got[:5] == (out, len(out), 0, -1, 5)
    assert one_step(out, [fed] + list(stop[12:]) + [3], list(stop[12:]) + [3, 3], max_new=40, stops=[stop])[:5] == ([7], 1, 2, 0, 3)
    assert one_step(out, [fed] + list(stop[12:]) + [3], list(stop[12:]) + [3, 3], max_new=40, stops=[stop], include_stop=True)[:5] == (
        [7] + list(stop), 17, 2, 0, 3)


# ---- draft_row_lists_reference -------------------------------------------------------------------------------------------------------
def test_draft_row_lists_reference():
    fed = torch.tensor([[1, 2, 3], [4, -5, 99]])
    lists, lens = sampling.draft_row_lists_reference(None, None, fed)  # no lists: the drafts alone
    assert lens.tolist() == [0, 1, 2, 0, 1, 2] and lists.shape == (6, 2)
    assert lists[2].tolist() == [2, 3] and lists[5].tolist() == [-5, 99] and lists[1].tolist() == [2, -1]
    gen = torch.tensor([[7, 8, 9], [6, 6, 6]], dtype=torch.int32)
    lists, lens = sampling.draft_row_lists_reference(gen, torch.tensor([0, 5], dtype=torch.int32), fed)  # empty, and beyond the stride (clamped)
    assert lens.tolist() == [0, 1, 2, 3, 4, 5] and lists.shape == (6, 5)
    assert lists[2, :2].tolist() == [2, 3] and lists[5].tolist() == [6, 6, 6, -5, 99] and lists[3, :3].tolist() == [6, 6, 6]
    # usable with penalize_logits: ids outside [0, n) among the drafts are ignored, the others count with the generated ones
    logits = torch.ones((6, 8))
    x = sampling.penalize_logits(logits, frequency_penalty=1.0, gen=lists, gen_len=lens)
    assert x[5].tolist() == [1, 1, 1, 1, 1, 1, -2, 1] and x[2].tolist() == [1, 1, 0, 0, 1, 1, 1, 1] and x[0].tolist() == [1] * 8


# ---- generate(): what stays refused on a model without a device ----------------------------------------------------------------------
def test_generate_names_what_it_still_refuses():
    from tests.test_speculative import PROMPT, cpu_model

    model = cpu_model()
    kw = dict(num_return_sequences=2, max_new_tokens=4, draft_tokens=2)
    for more, words in ((dict(stop=[[1, 2]]), "stop"), (dict(presence_penalty=0.5), "penalties"), (dict(logit_bias={3: 1.0}), "logit_bias"),
                        (dict(return_logprobs=True, top_logprobs=2), "top_logprobs"), (dict(return_logits=True), "return_logits"),
                        (dict(token_overrides=torch.ones((2, 4), dtype=torch.long)), "token_overrides"),
                        (dict(temperature=[0.5, 1.0]), "per-row"), (dict(seed=[1, 2]), "per-row"), (dict(max_new_tokens=[2, 4]), "per-row")):
        with pytest.raises(NotImplementedError, match=words):
            model.generate(PROMPT, **dict(kw, **more))
