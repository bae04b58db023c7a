"""-m "not gpu": speculative decoding under a token automaton -- the definitions in numpy / torch (constraint.forced_tokens_reference,
speculative.constrain_drafts_reference, speculative.accept_states_reference) on hand-written cases, and the step loop written with
them against one-token-at-a-time constrained decoding on random automata."""
import math
from pathlib import Path

import pytest
import torch

from hydragen_amd import sampling, speculative
from hydragen_amd.constraint import TokenDFA, forced_tokens_reference, pack_allowed
from hydragen_amd.sampling import DFA_FREE as FREE
from hydragen_amd.sampling import DFA_REJECT as REJ


# ---- forced_tokens_reference -----------------------------------------------------------------------------------------------------
def bitmap(rows, n, stride=None):
    """rows: per state the list of set bit positions (positions >= n allowed: stray bits) -> int32 [S, stride]."""
    words = (n + 31) // 32
    stride = stride or words
    out = torch.zeros((len(rows), stride), dtype=torch.int64)
    for s, bits in enumerate(rows):
        for v in bits:
            out[s, v // 32] |= 1 << (v % 32)
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


def hand_rows(n):
    """(bit positions per state, forced token per state): 0, 1 and 2 bits, a lone bit at token 0, at n - 1, in the partial last
    word, and a lone bit below n with stray bits at >= n (still forced)."""
    last_word = (n - 1) // 32 * 32  # first position of the (partial) last word
    top = ((n + 31) // 32) * 32     # first position past the row's words
    rows = [([], -1), ([5], 5), ([3, 17], -1), ([0], 0), ([n - 1], n - 1), ([last_word], last_word), ([0, n - 1], -1),
            (list(range(n)), -1), ([31], 31), ([32 % n], 32 % n)]
    if n < top:  # stray bits at positions n .. top - 1 are ignored
        rows += [([7] + list(range(n, top)), 7), (list(range(n, top)), -1), ([n - 1, n], n - 1)]
    return [r for r, _ in rows], [f for _, f in rows]


@pytest.mark.parametrize("n", [33, 50, 64, 1000])
def test_forced_tokens_reference_on_hand_written_bitmaps(n):
    rows, want = hand_rows(n)
    assert forced_tokens_reference(bitmap(rows, n), n).tolist() == want
    wide = bitmap(rows, n, stride=(n + 31) // 32 + 3)
    wide[:, (n + 31) // 32:] = -1  # words past ceil(n / 32) are not part of the row
    assert forced_tokens_reference(wide, n).tolist() == want


def test_token_dfa_keeps_its_forced_tokens():
    dfa = TokenDFA.from_choices([[4, 5, 6], [4, 7]], 40, eos=[1])
    # states: 0 -4-> 1 -5-> 2 -6-> 3 (accepting), 1 -7-> 4 (accepting), sinks 5, 6 behind EOS
    assert dfa.forced.tolist() == [4, -1, 6, 1, 1, 1, 1]
    assert dfa.forced is dfa.forced and dfa.to("cpu").forced.tolist() == dfa.forced.tolist()
    assert torch.equal(dfa.forced, forced_tokens_reference(pack_allowed(dfa.next), 40))


# ---- constrain_drafts_reference / accept_states_reference: hand cases ----------------------------------------------------------------
def hand_dfa():
    """n = 10.  0 -3-> 1 -4-> 2 -5-> 3 -6-> 4: a forced chain of four; 4 allows 7 (FREE) alone; 5 allows 1 -> 6 and 2 -> 5;
    6 allows 8 -> 0 alone."""
    nxt = torch.full((7, 10), REJ, dtype=torch.int32)
    for s, t, e in ((0, 3, 1), (1, 4, 2), (2, 5, 3), (3, 6, 4), (4, 7, FREE), (5, 1, 6), (5, 2, 5), (6, 8, 0)):
        nxt[s, t] = e
    return TokenDFA(nxt)


def constrain(dfa, state, drafts, n_prop=None, only_forced=False):
    fed = torch.tensor([[9] + d for d in drafts])
    np_ = None if n_prop is None else torch.tensor(n_prop, dtype=torch.int32)
    ss, nf = speculative.constrain_drafts_reference(dfa, torch.tensor(state, dtype=torch.int32), fed, np_, only_forced)
    return fed[:, 1:].tolist(), ss.tolist(), nf.tolist(), None if np_ is None else np_.tolist()


def test_constrain_drafts_hand_cases():
    dfa = hand_dfa()
    assert dfa.forced.tolist() == [3, 4, 5, 6, 7, -1, 8]
    # a forced chain longer than K: every draft is replaced, every step state is the chain's
    assert constrain(dfa, [0], [[0, 0, 0]], [0]) == ([[3, 4, 5]], [[0, 1, 2, 3]], [3], [3])
    # ... that ends in FREE: the row is unconstrained (-2) from then on and its drafts stay
    assert constrain(dfa, [3], [[0, 0, 9, 2]], [4]) == ([[6, 7, 9, 2]], [[3, 4, -2, -2, -2]], [2], [4])
    # a REJECT draft in the middle cuts n_proposed and every later step state is -1
    assert constrain(dfa, [5], [[2, 2, 3, 1]], [4]) == ([[2, 2, 3, 1]], [[5, 5, 5, -1, -1]], [0], [2])
    # an allowed draft into a forced state: the forced token overrides the proposal and raises n_proposed
    assert constrain(dfa, [5], [[1, 0, 0]], [1]) == ([[1, 8, 3]], [[5, 6, 0, 1]], [2], [3])
    # unconstrained rows: states -1, -2 and >= S keep state and drafts
    assert constrain(dfa, [-1, -2, 7], [[1, 2]] * 3, [2, 0, 1]) == ([[1, 2]] * 3, [[-1] * 3, [-2] * 3, [7] * 3], [0] * 3, [2, 0, 1])
    # a draft token outside [0, n) is rejected without a table read
    assert constrain(dfa, [5, 5], [[2, 10, 1], [-1, 1, 1]], [3, 3]) == ([[2, 10, 1], [-1, 1, 1]], [[5, 5, -1, -1], [5, -1, -1, -1]], [0, 0], [1, 0])
    # only_forced: the chain ends at the first state that is not forced, the remaining drafts keep what they hold
    assert constrain(dfa, [6, 5, -1], [[2, 2, 2, 2, 2, 2]] * 3, [0, 0, 0], True) == (
        [[8, 3, 4, 5, 6, 7], [2] * 6, [2] * 6], [[6, 0, 1, 2, 3, 4, -2], [5] + [-1] * 6, [-1] * 7], [6, 0, 0], [6, 0, 0])
    assert constrain(dfa, [3], [[1, 1, 1]], [0], True) == ([[6, 7, 1]], [[3, 4, -2, -1]], [2], [2])
    # n_proposed = None: nothing is counted, everything else is the same
    assert constrain(dfa, [5], [[2, 2, 3, 1]]) == ([[2, 2, 3, 1]], [[5, 5, 5, -1, -1]], [0], None)


def test_accept_states_hand_cases():
    T, mx, pad = 4, 6, 0
    fed = torch.tensor([[9, 3, 4, 5], [9, 3, 4, 5], [9, 3, 4, 5], [9, 3, 4, 5], [9, 3, 4, 5]])
    sampled = torch.tensor([[3, 4, 5, 6], [3, 8, 5, 6], [7, 4, 5, 6], [3, 4, 5, 6], [3, 4, 5, 6]])
    after = torch.tensor([[11, 12, 13, 14]] * 5, dtype=torch.int32)
    out, length, reason, stop_index, _ = speculative.new_state(5, mx, pad)
    length[3], reason[4] = 4, 1  # row 3 has room for two tokens, row 4 has finished
    state = torch.full((5,), 77, dtype=torch.int32)
    plain = speculative.new_state(5, mx, pad)
    plain[1][3], plain[2][4] = 4, 1
    start = torch.zeros(5, dtype=torch.int64)
    got = speculative.accept_states_reference(fed, sampled, after, state, out, length, reason, stop_index, start, None, [8], pad, mx)
    want = speculative.accept_reference(fed, sampled, *plain[:4], start, None, [8], pad, mx)
    # all accepted -> the state behind the fourth draw; cut at an EOS -> behind the EOS; first draft wrong -> behind the first
    # draw; cut at max_new_tokens -> behind the last token that fits; a finished row keeps its state
    assert state.tolist() == [14, 12, 11, 12, 77]
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
    assert all(torch.equal(a, b) for a, b in zip((out, length, reason, stop_index), plain[:4]))


# ---- the step loop written with the references == sequential constrained decoding -----------------------------------------------
S, N, MX, EOS, PAD = 8, 50, 20, 49, 0


def random_dfa(seed, forced_states=3):
    """S = 8 states over n = 50 tokens: `forced_states` states allow one token, the others 2 .. 40; targets are states, with
    some FREE entries; every state allows something."""
    g = torch.Generator().manual_seed(seed)
    nxt = torch.full((S, N), REJ, dtype=torch.int32)
    for s in range(S):
        k = 1 if s < forced_states else int(torch.randint(2, 41, (1,), generator=g))
        toks = torch.randperm(N, generator=g)[:k]
        tgt = torch.randint(0, S, (k,), generator=g).to(torch.int32)
        tgt[torch.rand(k, generator=g) < 0.05] = FREE
        nxt[s, toks] = tgt
    perm = torch.randperm(S, generator=g)  # (the forced states are not the first ones)
    inv = torch.argsort(perm).to(torch.int32)
    nxt = torch.where(nxt >= 0, inv[nxt.clamp(min=0).long()], nxt)[perm]
    return TokenDFA(nxt)


def fake_logits(table, states, positions):
    """The fake model: logits are a fixed table [states + 1, positions, n] by (automaton state -- the unconstrained states share the
    last row --, output position)."""
    n_states = table.shape[0] - 1
    idx = torch.where((states >= 0) & (states < n_states), states, torch.full_like(states, n_states)).long()
    return table[idx, positions.long().clamp(max=table.shape[1] - 1)]


def sequential(dfa, table, start):
    """One token per step: masked argmax, advance_state.  A row stops behind EOS."""
    B = start.shape[0]
    state = start.clone()
    out = torch.full((B, MX), PAD, dtype=torch.int64)
    length = torch.zeros(B, dtype=torch.int64)
    done = torch.zeros(B, dtype=torch.bool)
    for p in range(MX):
        x = sampling.constrain_logits(fake_logits(table, state, torch.full((B,), p)), dfa, state)
        tok = x.argmax(-1)
        new = sampling.advance_state(dfa, state, tok)
        run = ~done
        out[run, p] = tok[run]
        length[run] += 1
        state = torch.where(run, new, state)
        done |= tok == EOS
    return out, length, state


def speculative_loop(dfa, table, start, K, drafts, only_forced):
    """The loop generate() runs, on the references.  drafts(out, length) -> int64 [B, K] proposals, or None with only_forced.
    max_new_tokens is the table's number of positions."""
    MX = table.shape[1]
    B, T = start.shape[0], K + 1
    state = start.clone()
    out, length, reason, stop_index, _ = speculative.new_state(B, MX, PAD)
    pos0, offs = torch.zeros(B, dtype=torch.int64), torch.arange(T)[None, :]
    first = sampling.constrain_logits(fake_logits(table, state, pos0), dfa, state).argmax(-1)
    state.copy_(sampling.advance_state(dfa, state, first))
    feed = speculative.accept_reference(first[:, None], first[:, None], out, length, reason, stop_index, pos0, None, [EOS], PAD, MX)[0]
    fed = torch.full((B, T), PAD, dtype=torch.int64)
    steps = forced = proposed = accepted = 0
    while bool(((reason == 0) & (length < MX)).any()):
        fed[:, 0] = feed
        room = (MX - 1 - length).clamp(min=0) * (reason == 0)
        if only_forced:
            n_prop = torch.zeros(B, dtype=torch.int32)
        else:
            fed[:, 1:] = drafts(out, length)
            n_prop = torch.full((B,), K, dtype=torch.int32)
        step_state, n_forced = speculative.constrain_drafts_reference(dfa, state, fed, n_prop, only_forced)
        compare = torch.where(offs <= n_prop[:, None], fed, torch.full_like(fed, -1)) if only_forced else fed
        flat = step_state.view(-1)
        x = sampling.constrain_logits(fake_logits(table, flat, (length.long()[:, None] + offs).reshape(-1)), dfa, flat)
        tok = x.argmax(-1)
        flat.copy_(sampling.advance_state(dfa, flat, tok))
        feed, _, acc, _ = speculative.accept_states_reference(compare, tok.view(B, T), step_state, state, out, length, reason, stop_index,
                                                              pos0, None, [EOS], PAD, MX)
        steps += 1
        forced += int(torch.minimum(n_forced, room).sum())
        proposed += int(torch.minimum(n_prop, room).sum())
        accepted += int(acc.sum())
        assert steps <= MX
    return out, length.long(), state, (steps, proposed, forced, accepted)


@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("seed", range(6))
def test_the_step_loop_on_the_references_equals_sequential_decoding(seed, K):
    dfa = random_dfa(seed)
    g = torch.Generator().manual_seed(100 + seed)
    table = torch.randn((S + 1, MX, N), generator=g)
    table[:, :, EOS] += 1.0  # (some rows end early)
    start = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, -1, -2, S + 3, 0], dtype=torch.int32)
    want = sequential(dfa, table, start)

    def perfect(out, length):  # the sequential tokens where they exist, junk behind a row's end
        cols = (length.long()[:, None] + torch.arange(K)[None, :]).clamp(max=MX - 1)
        return want[0].gather(1, cols)

    def noisy(out, length):  # two drafts in three are right, the others random (often rejected by the automaton, or outside [0, n))
        d = perfect(out, length)
        junk = torch.randint(-2, N + 2, d.shape, generator=g)
        return torch.where(torch.rand(d.shape, generator=g) < 0.66, d, junk)

    for name, drafts, only in (("perfect", perfect, False), ("noisy", noisy, False), ("forced chain", None, True)):
        out, length, state, (steps, proposed, forced, accepted) = speculative_loop(dfa, table, start, K, drafts, only)
        assert torch.equal(length, want[1]) and torch.equal(out, want[0]) and torch.equal(state, want[2]), name
        assert accepted <= proposed and forced <= proposed
        if only:
            assert forced == proposed == accepted  # a forced draft is accepted by construction
    total = int(want[1].sum()) - len(start)
    assert total > 0


# ---- the fully forced automaton: the closed form of the step count -----------------------------------------------------------------
def forced_steps(length: int, K: int) -> int:
    """Steps of a generation whose every draft is accepted, for a row that emits `length` tokens (its EOS included): hyd_draft_accept
    emits n + 1 = K + 1 tokens per step while all K drafts equal the draws (cut behind the EOS), and the first token enters by a
    step of its own, drawn from the prefill logits: 1 + ceil((length - 1) / (K + 1))."""
    return 1 + math.ceil((length - 1) / (K + 1))


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("n_tokens", [20, 8, 1])
def test_a_fully_forced_choice_takes_the_closed_form_number_of_steps(K, n_tokens):
    choice = [(7 * i + 3) % 48 + 1 for i in range(n_tokens)]
    dfa = TokenDFA.from_choices([choice], N, eos=[EOS])
    assert bool((dfa.forced >= 0).all())
    total = n_tokens + 1  # with the EOS; max_new_tokens = total, so that only drafts that can become output count as proposed
    table = torch.randn((dfa.num_states + 1, total, N), generator=torch.Generator().manual_seed(K))
    out, length, state, (steps, proposed, forced, accepted) = speculative_loop(dfa, table, torch.zeros(3, dtype=torch.int32), K, None, True)
    assert out.tolist() == [choice + [EOS]] * 3 and length.tolist() == [total] * 3
    assert 1 + steps == forced_steps(total, K)  # (the loop counts the steps behind the first token's)
    # every step emits its accepted drafts and one more draw: total = 1 + steps + accepted per row
    assert proposed == forced == accepted == 3 * (total - 1 - steps)


# ---- the public face ---------------------------------------------------------------------------------------------------------------
def test_draft_stats_still_unpacks_as_three_fields():
    s = speculative.DraftStats(3, torch.ones(2), torch.zeros(2))
    steps, proposed, accepted = s
    assert steps == 3 and s.forced is None and len(s) == 3 and s._fields == ("steps", "proposed", "accepted")
    assert speculative.DraftStats(3, proposed, accepted, torch.ones(2)).forced.tolist() == [1, 1]


def test_generate_checks_the_constraint_draft_arguments():
    from tests.test_speculative import PROMPT, cpu_model

    model = cpu_model()
    with pytest.raises(ValueError, match="needs constraint"):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, draft="constraint")
    dfa = TokenDFA.from_choices([[1, 2]], model.vocab_size, on_accept="free")
    for kw, words in ((dict(repetition_penalty=1.2), "penalties"), (dict(stop=[[1, 2]]), "stop"), (dict(return_logits=True), "return_logits")):
        with pytest.raises(NotImplementedError, match=words):
            model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, draft="constraint", constraint=dfa, **kw)


def test_abi_mirrors_of_the_new_parameter_blocks_have_the_c_sizes():
    import ctypes as C
    import subprocess
    import tempfile

    from hydragen_amd import _lib

    repo = Path(__file__).resolve().parent.parent
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %zu\\n", sizeof(hyd_dfa_forced_params), '
           'sizeof(hyd_draft_constrain_params), sizeof(hyd_draft_accept_params));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(repo / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        sizes = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert sizes == [C.sizeof(_lib.DfaForcedParams), C.sizeof(_lib.DraftConstrainParams), C.sizeof(_lib.DraftAcceptParams)]


@pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")
def test_the_new_kernels_use_no_scratch_and_no_lds():
    """One wave per state with a shuffle reduction, one row per lane, one row per lane: nothing in LDS, nothing in scratch."""
    import re

    from tests.test_build_quality import _device_asm, _metadata

    ks = _metadata("draft_constrain.hip")[1] + [k for k in _metadata("draft_accept.hip")[1] if "draft_accept_kernel" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    # dfa_forced_kernel<vector loads or not>, draft_constrain_kernel, draft_accept_kernel<with states or not>
    assert len(ks) == 5 and names.count("dfa_forced_kernel") == 2 and "draft_constrain_kernel" in names, names
    for k in ks:
        print(k)
        assert k["scratch"] == 0 and k["spill"] == 0 and k["sspill"] == 0 and k["vgpr"] <= 64, k
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", _device_asm("draft_constrain.hip") + _device_asm("draft_accept.hip"))
    assert len(lds) == 5 and all(int(x) == 0 for x in lds), lds
