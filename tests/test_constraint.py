"""-m "not gpu": constrained decoding (hyd_sample_tokens_constrained, hydragen_amd/constraint.py) -- the host side: the export and
the struct, every refusal with its message, the automata built from choices and from regular expressions (against Python's re
on a synthetic byte vocabulary), the torch definition on CPU tensors, and the new kernels' registers and LDS."""
import ctypes as C
import math
import random
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, layer_ops, sampling
from hydragen_amd._lib import SamplePenaltyParams, TokenDfa
from hydragen_amd.constraint import TokenDFA, pack_allowed, regex_to_byte_dfa, table_bytes
from hydragen_amd.sampling import DFA_FREE, DFA_REJECT

REPO = Path(__file__).resolve().parent.parent
BAD, UNSUP = -1, -2


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_export_and_struct_layout():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    assert "hyd_sample_tokens_constrained" in set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert "hyd_sample_tokens_constrained" in _lib.EXPORTS and hasattr(lib, "hyd_sample_tokens_constrained")
    assert lib.hyd_version() == 500  # additive: the version stays
    assert "#define HYD_DFA_REJECT (-1)" in header and "#define HYD_DFA_FREE (-2)" in header
    assert (_lib.HYD_DFA_REJECT, _lib.HYD_DFA_FREE) == (DFA_REJECT, DFA_FREE) == (-1, -2)
    fields = ["allowed", "next", "state", "allowed_stride", "next_stride", "n_states", "advance"]
    src = ('#include "hydragen_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu %zu", sizeof(hyd_token_dfa), '
           'sizeof(hyd_sample_penalty_params));' + "".join(f'printf(" %zu", offsetof(hyd_token_dfa, {f}));' for f in fields)
           + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got[0] == C.sizeof(TokenDfa) == 48 and got[1] == C.sizeof(SamplePenaltyParams) == 304  # the existing struct is unchanged
    assert got[2:] == [getattr(TokenDfa, f).offset for f in fields]


def _pp(**kw):
    p = SamplePenaltyParams()
    p.logits = p.out = 4096  # never dereferenced: validation fails first
    p.rows, p.n, p.dtype, p.row_stride = 4, 1000, _lib.HYD_BF16, 1000
    p.temperature, p.top_p = 1.0, 1.0
    p.repetition_penalty = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cc(**kw):
    c = TokenDfa()
    c.allowed = c.next = c.state = 4096
    c.allowed_stride, c.next_stride, c.n_states, c.advance = 32, 1000, 3, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_constrained_argument_validation():
    lib = _lib.load()
    err = lambda: lib.hyd_last_error_string().decode()  # noqa: E731
    call = lambda p, c: lib.hyd_sample_tokens_constrained(C.byref(p), C.byref(c), None)  # noqa: E731
    for field in ("allowed", "next", "state"):
        assert call(_pp(), _cc(**{field: 0})) == BAD and field in err() and "null" in err()
        assert call(_pp(), _cc(**{field: 4098})) == BAD and field in err() and "aligned" in err()
    for ns in (0, -1):
        assert call(_pp(), _cc(n_states=ns)) == BAD and "n_states" in err()
    assert call(_pp(), _cc(allowed_stride=31)) == BAD and "allowed_stride" in err()
    assert call(_pp(n=1025, row_stride=1025), _cc(next_stride=1025)) == BAD and "allowed_stride" in err()  # ceil(1025 / 32) = 33
    assert call(_pp(), _cc(next_stride=999)) == BAD and "next_stride" in err()
    # everything the penalised entry point refuses, with a good automaton
    assert lib.hyd_sample_tokens_constrained(None, C.byref(_cc()), None) == BAD
    assert call(_pp(repetition_penalty=0.0), _cc()) == BAD and "repetition_penalty" in err()
    assert call(_pp(frequency_penalty=math.inf), _cc()) == BAD and "frequency_penalty" in err()
    assert call(_pp(n_context=_lib.SAMPLE_MAX_CONTEXT + 1), _cc()) == BAD and "n_context" in err()
    assert call(_pp(gen=4096), _cc()) == BAD and "gen and gen_len" in err()
    assert call(_pp(append_out=1), _cc()) == BAD and "append_out" in err()
    assert call(_pp(n_bias=3), _cc()) == BAD and "bias_ids" in err()
    assert call(_pp(top_k=-1), _cc()) == BAD and "top_k" in err()
    assert call(_pp(top_p=0.0), _cc()) == BAD and "top_p" in err()
    assert call(_pp(temperature=-1.0), _cc()) == BAD and "temperature" in err()
    assert call(_pp(row_stride=999), _cc()) == BAD and "row_stride" in err()
    assert call(_pp(logits=4097), _cc()) == BAD and "aligned" in err()
    assert call(_pp(dtype=7), _cc()) == UNSUP and "dtype 7" in err()
    assert call(_pp(gen=4096, gen_len=4096, gen_stride=_lib.SAMPLE_GEN_MAX + 1), _cc()) == UNSUP and "gen_stride" in err()
    assert call(_pp(rows=0), _cc()) == 0  # nothing to launch
    # c == NULL: the penalised entry point, its own refusals included
    null = lambda p: lib.hyd_sample_tokens_constrained(C.byref(p), None, None)  # noqa: E731
    assert lib.hyd_sample_tokens_constrained(None, None, None) == BAD
    assert null(_pp(repetition_penalty=-1.0)) == BAD and "repetition_penalty" in err()
    assert null(_pp(min_p=1.5)) == BAD and "min_p" in err()
    assert null(_pp(n=_lib.SAMPLE_FILTER_MAX_N + 1, row_stride=_lib.SAMPLE_FILTER_MAX_N + 1)) == UNSUP
    assert null(_pp(rows=0)) == 0


# ---- automata from choices -------------------------------------------------------------------------------------------------
def _walk(dfa, start, tokens):
    """The states a token sequence goes through, by the table (stops at a state outside the automaton)."""
    s, path = start, []
    for t in tokens:
        assert 0 <= s < dfa.num_states, (s, tokens)
        s = int(dfa.next[s, t])
        path.append(s)
    return path


def _consistent(dfa):
    n = dfa.vocab_size
    shifts = torch.arange(32)
    bits = ((dfa.allowed.long()[:, :, None] >> shifts) & 1).bool().reshape(dfa.num_states, -1)
    assert torch.equal(bits[:, :n], dfa.next != DFA_REJECT) and not bits[:, n:].any()
    assert torch.equal(dfa.allowed, pack_allowed(dfa.next))
    assert int(dfa.next.min()) >= DFA_FREE and int(dfa.next.max()) < dfa.num_states


def test_from_choices_eos_mode_prefixes_and_groups():
    V, EOS = 70, [68, 69]
    choices = [[5, 6, 7], [5, 6], [9], [5, 8, 8, 8], [64, 65, 66, 67, 3]]  # [5, 6] is a prefix of [5, 6, 7]
    dfa = TokenDFA.from_choices(choices, V, eos=EOS)
    _consistent(dfa)
    assert dfa.start_states == [0] and dfa.vocab_size == V
    for i, c in enumerate(choices):
        path = _walk(dfa, 0, c)
        assert int(dfa.choice_of(torch.tensor(path[-1]))) == i and bool(dfa.accepting[path[-1]])
        assert all(int(dfa.choice_of(torch.tensor(s))) in (-1, 1) for s in path[:-1])  # (only the prefix choice lies on a path)
        for e in EOS:  # EOS leads to a sink that still names the choice and allows only EOS
            sink = int(dfa.next[path[-1], e])
            assert sink >= 0 and int(dfa.choice_of(torch.tensor(sink))) == i
            assert (dfa.next[sink] != DFA_REJECT).nonzero().flatten().tolist() == EOS and int(dfa.next[sink, e]) == sink
    # the prefix choice still has its continuation; EOS is allowed only in accepting states; a token outside the trie is -1
    after = _walk(dfa, 0, [5, 6])[-1]
    assert int(dfa.next[after, 7]) >= 0 and int(dfa.next[after, 68]) >= 0
    assert int(dfa.next[0, 68]) == DFA_REJECT and int(dfa.next[_walk(dfa, 0, [5])[-1], 69]) == DFA_REJECT
    assert (dfa.next[0] != DFA_REJECT).nonzero().flatten().tolist() == [5, 9, 64]
    assert dfa.choice_of(torch.tensor([-1, dfa.num_states, -2])).tolist() == [-1, -1, -1]
    # nested groups: one table, separate start states, indices within the group; tensors as choices
    groups = [[[1, 2], [3]], [torch.tensor([3, 4]), [1], [2, 2]]]
    g = TokenDFA.from_choices(groups, V, eos=69)
    _consistent(g)
    assert len(g.start_states) == 2 and g.start_states[0] != g.start_states[1]
    for gi, grp in enumerate(groups):
        for i, c in enumerate(grp):
            c = c.tolist() if isinstance(c, torch.Tensor) else c
            assert int(g.choice_of(torch.tensor(_walk(g, g.start_states[gi], c)[-1]))) == i
    assert int(g.next[g.start_states[0], 2]) == DFA_REJECT and int(g.next[g.start_states[1], 2]) >= 0  # the groups do not mix
    # .to keeps both tensors and what the constructor remembered
    moved = dfa.to("cpu")
    assert torch.equal(moved.next, dfa.next) and torch.equal(moved.allowed, dfa.allowed) and moved.start_states == [0]
    assert moved.choice_of(torch.tensor([after])).tolist() == [1]
    for bad in ([], [[]], [[1], [1]], [[V]], [[-1]]):
        with pytest.raises(ValueError):
            TokenDFA.from_choices(bad, V, eos=EOS)
    with pytest.raises(ValueError, match="eos"):
        TokenDFA.from_choices([[1]], V, eos=[V])
    with pytest.raises(ValueError, match="on_accept"):
        TokenDFA.from_choices([[1]], V, on_accept="stop")


def test_from_choices_free_mode():
    V = 40
    choices = [[5, 6, 7], [9], [5, 8]]
    dfa = TokenDFA.from_choices(choices, V, on_accept="free")
    _consistent(dfa)
    for c in choices:
        path = _walk(dfa, 0, c)
        assert path[-1] == DFA_FREE and all(0 <= s < dfa.num_states for s in path[:-1])  # the last token frees the row
    assert int(dfa.next[0, 6]) == DFA_REJECT
    # the definition: a freed row is unconstrained and stays where it is
    st = sampling.advance_state(dfa, torch.tensor([0, 0], dtype=torch.int32), torch.tensor([9, 5]))
    assert st[0] == DFA_FREE and 0 <= st[1] < dfa.num_states
    assert sampling.advance_state(dfa, st, torch.tensor([3, 8])).tolist() == [DFA_FREE, DFA_FREE]
    assert dfa.choice_of(st).tolist()[0] == -1


def test_table_size_limit_and_value_range():
    assert table_bytes(8, 128256) == 8 * 128256 * 4 + 8 * 4008 * 4
    with pytest.raises(ValueError, match=r"4\.125"):
        TokenDFA(torch.zeros((4, 1000), dtype=torch.int32), max_table_bytes=16000)
    with pytest.raises(ValueError, match=str(table_bytes(3, 1000))):
        TokenDFA.from_choices([[1, 2]], 1000, max_table_bytes=10000)
    TokenDFA(torch.zeros((4, 1000), dtype=torch.int32), max_table_bytes=table_bytes(4, 1000))
    for bad in (torch.full((2, 5), 2), torch.full((2, 5), -3), torch.zeros(5), torch.zeros((2, 5))):
        with pytest.raises(ValueError):
            TokenDFA(bad)
    with pytest.raises(ValueError):
        TokenDFA(torch.zeros((2, 5), dtype=torch.int32), accepting=torch.ones(3))


# ---- automata from regular expressions, against Python's re ---------------------------------------------------------------------
PATTERNS = [r"(yes|no|maybe)", r"-?(0|[1-9][0-9]{0,3})(\.[0-9]{1,2})?", r'"[a-z ]*"', r'\{"a": (true|false), "n": [0-9]+\}', r"(ab)*c?",
            r'[^"\\]+', r"[A-D]"]


def _vocab():
    """All 256 single bytes, ~500 random printable strings of 2 to 6 bytes (half of them cut from strings the patterns match, so
    that long tokens are allowed somewhere), and a few None / empty tokens."""
    rng = random.Random(7)
    seeds = ["yes", "no", "maybe", "-1234.56", "907.5", '"hello world"', '{"a": true, "n": 1234567}', '{"a": false, "n": 0}', "ababababc",
             "ABCD", "some words, and more!"]
    vocab = [bytes([i]) for i in range(256)]
    for k in range(500):
        L = rng.randint(2, 6)
        if k % 2:
            s = rng.choice(seeds)
            i = rng.randrange(max(len(s) - L, 0) + 1)
            vocab.append(s[i : i + L].encode())
        else:
            vocab.append(bytes(rng.randint(32, 126) for _ in range(L)))
    vocab += [None, b"", None]
    return vocab


VOCAB = _vocab()
EOS_ID = len(VOCAB) - 1  # (a None token: EOS carries no bytes)


def _accepts(dfa, tokens):
    """Does the token sequence lead to an accepting state (an "eos"-mode automaton without using EOS)?"""
    s = 0
    for t in tokens:
        s = int(dfa.next[s, t])
        if s < 0:
            return False
    return bool(dfa.accepting[s])


def _tokenise(data: bytes, rng):
    """A random tokenisation of `data` over VOCAB (single bytes make every position reachable)."""
    by_bytes = _tokenise.index
    out, i = [], 0
    while i < len(data):
        cands = [by_bytes[data[i : i + L]] for L in range(1, 7) if data[i : i + L] in by_bytes and i + L <= len(data)]
        t = rng.choice(cands)
        out.append(t)
        i += len(VOCAB[t])
    return out


_tokenise.index = {}
for _i, _b in enumerate(VOCAB):
    if _b:
        _tokenise.index.setdefault(_b, _i)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_from_regex_against_re(pattern):
    dfa = TokenDFA.from_regex(pattern, VOCAB, eos=[EOS_ID])
    _consistent(dfa)
    full = re.compile(pattern.encode())
    rng = random.Random(len(pattern))
    allowed = dfa.next != DFA_REJECT
    allowed[:, EOS_ID] = False  # the walks stay inside the pattern
    for none in (len(VOCAB) - 3, len(VOCAB) - 2):
        assert not allowed[:, none].any()  # a token without bytes is never allowed
    matched = set()
    for _ in range(200):
        s, data = 0, b""
        for _ in range(64):
            if dfa.accepting[s]:
                assert full.fullmatch(data), (pattern, data)
                matched.add(data)
            ok = allowed[s].nonzero().flatten().tolist()
            if not ok:
                assert dfa.accepting[s], (pattern, data)  # never stuck before the output is complete
                break
            t = rng.choice(ok)
            s = int(dfa.next[s, t])
            data += VOCAB[t]
            assert 0 <= s < dfa.num_states
        # EOS exactly in accepting states
        assert (int(dfa.next[s, EOS_ID]) != DFA_REJECT) == bool(dfa.accepting[s])
    assert matched
    for data in sorted(matched)[:40]:
        for _ in range(3):  # any tokenisation of a matching string is accepted
            assert _accepts(dfa, _tokenise(data, rng)), (pattern, data)
        if data:  # one byte mutated: accepted iff re matches
            i = rng.randrange(len(data))
            mutated = data[:i] + bytes([rng.choice(b'0a."-{ }Zb\\\n')]) + data[i + 1 :]
            assert _accepts(dfa, _tokenise(mutated, rng)) == bool(full.fullmatch(mutated)), (pattern, mutated)
        longer = data + bytes([rng.choice(b"0ab c9")])
        assert _accepts(dfa, _tokenise(longer, rng)) == bool(full.fullmatch(longer)), (pattern, longer)


def test_from_regex_free_mode_classes_and_unsupported_syntax():
    vocab = [bytes([i]) for i in range(256)]
    free = TokenDFA.from_regex(r"[0-9]{2}", vocab, on_accept="free")
    assert int(free.next[0, ord("7")]) >= 0 and int(free.next[int(free.next[0, ord("7")]), ord("1")]) == DFA_FREE
    assert int(free.next[0, ord("a")]) == DFA_REJECT
    # escapes, the dot, UTF-8 literals, counted repetition, against re
    for pattern, yes, no in [(r"\d+\s\w*", [b"12 ab_9", b"7\t"], [b"12", b"a 1", b"1  "]), (r".{2,3}", [b"ab", b"abc"], [b"a", b"abcd", b"a\n"]),
                             ("é+", ["éé".encode()], [b"\xc3", b"e"]), (r"(?:a|bc){2,}", [b"abc", b"bcbca"], [b"a", b"bcb"]),
                             (r"a\.\*\\", [b"a.*\\"], [b"ab*\\"]), (r"[\d\-x]\n\t", [b"-\n\t", b"5\n\t"], [b"y\n\t"])]:
        trans, acc = regex_to_byte_dfa(pattern)

        def match(data):
            s = 0
            for b in data:
                s = int(trans[s, b])
                if s < 0:
                    return False
            return bool(acc[s])

        for d in yes + no:
            # (re on str: a quantifier behind a UTF-8 literal repeats the character, not its last byte)
            assert match(d) == (d in yes) == bool(re.fullmatch(pattern, d.decode("utf-8", "surrogateescape"))), (pattern, d)
    for bad, word in [(r"^a", "anchor"), (r"a$", "anchor"), (r"(?=a)b", "group extension"), (r"a*?", "lazy"), (r"\bword", r"\\b"), (r"(a)\1", r"\\1"),
                      (r"\D", r"\\D"), (r"[[:alpha:]]", "POSIX"), (r"a{2,1}", "bounds"), (r"(a", r"\)"), (r"a)", "unbalanced"), (r"*a", "quantifier"),
                      (r"[é]", "non-ASCII"), (r"[a", "class"), ("a\\", "backslash")]:
        with pytest.raises(ValueError, match=word):
            TokenDFA.from_regex(bad, vocab)

# ---- the torch definition on CPU ---------------------------------------------------------------------------------------------
def _five_state_table(V=70):
    """5 states over 70 tokens (a last partial word): 0 allows {3 -> 1, 69 -> 2, 40 -> FREE}, 1 allows everything -> 1, 2 rejects
    everything, 3 allows the odd tokens -> 4, 4 allows {0 -> 0}."""
    nxt = torch.full((5, V), DFA_REJECT, dtype=torch.int32)
    nxt[0, 3], nxt[0, 69], nxt[0, 40] = 1, 2, DFA_FREE
    nxt[1, :] = 1
    nxt[3, 1::2] = 4
    nxt[4, 0] = 0
    return TokenDFA(nxt)


def test_torch_definition_on_cpu():
    dfa = _five_state_table()
    V = dfa.vocab_size
    g = torch.Generator().manual_seed(3)
    state = torch.tensor([0, 1, 2, 3, 4, -1, 5, DFA_FREE], dtype=torch.int32)
    logits = torch.randn(8, V, generator=g)
    x = sampling.constrain_logits(logits, dfa, state)
    want = torch.zeros(8, V, dtype=torch.bool)
    want[0, [3, 69, 40]] = True
    want[1] = True
    want[3, 1::2] = True
    want[4, 0] = True
    want[5:] = True  # states -1, S and FREE: unconstrained
    assert torch.equal(x == -math.inf, ~want) and torch.equal(x[want], logits[want]) and x.dtype == logits.dtype
    # bits past n are irrelevant: poison them
    poisoned = TokenDFA(dfa.next)
    poisoned.allowed = dfa.allowed.clone()
    poisoned.allowed[:, -1] |= torch.tensor(-(1 << (V % 32)), dtype=torch.int32)  # bits V % 32 .. 31 of the last word
    assert not torch.equal(poisoned.allowed, dfa.allowed) and torch.equal(sampling.constrain_logits(logits, poisoned, state), x)
    tok = torch.tensor([40, 9, 0, 5, 0, 7, 7, 7])
    drawn = torch.tensor([True, True, False, True, True, True, True, True])
    assert sampling.advance_state(dfa, state, tok, drawn).tolist() == [DFA_FREE, 1, 2, 4, 0, -1, 5, DFA_FREE]
    assert sampling.advance_state(dfa, state, tok[:, None]).tolist() == [DFA_FREE, 1, -1, 4, 0, -1, 5, DFA_FREE]  # (every row drew: REJECT)
    # the operator on CPU logits: greedy under the mask, log-probs of the constrained distribution, the state advances in place
    st = state.clone()
    t, lp = layer_ops.sample_tokens(logits, 0.0, return_logprobs=True, constraint=(dfa, st, True))
    assert torch.equal(t[:, 0] * drawn, x.argmax(-1) * drawn) and int(t[2]) == 0 and torch.isnan(lp[2]).all()
    ref = torch.log_softmax(x.double(), -1).gather(1, t)[:, 0]
    assert (lp[drawn, 0].double() - ref[drawn]).abs().max() < 1e-6
    assert st.tolist() == sampling.advance_state(dfa, state, t, drawn).tolist() and st[2] == 2
    st2 = state.clone()
    layer_ops.sample_tokens(logits, 1.0, top_k=3, constraint=(dfa, st2, False))
    assert torch.equal(st2, state)  # advance off: untouched
    hot = layer_ops.sample_tokens(logits.repeat(64, 1), 1.0, constraint=(dfa, state.repeat(64), False))
    assert want.repeat(64, 1).gather(1, hot)[drawn.repeat(64)].all()  # never a token that is not allowed
    # host validation
    sampling.check_constraint(dfa, V, 8)
    with pytest.raises(ValueError, match="tokens"):
        sampling.check_constraint(dfa, V + 1, 8)
    with pytest.raises(ValueError, match="state"):
        sampling.check_constraint(dfa, V, 8, state[:7])
    with pytest.raises(ValueError, match="state"):
        sampling.check_constraint(dfa, V, 8, state.long())


def test_generate_refuses_bad_constraint_arguments():
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                      vocab_size=64, max_position_embeddings=64, rms_norm_eps=1e-5)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.float32, device="cpu", seed=0)
    m.setup_caches(max_unique_batch_size=2, max_unique_seq_length=16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[16])
    dfa = TokenDFA.from_choices([[1, 2], [3]], 64, eos=[0])
    kw = dict(input_ids=torch.arange(1, 9)[None], num_return_sequences=2, max_new_tokens=3, temperature=0.0)
    with pytest.raises(ValueError, match="token_overrides"):
        m.generate(constraint=dfa, token_overrides=torch.zeros((2, 3), dtype=torch.long), **kw)
    with pytest.raises(ValueError, match="constraint"):
        m.generate(constraint_state=torch.zeros(2, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="constraint"):
        m.generate(return_constraint_state=True, **kw)
    with pytest.raises(ValueError, match="64"):
        m.generate(constraint=TokenDFA.from_choices([[1]], 65), **kw)


# ---- the new kernels' registers and LDS ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")
def test_constrain_kernels_have_no_scratch_and_keep_two_rows_per_cu():
    """Read from the assembly's metadata the way tests/test_build_quality.py reads it (the same per-session compile): six kernels,
    nothing spilled, no scratch; the penalised-and-constrained instantiations keep the penalty kernel's two workgroups per CU:
    <= 80 KB of the CU's 160 KB LDS and <= 64 VGPRs (1024 threads = 4 waves per SIMD per workgroup)."""
    from tests.test_build_quality import _device_asm, _metadata

    _, kernels = _metadata("sample_constrain.hip")
    plain = [k for k in kernels if "sample_constrain_kernel" in k["name"]]
    pen = [k for k in kernels if "sample_constrain_penalty_kernel" in k["name"]]
    assert len(plain) == 3 and len(pen) == 3 and len(kernels) == 6, [k["name"] for k in kernels]
    for k in kernels:
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
    lds = {}
    for blk in _device_asm("sample_constrain.hip").split("  - .agpr_count:")[1:]:
        lds[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    for k in pen:
        assert lds[k["name"]] <= 80 * 1024 and k["vgpr"] <= 64, (k, lds[k["name"]])
    for k in plain:
        assert lds[k["name"]] <= 4096, (k, lds[k["name"]])  # sample_filter.hip's histogram and reduction slots, no staging buffer
