"""Token automata for constrained decoding: the tables `hyd_sample_tokens_constrained` (csrc/sample_constrain.hip) reads, built on
the host.  hydragen_amd/sampling.py states what a table means; this module makes them from

  * a list of allowed token-id sequences (`TokenDFA.from_choices`: multiple choice, classification labels), and
  * a regular expression over the tokens' BYTES (`TokenDFA.from_regex`: a number, a JSON fragment, a tool-call skeleton).

A table is dense, int32 [states, vocabulary] plus one bit per entry: S * n * 4.125 bytes.  Sparse or compressed tables, grammars
beyond regular languages and tokenizer handling (which bytes a token id stands for is the caller's knowledge) are out of scope."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .sampling import DFA_FREE, DFA_REJECT

MAX_TABLE_BYTES = 4 << 30


def table_bytes(states: int, n: int) -> int:
    """Bytes of the two tensors of an automaton: next (4 per entry) and allowed (1 bit per entry, rows padded to 32 tokens)."""
    return states * n * 4 + states * ((n + 31) // 32) * 4


def pack_allowed(nxt: Tensor) -> Tensor:
    """next int32 [S, n] -> allowed int32 [S, ceil(n / 32)]: bit v % 32 of word v // 32 is set iff next[s, v] != DFA_REJECT."""
    S, n = nxt.shape
    words = (n + 31) // 32
    ok = torch.zeros((S, words * 32), dtype=torch.int64, device=nxt.device)
    ok[:, :n] = (nxt != DFA_REJECT).long()
    weights = torch.ones(32, dtype=torch.int64, device=nxt.device) << torch.arange(32, device=nxt.device)
    packed = (ok.reshape(S, words, 32) * weights).sum(-1)
    return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)


def forced_tokens_reference(allowed: Tensor, n: int) -> Tensor:
    """The rule hyd_dfa_forced_tokens implements, in numpy -> forced int32 [S] on the CPU: forced[s] = the token of the ONE bit
    at a position below n in row s of allowed (int32 [S, >= ceil(n / 32)] words, pack_allowed's layout), -1 for a row with no
    such bit or with two and more.  Bits at positions >= n and words past ceil(n / 32) do not count."""
    a = np.ascontiguousarray(allowed.detach().cpu().numpy())
    if a.ndim != 2 or a.dtype != np.int32 or n <= 0 or a.shape[1] < (n + 31) // 32:
        raise ValueError(f"allowed must be int32 [S, >= ceil(n / 32) = {(n + 31) // 32}] with n > 0, got {a.shape} {a.dtype}, n = {n}")
    S, words = a.shape[0], (n + 31) // 32
    forced = np.full(S, -1, dtype=np.int32)
    rows = max(1, (64 << 20) // (words * 32))  # (rows unpacked at a time: one byte per bit)
    for r in range(0, S, rows):
        w = np.ascontiguousarray(a[r : r + rows, :words]).astype("<u4").view(np.uint8)
        bits = np.unpackbits(w, axis=1, bitorder="little")[:, :n]
        forced[r : r + rows] = np.where(bits.sum(1) == 1, bits.argmax(1), -1)
    return torch.from_numpy(forced)


def forced_tokens(allowed: Tensor, n: int) -> Tensor:
    """hyd_dfa_forced_tokens, one launch -> forced int32 [S] on allowed's device; CPU tensors take forced_tokens_reference.
    allowed int32 [S, stride >= ceil(n / 32)] with a unit last stride (a row stride wider than the row is honoured)."""
    if allowed.device.type != "cuda":
        return forced_tokens_reference(allowed, n)
    import ctypes as C

    from . import _lib

    if allowed.ndim != 2 or allowed.dtype != torch.int32 or allowed.stride(1) != 1 or n <= 0 or allowed.shape[1] < (n + 31) // 32:
        raise ValueError(f"allowed must be int32 [S, >= ceil(n / 32)] with a unit last stride, got {tuple(allowed.shape)} {allowed.dtype}")
    S = allowed.shape[0]
    forced = torch.empty((S,), dtype=torch.int32, device=allowed.device)
    p = _lib.DfaForcedParams()
    p.allowed, p.forced, p.allowed_stride = allowed.data_ptr(), forced.data_ptr(), allowed.stride(0) if S > 1 else allowed.shape[1]
    p.n_states, p.n = S, n
    with torch.cuda.device(allowed.device):
        _lib.check(_lib.load().hyd_dfa_forced_tokens(C.byref(p), torch.cuda.current_stream().cuda_stream))
    return forced


class TokenDFA:
    """A token automaton: next int32 [S, n] (>= 0: the next state, DFA_REJECT, DFA_FREE) and the bitmap allowed int32
    [S, ceil(n / 32)] derived from it once.  accepting: bool [S] or None (all False): the states in which the output so far is
    complete.  meta: whatever the constructor wants to remember (from_choices keeps the choice of every state).
    start_states: the entry states (one per group of choices; [0] otherwise).  forced int32 [S]: the one token a state
    allows, or -1 (speculative decoding's certain drafts), made from the bitmap on first use and kept."""

    def __init__(self, next: Tensor, accepting: Optional[Tensor] = None, meta: Optional[dict] = None,
                 max_table_bytes: int = MAX_TABLE_BYTES, _allowed: Optional[Tensor] = None, _forced: Optional[Tensor] = None):
        nxt = torch.as_tensor(next)
        if nxt.ndim != 2 or nxt.shape[0] <= 0 or nxt.shape[1] <= 0:
            raise ValueError(f"next must be [S, n] with S, n > 0, got {tuple(nxt.shape)}")
        if nxt.dtype.is_floating_point or nxt.dtype == torch.bool:
            raise ValueError(f"next must hold integers, got {nxt.dtype}")
        S, n = nxt.shape
        size = table_bytes(S, n)
        if size > max_table_bytes:
            raise ValueError(f"a table of {S} states x {n} tokens takes {size} bytes (S * n * 4.125), more than max_table_bytes = "
                             f"{max_table_bytes}: sparse tables are not supported")
        if _allowed is None and (int(nxt.min()) < DFA_FREE or int(nxt.max()) >= S):
            raise ValueError(f"next entries must be in [0, {S}), DFA_REJECT ({DFA_REJECT}) or DFA_FREE ({DFA_FREE}); found "
                             f"{int(nxt.min())} .. {int(nxt.max())}")
        self.next = nxt.to(torch.int32).contiguous()
        self.allowed = pack_allowed(self.next) if _allowed is None else _allowed
        self._forced = _forced
        if accepting is None:
            accepting = torch.zeros(S, dtype=torch.bool)
        accepting = torch.as_tensor(accepting).bool().reshape(-1)
        if accepting.shape[0] != S:
            raise ValueError(f"accepting must hold {S} flags, got {accepting.shape[0]}")
        self.accepting = accepting.cpu()
        self.meta = dict(meta or {})
        self.start_states = list(self.meta.get("start_states", [0]))
        self.max_table_bytes = max_table_bytes

    num_states = property(lambda self: self.next.shape[0])
    vocab_size = property(lambda self: self.next.shape[1])
    device = property(lambda self: self.next.device)

    @property
    def forced(self) -> Tensor:
        """int32 [S] on the automaton's device: the token of a state that allows exactly one, else -1 (hyd_dfa_forced_tokens on
        the GPU, forced_tokens_reference on the CPU; computed once)."""
        if self._forced is None:
            self._forced = forced_tokens(self.allowed, self.vocab_size)
        return self._forced

    def to(self, device) -> "TokenDFA":
        """The same automaton with its tensors on `device` (the bitmap, and forced once it exists, are copied, not rebuilt)."""
        return TokenDFA(self.next.to(device), self.accepting, self.meta, self.max_table_bytes, _allowed=self.allowed.to(device),
                        _forced=None if self._forced is None else self._forced.to(device))

    def choice_of(self, states) -> Tensor:
        """from_choices automata: for every state, the index (within its group) of the choice that has been completed there --
        the state behind a choice's last token, or the sink behind its EOS -- else -1 (unconstrained states included: with
        on_accept="free" a finished row is in no state at all).  int64, on the states' device."""
        table = self.meta.get("choice_of_state")
        if table is None:
            raise ValueError("choice_of needs an automaton made by TokenDFA.from_choices")
        st = torch.as_tensor(states).long()
        t = torch.as_tensor(table, dtype=torch.int64, device=st.device)
        on = (st >= 0) & (st < t.shape[0])
        return torch.where(on, t[torch.where(on, st, torch.zeros_like(st))], torch.full_like(st, -1))

    # ---- constructors ----------------------------------------------------------------------------------------------------
    @classmethod
    def _finish(cls, core: np.ndarray, accepting: np.ndarray, eos, on_accept: str, meta: dict, max_table_bytes: int) -> "TokenDFA":
        """core int32 [S, n] over {>= 0, DFA_REJECT} with its accepting flags -> the automaton for on_accept.
        "eos": every accepting state also allows the EOS ids, which lead to a sink of its own where only they are allowed (a row
        that has finished keeps emitting EOS: generate(eos_token_id=[...]) ends it through the stop kernel; no EOS ids: an
        accepting state without continuations allows nothing).  "free": a token that completes the output leads to DFA_FREE."""
        if on_accept not in ("eos", "free"):
            raise ValueError(f'on_accept must be "eos" or "free", got {on_accept!r}')
        S, n = core.shape
        eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
        if any(e < 0 or e >= n for e in eos):
            raise ValueError(f"eos ids {eos} must be in [0, {n})")
        origin = np.arange(S)
        if on_accept == "free":
            hit = (core >= 0) & accepting[np.maximum(core, 0)]
            nxt = np.where(hit, DFA_FREE, core).astype(np.int32)
            acc = accepting
        else:
            # one sink per accepting state where the state says which choice was made (choice_of), else one for all
            acc_states = np.flatnonzero(accepting)
            per_state = "choice_of_state" in meta
            k = (len(acc_states) if per_state else min(len(acc_states), 1)) if eos else 0
            if table_bytes(S + k, n) > max_table_bytes:
                raise ValueError(f"a table of {S + k} states x {n} tokens takes {table_bytes(S + k, n)} bytes (S * n * 4.125), more "
                                 f"than max_table_bytes = {max_table_bytes}: sparse tables are not supported")
            nxt = np.full((S + k, n), DFA_REJECT, dtype=np.int32)
            nxt[:S] = core
            acc = np.concatenate([accepting, np.ones(k, dtype=bool)])
            origin = np.concatenate([origin, acc_states[:k]])
            for i, a in enumerate(acc_states if k else []):
                sink = S + (i if per_state else 0)
                nxt[a, eos] = sink
                nxt[sink, eos] = sink
        meta = dict(meta, origin=origin.tolist(), eos=eos, on_accept=on_accept)
        if "choice_of_state" in meta:
            meta["choice_of_state"] = [meta["choice_of_state"][o] for o in origin]
        return cls(torch.from_numpy(nxt), torch.from_numpy(acc), meta, max_table_bytes)

    @classmethod
    def from_choices(cls, choices, vocab_size: int, eos=None, on_accept: str = "eos",
                     max_table_bytes: int = MAX_TABLE_BYTES) -> "TokenDFA":
        """The output must be one of `choices`, token-id sequences (lists, tuples or 1-d tensors, none empty).  A list of LISTS of
        sequences gives one trie per group in one table: start_states[g] is group g's entry state (pass it per row as
        generate(constraint_state=)), and choice_of counts within the group.  A choice that is a prefix of another is accepting and
        still has continuations.  on_accept="eos": after a choice only the EOS ids; "free": the last token of a choice frees the
        row (of two choices where one is a prefix of the other, the shorter then decides: anything may follow it)."""
        def seq(c):
            c = [int(t) for t in (c.tolist() if isinstance(c, Tensor) else c)]
            if not c:
                raise ValueError("a choice must be a non-empty sequence of token ids")
            if any(t < 0 or t >= vocab_size for t in c):
                raise ValueError(f"choice {c} has a token id outside [0, {vocab_size})")
            return c

        choices = list(choices)
        if not choices:
            raise ValueError("no choices")
        first = choices[0].tolist() if isinstance(choices[0], Tensor) else choices[0]
        nested = len(first) > 0 and isinstance(first[0], (list, tuple, Tensor))
        groups = [[seq(c) for c in g] for g in choices] if nested else [[seq(c) for c in choices]]
        if any(not g for g in groups):
            raise ValueError("a group without choices")
        edges, choice, starts = [], [], []  # per state: {token: state}, completed choice or -1
        for g in groups:
            starts.append(len(edges))
            edges.append({})
            choice.append(-1)
            for ci, c in enumerate(g):
                s = starts[-1]
                for t in c:
                    if t not in edges[s]:
                        edges[s][t] = len(edges)
                        edges.append({})
                        choice.append(-1)
                    s = edges[s][t]
                if choice[s] != -1:
                    raise ValueError(f"choice {c} is given twice in its group")
                choice[s] = ci
        S = len(edges)
        if table_bytes(S, vocab_size) > max_table_bytes:
            raise ValueError(f"a table of {S} states x {vocab_size} tokens takes {table_bytes(S, vocab_size)} bytes (S * n * 4.125), "
                             f"more than max_table_bytes = {max_table_bytes}: sparse tables are not supported")
        core = np.full((S, vocab_size), DFA_REJECT, dtype=np.int32)
        for s, e in enumerate(edges):
            if e:
                core[s, list(e.keys())] = list(e.values())
        meta = dict(start_states=starts, choice_of_state=choice, groups=groups)
        return cls._finish(core, np.array(choice) >= 0, eos, on_accept, meta, max_table_bytes)

    @classmethod
    def from_regex(cls, pattern: str, vocab_bytes: Sequence, eos=None, on_accept: str = "eos",
                   max_table_bytes: int = MAX_TABLE_BYTES) -> "TokenDFA":
        """The bytes of the whole output must match `pattern`.  vocab_bytes[v]: the bytes token v stands for (bytes; None or empty:
        the token is never allowed).  The pattern is compiled over BYTES: literals are UTF-8 encoded, `.` is any byte but a newline,
        classes are ASCII.  Syntax: literals, \\ escapes of metacharacters, \\d \\w \\s \\n \\t, `.`, [...] and [^...] with ranges,
        groups (...) and (?:...), |, * + ?, {m}, {m,n}, {m,}; anything else raises a ValueError that names it.  Thompson NFA ->
        subset construction -> states that cannot reach acceptance removed -> minimisation; a token is allowed in a state iff
        walking its bytes from there ends in a live state."""
        trans, accepting = regex_to_byte_dfa(pattern)
        Sb = trans.shape[0]
        n = len(vocab_bytes)
        if n == 0:
            raise ValueError("empty vocabulary")
        if table_bytes(Sb, n) > max_table_bytes:
            raise ValueError(f"a table of {Sb} states x {n} tokens takes {table_bytes(Sb, n)} bytes (S * n * 4.125), more than "
                             f"max_table_bytes = {max_table_bytes}: sparse tables are not supported")
        lens = np.array([len(b) if b is not None else 0 for b in vocab_bytes], dtype=np.int64)
        L = int(lens.max()) if n else 0
        tok = np.zeros((n, max(L, 1)), dtype=np.int64)
        for v, b in enumerate(vocab_bytes):
            if b:
                tok[v, : len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        step = np.concatenate([np.where(trans < 0, Sb, trans), np.full((1, 256), Sb, dtype=trans.dtype)])  # state Sb: dead
        cur = np.broadcast_to(np.arange(Sb, dtype=np.int64)[:, None], (Sb, n)).copy()
        for j in range(L):  # byte position by byte position, every (state, token) at once
            live = lens > j
            cur[:, live] = step[cur[:, live], tok[live, j][None, :]]
        cur[:, lens == 0] = Sb
        core = np.where(cur == Sb, DFA_REJECT, cur).astype(np.int32)
        return cls._finish(core, accepting, eos, on_accept, dict(pattern=pattern, start_states=[0]), max_table_bytes)


# ---- regular expressions over bytes -------------------------------------------------------------------------------------------
_META = set("\\.[]()|*+?{}^$")
_DIGIT = frozenset(range(48, 58))
_WORD = frozenset(list(range(48, 58)) + list(range(65, 91)) + list(range(97, 123)) + [95])
_SPACE = frozenset(b" \t\n\r\f\v")
_ANY = frozenset(range(256)) - {10}


class _Parser:
    """pattern -> AST: ("set", frozenset of bytes) | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None)."""

    def __init__(self, pattern: str):
        self.p, self.i = pattern, 0

    def fail(self, what):
        raise ValueError(f"unsupported regular expression syntax in {self.p!r} at {self.i}: {what}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.fail(f"unbalanced {self.p[self.i]!r}")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.peek() is not None and self.peek() not in "|)":
            parts.append(self.repeat())
        return ("cat", parts)

    def repeat(self):
        node = self.atom()
        while self.peek() is not None and self.peek() in "*+?{":
            c = self.peek()
            if c == "{":
                j = self.p.find("}", self.i)
                body = self.p[self.i + 1 : j] if j > 0 else ""
                lo, sep, hi = body.partition(",")
                if j < 0 or not lo.isdigit() or (hi and not hi.isdigit()):
                    self.fail("a repetition {m}, {m,n} or {m,} with decimal bounds")
                m, n = int(lo), (int(lo) if not sep else (int(hi) if hi else None))
                if n is not None and n < m:
                    self.fail(f"repetition bounds {{{body}}}")
                self.i = j + 1
            else:
                m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
                self.i += 1
            if self.peek() is not None and self.peek() in "?+":
                self.fail(f"lazy or possessive quantifier {c}{self.peek()}")
            node = ("rep", node, m, n)
        return node

    def escape(self, in_class: bool):
        self.i += 1
        c = self.peek()
        if c is None:
            self.fail("a trailing backslash")
        self.i += 1
        if c == "d":
            return _DIGIT
        if c == "w":
            return _WORD
        if c == "s":
            return _SPACE
        if c == "n":
            return frozenset([10])
        if c == "t":
            return frozenset([9])
        if ord(c) < 128 and not c.isalnum():  # (every metacharacter, and what Python's re also takes as a literal)
            return frozenset([ord(c)])
        self.i -= 2
        self.fail(f"the escape \\{c}")

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i : self.i + 2] != "?:":
                    self.fail(f"the group extension ({self.p[self.i : self.i + 3]}")
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                self.fail("a group without its )")
            self.i += 1
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            self.i += 1
            return ("set", _ANY)
        if c == "\\":
            return ("set", self.escape(False))
        if c in "^$":
            self.fail(f"the anchor {c} (the pattern always matches the whole output)")
        if c in "*+?{":
            self.fail(f"a quantifier {c} with nothing to repeat")
        if c in ")]}":
            self.fail(f"unbalanced {c!r}")
        self.i += 1
        b = c.encode("utf-8")
        return ("set", frozenset(b)) if len(b) == 1 else ("cat", [("set", frozenset([x])) for x in b])

    def char_class(self):
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members, first = set(), True
        while True:
            c = self.peek()
            if c is None:
                self.fail("a class without its ]")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i : self.i + 2] == "[:":
                self.fail("a POSIX class [:name:]")
            if c == "\\":
                lo = self.escape(True)
            else:
                if ord(c) > 127:
                    self.fail(f"the non-ASCII class member {c!r}")
                lo = frozenset([ord(c)])
                self.i += 1
            if self.peek() == "-" and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                if len(lo) != 1:
                    self.fail("a range that starts at a class escape")
                self.i += 1
                c2 = self.peek()
                if c2 == "\\":
                    hi = self.escape(True)
                else:
                    if ord(c2) > 127:
                        self.fail(f"the non-ASCII class member {c2!r}")
                    hi = frozenset([ord(c2)])
                    self.i += 1
                a, b = next(iter(lo)), next(iter(hi))
                if len(hi) != 1 or b < a:
                    self.fail("a reversed or non-literal range")
                members.update(range(a, b + 1))
            else:
                members.update(lo)
        return frozenset(range(256)) - members if negate else frozenset(members)


def regex_to_byte_dfa(pattern: str):
    """-> (trans int32 [S, 256], accepting bool [S]): the minimal byte automaton of `pattern` without dead states (transitions
    into them are -1), start state 0.  A pattern that matches nothing raises."""
    ast = _Parser(pattern).parse()
    # Thompson construction: eps[s] = epsilon successors, arcs[s] = [(byte set, target)]
    eps, arcs = [], []

    def new():
        eps.append([])
        arcs.append([])
        return len(eps) - 1

    def build(node):  # -> (entry, exit)
        kind = node[0]
        if kind == "set":
            a, b = new(), new()
            arcs[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = new()
            for part in node[1]:
                x, y = build(part)
                eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = new(), new()
            for part in node[1]:
                x, y = build(part)
                eps[a].append(x)
                eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = new()
        for _ in range(m):
            x, y = build(sub)
            eps[b].append(x)
            b = y
        if n is None:
            x, y = build(sub)
            end = new()
            eps[b] += [x, end]
            eps[y] += [x, end]
            b = end
        else:
            end = new()
            for _ in range(n - m):
                x, y = build(sub)
                eps[b] += [x, end]
                b = y
            eps[b].append(end)
            b = end
        return a, b

    start, final = build(ast)

    def closure(states):
        seen, stack = set(states), list(states)
        while stack:
            for t in eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    # subset construction
    ids = {closure([start]): 0}
    order = [closure([start])]
    rows = []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = np.full(256, -1, dtype=np.int64)
        by_byte = {}
        for s in cur:
            for bs, t in arcs[s]:
                for byte in bs:
                    by_byte.setdefault(byte, set()).add(t)
        cache = {}
        for byte, targets in by_byte.items():
            key = frozenset(targets)
            if key not in cache:
                c = closure(key)
                if c not in ids:
                    ids[c] = len(order)
                    order.append(c)
                cache[key] = ids[c]
            row[byte] = cache[key]
        rows.append(row)
    trans = np.stack(rows)
    acc = np.array([final in s for s in order])
    S = trans.shape[0]
    # states that cannot reach acceptance become -1
    live = acc.copy()
    while True:
        grown = live | (np.where(trans >= 0, live[np.maximum(trans, 0)], False).any(1))
        if (grown == live).all():
            break
        live = grown
    if not live[0]:
        raise ValueError(f"the regular expression {pattern!r} matches nothing")
    trans = np.where((trans >= 0) & live[np.maximum(trans, 0)], trans, -1)
    # Moore minimisation over the live states (dead = class of its own, label -1)
    keep = np.flatnonzero(live)
    label = np.where(live, acc.astype(np.int64), -1)
    while True:
        sig = np.concatenate([label[:, None], np.where(trans >= 0, label[np.maximum(trans, 0)], -1)], axis=1)[keep]
        _, new_label = np.unique(sig, axis=0, return_inverse=True)
        new_label = new_label.reshape(-1)
        full = np.full(S, -1, dtype=np.int64)
        full[keep] = new_label
        if len(np.unique(new_label)) == len(np.unique(label[keep])):
            label = full
            break
        label = full
    # renumber: the start state's class is 0, the others in order of first appearance
    remap, reps = {}, []
    for s in [0] + [int(x) for x in keep]:
        c = int(label[s])
        if c not in remap:
            remap[c] = len(reps)
            reps.append(s)
    out = np.full((len(reps), 256), -1, dtype=np.int32)
    for c, s in enumerate(reps):
        t = trans[s]
        out[c] = np.where(t >= 0, np.vectorize(lambda x: remap.get(int(label[x]), -1))(np.maximum(t, 0)), -1)
    return out, acc[reps]
