"""Shared by tests/test_spec_stop_penalties.py and tests/test_spec_stop_penalties_gpu.py: whole speculative generations over random
draws -- every step's inputs come from a seeded generator and do not depend on the state, so the torch definition, the
sequential form and the kernel can be driven over THE SAME generations and compared step by step."""
from dataclasses import dataclass

import torch

from hydragen_amd import speculative, stopping

ROWS = 130  # two full waves and a partial one
EOS = (5,)
STOPS = ((4, 1), (1,), (2, 5), (0, 2, 3), (3, 3))
RANGES = {"a": (6, 24), "b": (16, 10)}  # name -> (vocabulary, max_new_tokens)
PAD = 63
GEN_STRIDE = 8  # narrower than either max_new_tokens: the list's clamp is part of every run


def spec(include_stop: bool) -> stopping.StopSpec:
    return stopping.StopSpec(eos=EOS, stops=STOPS, pad=PAD, include_stop=include_stop)


def step_inputs(K: int, vocab: int, max_new: int, seed: int, rows: int = ROWS):
    """Per step: (fed, sampled int64 [rows, T], logprobs f32 [rows, T], step_state_after int32 [rows, T]).  Drafts equal the draw
    before them with probability 0.6; a wrong draft is the draw plus one (mod vocab), so it never equals it.  max_new steps
    cover every generation: a running row emits at least one token per step."""
    g = torch.Generator().manual_seed(seed)
    T = K + 1
    steps = []
    for _ in range(max_new):
        sampled = torch.randint(0, vocab, (rows, T), generator=g)
        right = torch.rand((rows, T), generator=g) < 0.6
        fed = torch.full((rows, T), PAD, dtype=torch.int64)
        fed[:, 1:] = torch.where(right[:, :-1], sampled[:, :-1], (sampled[:, :-1] + 1) % vocab)
        lp = -torch.rand((rows, T), generator=g)
        after = torch.randint(0, 1000, (rows, T), generator=g).to(torch.int32)
        steps.append((fed, sampled, lp, after))
    return steps


@dataclass
class State:
    out: torch.Tensor
    length: torch.Tensor
    reason: torch.Tensor
    stop_index: torch.Tensor
    out_lp: torch.Tensor
    gen: torch.Tensor
    gen_len: torch.Tensor
    state: torch.Tensor
    start_pos: torch.Tensor
    shared_len: torch.Tensor

    def snapshot(self):
        return {k: v.detach().cpu().clone() for k, v in self.__dict__.items()}


def new_state(rows: int, max_new: int, device=None) -> State:
    out, length, reason, stop_index, out_lp = speculative.new_state(rows, max_new, PAD, device, logprobs=True)
    return State(out, length, reason, stop_index, out_lp,
                 torch.full((rows, GEN_STRIDE), -7, dtype=torch.int32, device=device), torch.zeros((rows,), dtype=torch.int32, device=device),
                 torch.full((rows,), -3, dtype=torch.int32, device=device),
                 (torch.arange(rows, dtype=torch.int64) * 3 + 11).to(device), (torch.arange(rows, dtype=torch.int64) % 5 + 2).to(device))


def run(accept, steps, max_new: int, device=None, rows: int = ROWS):
    """Drive `accept(fed, sampled, lp, after, st: State) -> (feed, next_pos, accepted, live int)` over `steps` -> one record per step:
    the state's snapshot and the call's four results (CPU)."""
    st = new_state(rows, max_new, device)
    records = []
    for fed, sampled, lp, after in steps:
        feed, pos, acc, live = accept(fed.to(device), sampled.to(device), lp.to(device), after.to(device), st)
        records.append(dict(st.snapshot(), feed=feed.cpu(), next_pos=pos.cpu(), accepted=acc.cpu(), live=int(live)))
    return records


def reference_accept(spec_, max_new, retire=True):
    def accept(fed, sampled, lp, after, st):
        return speculative.accept_stop_reference(fed, sampled, st.out, st.length, st.reason, st.stop_index, st.start_pos, st.shared_len,
                                                 spec_.eos, spec_.pad, max_new, retire, lp, st.out_lp, stop=spec_, gen=st.gen,
                                                 gen_len=st.gen_len, states=(after, st.state))
    return accept
