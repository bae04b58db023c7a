"""Token matrices and stop conditions shared by tests/test_stopping.py (CPU: the two definitions against each other) and
tests/test_stopping_gpu.py (hyd_stop_update against them).  Tokens come from a vocabulary of 6 so that stops really occur; token 5
is no EOS id and ends no stop sequence, so a planted row of 5s never finishes.  Every case plants the rows its name promises."""
import torch

VOCAB = 6
SAFE = 5
T = 14

# name -> (eos ids, stop sequences, planted row prefixes)
CASES = {
    # two stops that overlap each other: 1 2 1 2 holds both, the one that COMPLETES first finishes the row
    "overlapping": ([4], [[1, 2, 1], [2, 1, 2]], [[5, 1, 2, 1, 2, 5], [5, 2, 1, 2, 1, 5], [1, 2, 5, 1, 2, 1]]),
    # a stop that is a prefix of another, in both list orders: the shorter one always completes first
    "prefix-long-first": ([4], [[1, 2, 3], [1, 2]], [[5, 1, 2, 3, 5], [1, 2, 3]]),
    "prefix-short-first": ([4], [[1, 2], [1, 2, 3]], [[5, 1, 2, 3, 5], [1, 2, 3]]),
    # a stop longer than what has been generated: its tail at the very start is no match (nothing reaches into the prompt)
    "longer-than-generated": ([4], [[0, 1, 2, 3], [3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3]],
                              [[1, 2, 3, 5, 5, 0, 1, 2, 3], [2, 3, 5, 5, 5], [3] * T]),
    # EOS and a stop on the same step: EOS is tested first (the token is kept whatever include_stop says)
    "eos-and-stop-together": ([3, 4], [[2, 3], [4], [1, 1]], [[5, 2, 3, 5], [5, 4, 5], [5, 1, 1, 5]]),
    # several stops complete on the same step: the lowest k wins
    "lowest-k": ([4], [[2, 1], [1], [0, 2, 1], [5, 0, 2, 1]], [[5, 0, 2, 1, 5], [0, 2, 1], [5, 5, 1]]),
    # several EOS ids next to one long-ish stop
    "many-eos": ([0, 3], [[1, 1, 1, 1]], [[5, 5, 3], [0], [5, 1, 1, 1, 1]]),
}


def tokens(name, rows, seed=0, steps=T):
    """int64 [rows, steps] CPU: random rows over the small vocabulary, the case's planted rows (padded with SAFE) and one row
    of SAFE only, cycled through in this order when rows is small."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, name)))
    tok = torch.randint(0, VOCAB, (rows, steps), generator=g)
    planted = [p[:steps] + [SAFE] * (steps - len(p)) for p in CASES[name][2]] + [[SAFE] * steps]
    for i, p in enumerate(planted):
        if i < rows:
            tok[rows - 1 - i] = torch.tensor(p)
    return tok


def spec(name, include_stop, pad=None):
    from hydragen_amd import stopping

    eos, stops, _ = CASES[name]
    return stopping.check_stop(eos, stops, SAFE if pad is None else pad, include_stop, VOCAB)
