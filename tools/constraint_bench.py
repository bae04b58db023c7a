#!/usr/bin/env python3
"""Time one constrained sampling call over [B, V] logits with HIP events after warm-up, and write profiles/constrained_sampling.md.

    python tools/constraint_bench.py [--batch 1024] [--vocabs 32000,128256] [--states 8,512] [--fractions 0.01,0.5]
                                     [--iters 30] [--warmup 5] [--repeats 3] [--out profiles/constrained_sampling.md]

bf16 logits, T = 0.7, top-p 0.95.  Per (V, states, allowed fraction), three legs, interleaved `--repeats` times in one process:
  floor        hyd_sample_tokens_filtered alone on the same logits: the cost the constraint is measured against;
  constrained  hyd_sample_tokens_constrained (neutral penalties), states advancing: mask, draw and state update in one launch;
  torch        the route without the kernel: gather a bool [B, V] mask from a [S, V] table, masked_fill, the filtered kernel, gather
               the next state from `next`.
The automaton is random: every state allows the given fraction of the vocabulary, every allowed token leads to a random state,
the rows start in random states.  Prints one JSON line per leg; needs a GPU (there is no CPU fallback)."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import torch

from hydragen_amd import layer_ops
from hydragen_amd.constraint import TokenDFA

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--states", default="8,512")
ap.add_argument("--fractions", default="0.01,0.5")
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=str(REPO / "profiles" / "constrained_sampling.md"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("constraint_bench.py measures on a GPU: none found")
dev = "cuda:0"
T, TOP_P = 0.7, 0.95
B = a.batch


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


rows = []
for V in map(int, a.vocabs.split(",")):
    g = torch.Generator(device=dev).manual_seed(B + V)
    x = (torch.randn(B, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    for S in map(int, a.states.split(",")):
        for frac in map(float, a.fractions.split(",")):
            ok = torch.rand(S, V, device=dev, generator=g) < frac
            ok[:, 0] = True  # (no state rejects everything)
            target = torch.randint(0, S, (S, V), device=dev, generator=g, dtype=torch.int32)
            dfa = TokenDFA(torch.where(ok, target, torch.full_like(target, -1)))
            start = torch.randint(0, S, (B,), device=dev, generator=g, dtype=torch.int32)
            state = start.clone()
            tstate = start.long()
            table = dfa.next  # the torch route gathers from the same table

            def floor():
                return layer_ops.sample_tokens_filtered(x, T, top_p=TOP_P)

            def constrained():
                return layer_ops.sample_tokens_constrained(x, T, constraint=(dfa, state, True), top_p=TOP_P)

            def torch_route():
                global tstate
                mask = ok[tstate]
                tok, lp, kept = layer_ops.sample_tokens_filtered(x.masked_fill(~mask, float("-inf")), T, top_p=TOP_P)
                tstate = table[tstate, tok[:, 0]].long()
                return tok, lp, kept

            legs = {"floor": floor, "constrained": constrained, "torch": torch_route}
            got = {k: [] for k in legs}
            for _ in range(a.repeats):  # interleaved: every leg sees the same drift of the machine
                for name, fn in legs.items():
                    got[name].append(round(timed(fn), 1))
            for name in legs:
                print(json.dumps({"B": B, "V": V, "states": S, "allowed": frac, "leg": name, "us_median": got[name], "iters": a.iters}), flush=True)
            rows.append((V, S, frac, got))
            del ok, target, dfa
            torch.cuda.empty_cache()

fmt = lambda v: " / ".join(f"{t:.1f}" for t in v)  # noqa: E731
mid = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
lines = [
    "# Constrained sampling in the sampling launch (`hyd_sample_tokens_constrained`, DESIGN.md §4.16)",
    "",
    f"Method: `tools/constraint_bench.py`, one MI355X ({torch.cuda.get_device_name(0)}), one process, HIP events around one call after "
    f"{a.warmup} warm-up calls, median of {a.iters} calls; the three legs interleaved, {a.repeats} repeats each (all shown).  B = {B}, bf16, "
    f"T = {T}, top-p {TOP_P}.  Random automata: every state allows the given share of the vocabulary, the rows start in random states and "
    "advance with every call.  Microseconds per call.",
    "",
    "* floor: `hyd_sample_tokens_filtered` alone on the same logits.",
    "* constrained: `hyd_sample_tokens_constrained`, neutral penalties (mask, cuts, draw, log-prob and state update in one launch).",
    "* torch: bool `[B, V]` gather from a `[S, V]` table, `masked_fill`, the filtered kernel, gather of `next`.",
    "",
    "| V | states | allowed | floor | constrained | torch | constrained / floor | torch / constrained |",
    "|---|---|---|---|---|---|---|---|",
]
for V, S, frac, got in rows:
    f, c, t = mid(got["floor"]), mid(got["constrained"]), mid(got["torch"])
    lines.append(f"| {V} | {S} | {frac:.0%} | {fmt(got['floor'])} | {fmt(got['constrained'])} | {fmt(got['torch'])} | {c / f:.2f} | {t / c:.2f} |")
lines += ["", "The ratios are between the medians of the repeats.  No ratio was fixed in advance: this is what was measured.", ""]
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines))
print(f"wrote {a.out}")
