"""Speculative decoding under a token automaton on a Llama-2-7B shell (random weights, bf16, P = 2048, graph decode): tokens/s of
generate(constraint=, draft_tokens=K, draft="constraint") -- the drafts are the tokens the automaton forces, accepted by construction
whatever the weights are -- against generate(constraint=) without drafts, in the same process, alternating.  Writes
profiles/constrained_speculative.md (markdown, also to stdout) -- nothing here is promised in advance.

    python tools/constrained_spec_bench.py [--batches 32,128] [--drafts 3,7] [--prefix 2048] [--layers 32] [--reps 3] [--no-graph]

Two automata: a fully forced skeleton of 64 tokens (TokenDFA.from_choices with one choice: every state is forced, so the measured
acceptance must be exactly 1.0) and a from_regex JSON fragment over a byte vocabulary, whose literal pieces are forced and whose
values are not.  Tokens/s counts emitted tokens (EOS included) over the decode time: the call's time minus the time of the same call
with max_new_tokens = 1.  The figures to read a ratio against are the step-cost ratios of profiles/speculative.md."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

DEV = "cuda:0"
JSON = r'\{"name": "[a-z]{3,8}", "age": [1-9][0-9]?, "ok": (true|false)\}'


def automata(vocab, eos):
    from hydragen_amd.constraint import TokenDFA

    skeleton = [(977 * i + 13) % (vocab - 2) + 1 for i in range(64)]
    byte_vocab = [bytes([i]) for i in range(256)] + [None] * (vocab - 256)
    return {
        "forced skeleton (64 tokens)": (TokenDFA.from_choices([skeleton], vocab, eos=[eos]).to(DEV), 65),
        "JSON fragment (from_regex)": (TokenDFA.from_regex(JSON, byte_vocab, eos=[eos]).to(DEV), 48),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--drafts", default="3,7")
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "constrained_speculative.md"))
    args = ap.parse_args()
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig.llama2_7b()
    cfg.num_hidden_layers = args.layers
    cfg.max_position_embeddings = max(cfg.max_position_embeddings, args.prefix + 128)
    model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
    model.graph(not args.no_graph)
    eos = cfg.vocab_size - 1
    prompt = torch.randint(1, cfg.vocab_size - 1, (1, args.prefix), device=DEV)
    lines = ["# Speculative decoding under a token automaton: measurements", "",
             f"Llama-2-7B shell ({args.layers} layers, random weights, bf16), P = {args.prefix}, {'eager' if args.no_graph else 'HIP-graph'} decode, "
             f"temperature 1, best of {args.reps} alternating runs.  Baseline: `generate(constraint=)` without drafts; drafted: "
             '`generate(constraint=, draft_tokens=K, draft="constraint")`.  Acceptance = accepted / proposed drafts.', ""]
    for B in (int(b) for b in args.batches.split(",")):
        model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=96, max_shared_batch_sizes=[1], max_shared_seq_lengths=[args.prefix])
        for name, (dfa, new) in automata(cfg.vocab_size, eos).items():
            n_forced = int((dfa.forced >= 0).sum())

            def run(n, **kw):
                torch.manual_seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=n, temperature=1.0, eos_token_id=[eos],
                                     constraint=dfa, return_finish=True, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            lines += [f"## B = {B}, {name}: {dfa.num_states} states, {n_forced} forced", "",
                      "| K | baseline tokens/s | drafted tokens/s | ratio | steps | proposed | forced | accepted | acceptance |", "|---|---|---|---|---|---|---|---|---|"]
            for K in (int(k) for k in args.drafts.split(",")):
                kw = dict(draft_tokens=K, draft="constraint", return_draft_stats=True)
                run(4), run(4, **kw)
                pre = min(run(1)[0] for _ in range(2))
                base, spec = [], []
                for _ in range(args.reps):  # alternating: both see the same clocks
                    base.append(run(new))
                    spec.append(run(new, **kw))
                tb, (_, fb) = min(base, key=lambda r: r[0])
                ts, (_, fs, st) = min(spec, key=lambda r: r[0])
                rate_b, rate_s = int(fb.lengths.sum()) / (tb - pre), int(fs.lengths.sum()) / (ts - pre)
                prop, forc, acc = int(st.proposed.sum()), int(st.forced.sum()), int(st.accepted.sum())
                lines.append(f"| {K} | {rate_b:.0f} | {rate_s:.0f} | {rate_s / rate_b:.2f} | {st.steps} | {prop} | {forc} | {acc} | "
                             f"{acc / max(prop, 1):.3f} |")
            lines.append("")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
