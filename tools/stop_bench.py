#!/usr/bin/env python3
"""What retiring finished rows gives back, and what deciding the stop conditions on the device costs.

    python tools/stop_bench.py [--model llama2-7b] [--batch 1024] [--prefix 2048] [--lens 64,256] [--fractions 0,25,50,75,95]

Part 1 -- the decode step (graph replay of the decoder stack + lm_head, the setup of tools/bench_model.py: one shared prompt of
--prefix tokens, --batch sequences) with a fraction of the rows finished.  Every live row sits at unique length S (its cache
index is S - 1: the suffix pass streams S keys of it); a finished row is fed either the same position (retire off: what a loop
without hyd_stop_update's position feed pays, and at 0 % the parent's step) or position shared_len - 1 (retire on: the RoPE +
append kernel skips it and the suffix pass sees length 0).  retire on / off alternate inside one process; the figure is the
median over --reps windows of --steps steps, device events around each window.  The finished rows are a random subset.

Part 2 -- per decode step, hyd_stop_update (one launch, no synchronisation) next to the torch ops + host synchronisation it
replaces on the single-EOS path (`done | (nxt == eos)`, `bool(done.all())`), both on an otherwise idle queue: host wall time per
iteration.  The old path's real cost is larger than this figure: its synchronisation also drains the launch queue every step.

Part 3 -- what the host's poll costs: generate() on the stop path (a stop sequence that never occurs, so every call runs all
--new-tokens steps) with stop_poll_steps = 8 against a period longer than the generation (no copy, no wait), alternating in one
process: wall time per generated token, prefill included in both.

--parts picks among them.  Prints one JSON line per measurement."""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from hydragen_amd import layer_ops, stopping
from hydragen_amd.llama import AttentionMode, HydragenLlamaForCausalLM, LlamaConfig

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama2-7b")
ap.add_argument("--layers", type=int, default=0, help="override the layer count (0 = architecture's own)")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--prefix", type=int, default=2048)
ap.add_argument("--lens", default="64,256", help="unique lengths S the caches are grown to")
ap.add_argument("--fractions", default="0,25,50,75,95", help="percent of the rows finished")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--parts", default="1,2,3")
ap.add_argument("--new-tokens", type=int, default=64, help="part 3: tokens per generate() call")
ap.add_argument("--kv-dtype", default="bf16", help="bf16 or fp8")
a = ap.parse_args()

assert torch.cuda.is_available(), "stop_bench.py measures on the GPU: there is no CPU figure"
dev = "cuda:0"
lens = [int(x) for x in a.lens.split(",")]
parts = {int(x) for x in a.parts.split(",")}
cfg = LlamaConfig.llama2_7b() if a.model == "llama2-7b" else LlamaConfig.llama3_70b()
if a.layers:
    cfg.num_hidden_layers = a.layers
cfg.max_position_embeddings = max(cfg.max_position_embeddings, a.prefix + max(lens) + 16)
model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=dev, seed=0)
model.graph(True)
B, P = a.batch, a.prefix
model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=max(max(lens) + 16, a.new_tokens + 1), max_shared_batch_sizes=[1],
                   max_shared_seq_lengths=[P], kv_cache_dtype=torch.float8_e4m3fn if a.kv_dtype == "fp8" else None)
torch.manual_seed(0)
model.empty_shared_cache()
model.append_shared(torch.randint(1, cfg.vocab_size, (1, P), device=dev))
model.set_mode(AttentionMode.DECODE)
ids = torch.randint(1, cfg.vocab_size, (B, 1), device=dev)
perm = torch.randperm(B, device=dev)


def positions(S, percent, retire):
    pos = torch.full((B, 1), P + S - 1, dtype=torch.int64, device=dev)
    if retire:
        pos[perm[: B * percent // 100]] = P - 1
    return pos


def window(pos):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        model(input_ids=ids, position_ids=pos, use_graph=True, raw_logits=True)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.steps


def part1():
    for S in lens:
        for percent in [int(x) for x in a.fractions.split(",")]:
            pos = {r: positions(S, percent, r) for r in (True, False)}
            for r in (True, False):
                window(pos[r])  # warm-up (graph capture on the first call)
            ms = {True: [], False: []}
            for _ in range(a.reps):
                for r in (True, False):
                    ms[r].append(window(pos[r]))
            on, off = statistics.median(ms[True]), statistics.median(ms[False])
            print(json.dumps({"part": "step", "model": a.model, "layers": cfg.num_hidden_layers, "batch": B, "prefix": P, "kv_dtype": a.kv_dtype,
                              "unique_len": S, "finished_percent": percent, "ms_per_step_retire_off": round(off, 4),
                              "ms_per_step_retire_on": round(on, 4), "saved_percent": round(100 * (off - on) / off, 2),
                              "spread_off_ms": [round(min(ms[False]), 4), round(max(ms[False]), 4)],
                              "spread_on_ms": [round(min(ms[True]), 4), round(max(ms[True]), 4)], "steps": a.steps, "reps": a.reps}), flush=True)


def part2():
    n = 200
    tok = torch.randint(1, cfg.vocab_size, (B, 1), device=dev)
    spec = stopping.check_stop([2, 3], [[5, 6], [7, 8, 9], [10], [11, 12, 13, 14]], 0, False, cfg.vocab_size)
    state = stopping.new_state(B, n, spec, dev)
    start = torch.full((B,), P, dtype=torch.int64, device=dev)
    shared = torch.full((B,), P, dtype=torch.int64, device=dev)
    table = spec.stop_table(dev)[0]
    wall = {"hyd_stop_update": [], "torch_done_all_sync": []}
    for rep in range(a.reps + 1):
        for x in state[1:]:
            x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(n):
            layer_ops.stop_update(tok, t, spec, *state, start, shared, True, table)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        done = torch.zeros((B, 1), dtype=torch.bool, device=dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for t in range(n):
            done = done | (tok == 2)
            if bool(done.all()):
                break
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if rep:  # (the first pass warms both up)
            wall["hyd_stop_update"].append((t1 - t0) / n * 1e6)
            wall["torch_done_all_sync"].append((t3 - t2) / n * 1e6)
    print(json.dumps({"part": "stop_cost", "batch": B, "iterations": n, "eos_ids": len(spec.eos), "stop_sequences": len(spec.stops),
                      "us_per_step_hyd_stop_update": round(statistics.median(wall["hyd_stop_update"]), 2),
                      "us_per_step_torch_done_all_sync": round(statistics.median(wall["torch_done_all_sync"]), 2),
                      "spread_hyd_us": [round(min(wall["hyd_stop_update"]), 2), round(max(wall["hyd_stop_update"]), 2)],
                      "spread_torch_us": [round(min(wall["torch_done_all_sync"]), 2), round(max(wall["torch_done_all_sync"]), 2)]}), flush=True)


def part3():
    N = a.new_tokens
    prompt = torch.randint(1, cfg.vocab_size, (1, P), device=dev)
    periods = {"poll_8": 8, "no_poll": N + 1}
    ms = {k: [] for k in periods}
    for rep in range(a.reps + 1):
        for name, period in periods.items():
            model.stop_poll_steps = period
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(input_ids=[prompt], num_return_sequences=B, max_new_tokens=N, temperature=0.0,
                                 stop=[[1, 2, 3, 4, 5, 6, 7, 8]], shared_cache_op="wipe")  # (the set-up's level holds the one slot)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert out.shape == (B, N), "a row met the stop sequence: the two settings did not run the same steps"
            if rep:  # (the first pass captures the graph)
                ms[name].append((t1 - t0) / N * 1e3)
    print(json.dumps({"part": "poll_cost", "batch": B, "prefix": P, "new_tokens": N,
                      "ms_per_token_poll_8": round(statistics.median(ms["poll_8"]), 4),
                      "ms_per_token_no_poll": round(statistics.median(ms["no_poll"]), 4),
                      "spread_poll_8_ms": [round(min(ms["poll_8"]), 4), round(max(ms["poll_8"]), 4)],
                      "spread_no_poll_ms": [round(min(ms["no_poll"]), 4), round(max(ms["no_poll"]), 4)], "reps": a.reps}), flush=True)


with torch.no_grad():
    for number, part in ((1, part1), (2, part2), (3, part3)):
        if number in parts:
            part()
