#!/usr/bin/env python3
"""What a fork costs next to re-prefilling the survivors, and what the promote launch moves.

    python tools/fork_bench.py [--model llama2-7b] [--batch 1024] [--prefix 2048] [--step 64] [--expand 4] [--out profiles/fork.md]

The setup of tools/bench_model.py: one shared prompt of --prefix tokens, --batch completions, graph replay.  A first round
generates --step tokens per completion; one completion in every --expand is then kept (batch / expand survivors, step - 1 cached
tokens each) and continued --expand times for another --step tokens.

Part 1 -- one layer's promote launch (hyd_kv_promote: K and V of the survivors into the next shared level) against
promote_kv_reference (dequantize / index_select / cat / slice assignment in torch, with its host read of the lengths) on the same
caches: device time between events, median over --reps, and the bytes per second the launch moves (2 x k x len x Hkv x D elements
read and written).

Part 2 -- the step from one round to the next, host wall time with a synchronisation at both ends, median over --reps,
alternating in one process: model.fork (every layer's launch + the token bitmap) against append_shared of the survivors' tokens
(the forward pass over tokens whose K/V already sit in the unique caches), and -- once each, for scale -- the round's generate()
that follows.

Writes the table to --out and prints one JSON line per measurement."""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from hydragen_amd.fork import promote_kv, promote_kv_reference
from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama2-7b")
ap.add_argument("--layers", type=int, default=0, help="override the layer count (0 = architecture's own)")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--prefix", type=int, default=2048)
ap.add_argument("--step", type=int, default=64, help="tokens per round")
ap.add_argument("--expand", type=int, default=4, help="children per survivor: batch / expand completions survive")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--kv-dtype", default="bf16", help="bf16 or fp8")
ap.add_argument("--out", default="profiles/fork.md")
a = ap.parse_args()

assert torch.cuda.is_available(), "fork_bench.py measures on the GPU: there is no CPU figure"
dev = "cuda:0"
B, P, T, E = a.batch, a.prefix, a.step, a.expand
assert B % E == 0 and T >= 2
k, L = B // E, T - 1
cfg = LlamaConfig.llama2_7b() if a.model == "llama2-7b" else LlamaConfig.llama3_70b()
if a.layers:
    cfg.num_hidden_layers = a.layers
cfg.max_position_embeddings = max(cfg.max_position_embeddings, P + 2 * T + 16)
model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=dev, seed=0)
model.graph(True)
model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=T + 16, max_shared_batch_sizes=[1, k], max_shared_seq_lengths=[P, T],
                   kv_cache_dtype=torch.float8_e4m3fn if a.kv_dtype == "fp8" else None)
torch.manual_seed(0)
results = []


def emit(**kw):
    results.append(kw)
    print(json.dumps(kw), flush=True)


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


with torch.no_grad():
    prompt = torch.randint(1, cfg.vocab_size, (1, P), device=dev)
    first = dict(input_ids=prompt, num_return_sequences=B, max_new_tokens=T, temperature=1.0, shared_cache_op="wipe")
    tokens = model.generate(**first)  # (captures the graph of the one-level round)
    t_round0 = wall_ms(lambda: model.generate(**first))
    rows = torch.arange(0, B, E, device=dev)
    lens = torch.full((k,), L, dtype=torch.int32, device=dev)
    fed, last = tokens[rows, :L], tokens[rows, L]

    # part 1: one layer
    kv = model.model.layers[0].self_attn.kv_cache
    sc = kv.shared_caches[1]
    args = (kv.per_completion_k_cache, kv.per_completion_v_cache, rows, lens, sc.k_cache, sc.v_cache)
    hkv, d = kv.per_completion_k_cache.shape[2:]
    moved = 2 * k * L * hkv * (d * kv.per_completion_k_cache.element_size() + sc.k_cache.shape[2] * sc.k_cache.element_size())
    ms = {"kernel": [], "torch": []}
    for rep in range(a.reps + 1):
        for name, fn in (("kernel", lambda: promote_kv(*args, max_len=L, **kv.scales())), ("torch", lambda: promote_kv_reference(*args, **kv.scales()))):
            t = device_ms(fn)
            if rep:
                ms[name].append(t)
    ker, ref = statistics.median(ms["kernel"]), statistics.median(ms["torch"])
    emit(part="promote_launch", model=a.model, kv_dtype=a.kv_dtype, survivors=k, tokens=L, kv_heads=hkv, head_dim=d, bytes_moved=moved,
         us_kernel=round(ker * 1e3, 1), us_torch_reference=round(ref * 1e3, 1), gb_per_s_kernel=round(moved / ker / 1e6, 1),
         spread_kernel_us=[round(min(ms["kernel"]) * 1e3, 1), round(max(ms["kernel"]) * 1e3, 1)],
         spread_torch_us=[round(min(ms["torch"]) * 1e3, 1), round(max(ms["torch"]) * 1e3, 1)], reps=a.reps)

    # part 2: fork against re-prefilling the survivors
    def do_fork():
        model.fork(rows, lens, fed, old_batch=B)

    def do_prefill():
        model.append_shared(fed)

    ms = {"fork": [], "append_shared": []}
    for rep in range(a.reps + 1):
        for name, fn in (("fork", do_fork), ("append_shared", do_prefill)):
            model.truncate_shared_caches(1)
            t = wall_ms(fn)
            if rep:
                ms[name].append(t)
    nxt = dict(input_ids=last.repeat_interleave(E, 0)[:, None], num_return_sequences=1, max_new_tokens=T, temperature=1.0, shared_cache_op="preserve")
    gen = {}
    for name, fn in (("fork", do_fork), ("append_shared", do_prefill)):
        model.truncate_shared_caches(1)
        fn()
        model.generate(**nxt)  # (captures the graph of the two-level round)
        gen[name] = wall_ms(lambda: model.generate(**nxt))
    model.truncate_shared_caches(1)
    f, p = statistics.median(ms["fork"]), statistics.median(ms["append_shared"])
    emit(part="round_step", model=a.model, layers=cfg.num_hidden_layers, kv_dtype=a.kv_dtype, batch=B, prefix=P, step_tokens=T, survivors=k,
         expand=E, ms_fork=round(f, 3), ms_append_shared=round(p, 3), spread_fork_ms=[round(min(ms["fork"]), 3), round(max(ms["fork"]), 3)],
         spread_append_shared_ms=[round(min(ms["append_shared"]), 3), round(max(ms["append_shared"]), 3)],
         ms_first_round_generate=round(t_round0, 1), ms_next_round_generate_after_fork=round(gen["fork"], 1),
         ms_next_round_generate_after_append_shared=round(gen["append_shared"], 1), reps=a.reps)

r1, r2 = results
out = Path(a.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(f"""# Fork: promote unique K/V rows to a shared level (tools/fork_bench.py)

{a.model} shell ({r2['layers']} layers, random weights, bf16; unique cache {a.kv_dtype}), one shared prompt of {P} tokens, {B} completions,
{T}-token rounds, HIP-graph decode.  After a round, one completion in {E} survives ({k} survivors, {L} cached tokens each) and is
continued {E} times.  Medians over {a.reps} repetitions, (min .. max) behind them.

| what | fork (hyd_kv_promote) | without it |
|---|---|---|
| one layer: K and V of the survivors into the new level, device time | {r1['us_kernel']} us ({r1['spread_kernel_us'][0]} .. {r1['spread_kernel_us'][1]}), {r1['gb_per_s_kernel']} GB/s over {r1['bytes_moved'] / 1e6:.1f} MB read + written | promote_kv_reference in torch: {r1['us_torch_reference']} us ({r1['spread_torch_us'][0]} .. {r1['spread_torch_us'][1]}) |
| the step between two rounds, all layers, host wall time | model.fork: {r2['ms_fork']} ms ({r2['spread_fork_ms'][0]} .. {r2['spread_fork_ms'][1]}) | append_shared of the survivors' tokens: {r2['ms_append_shared']} ms ({r2['spread_append_shared_ms'][0]} .. {r2['spread_append_shared_ms'][1]}) |
| the next round's generate() ({B} x {T} tokens), once | {r2['ms_next_round_generate_after_fork']} ms | {r2['ms_next_round_generate_after_append_shared']} ms |

The first round's generate() (prefill of the prompt included, once): {r2['ms_first_round_generate']} ms.
""")
print(f"wrote {out}")
