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

Writes the table to --out and prints one JSON line per measurement.

    python tools/fork_bench.py --merge [--rounds 8] [--out profiles/fork_merge.md]

The merged fork (model.fork(merge_from=1): hyd_kv_gather_paths + one copy per layer) against the chain fork above, round by round,
on the same shape: after round r the chain hierarchy holds the prompt and r promoted levels, the merged one the prompt and ONE level
of r * step - 1 tokens per survivor.  Per round: one layer's gather launch (device time, bytes, next to hyd_kv_promote and to
gather_paths_reference in torch), the step between two rounds (chain fork / merged fork, host wall time), and the next round's
generate() on either hierarchy (once each, after the call that captures its graph).  Both hierarchies are kept alive side by side:
the chain's first level is saved before a merged fork overwrites its slot and put back afterwards."""
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
ap.add_argument("--out", default=None, help="default: profiles/fork.md, with --merge profiles/fork_merge.md")
ap.add_argument("--merge", action="store_true", help="the merged-fork leg: chain fork against fork(merge_from=1), rounds 1 .. --rounds")
ap.add_argument("--rounds", type=int, default=8)
a = ap.parse_args()
a.out = a.out or ("profiles/fork_merge.md" if a.merge else "profiles/fork.md")

assert torch.cuda.is_available(), "fork_bench.py measures on the GPU: there is no CPU figure"
dev = "cuda:0"
B, P, T, E = a.batch, a.prefix, a.step, a.expand
assert B % E == 0 and T >= 2
k, L = B // E, T - 1
cfg = LlamaConfig.llama2_7b() if a.model == "llama2-7b" else LlamaConfig.llama3_70b()
if a.layers:
    cfg.num_hidden_layers = a.layers
R = a.rounds if a.merge else 1
cfg.max_position_embeddings = max(cfg.max_position_embeddings, P + (R + 1) * T + 16)
model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=dev, seed=0)
model.graph(True)
# --merge: a level per round for the chain, and the first of them large enough for the merged paths of the last round
model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=T + 16, max_shared_batch_sizes=[1] + [k] * R,
                   max_shared_seq_lengths=[P] + ([R * T] + [T] * (R - 1) if a.merge else [T]),
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


def merge_leg():
    """--merge: see the module docstring."""
    from hydragen_amd.fork import gather_paths, gather_paths_reference

    med = statistics.median
    prompt = torch.randint(1, cfg.vocab_size, (1, P), device=dev)
    tokens = model.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=T, temperature=1.0, shared_cache_op="wipe")
    caches = [layer.self_attn.kv_cache for layer in model.model.layers]
    kv = caches[0]
    hkv, d = kv.per_completion_k_cache.shape[2:]
    D = kv.shared_caches[1].k_cache.shape[2]
    esz_u, esz_s = kv.per_completion_k_cache.element_size(), kv.shared_caches[1].k_cache.element_size()
    rows = torch.arange(0, B, E, device=dev)
    evict = torch.empty(1 << 30, dtype=torch.uint8, device=dev)  # written before every timed launch of part 1 (4 x the Infinity Cache)
    saved = None  # the chain's first level (slot 1) of every layer, as the round-1 chain fork left it

    def save_slot1():
        out = []
        for c in caches:
            sc = c.shared_caches[1]
            n = k * L
            out.append((sc.k_cache[:n].clone(), sc.v_cache[:n].clone(), sc.seq_lens.clone(), sc.cumsum_lengths.clone(), sc.use_varlen,
                        sc.sliced_sequence_length, sc.current_batch_size))
        return out

    def restore(used, bitmaps):
        for c, snap in zip(caches, saved or [None] * len(caches)):
            if snap is not None:
                sc = c.shared_caches[1]
                sc.k_cache[: snap[0].shape[0]].copy_(snap[0])
                sc.v_cache[: snap[1].shape[0]].copy_(snap[1])
                sc.seq_lens.copy_(snap[2])
                sc.cumsum_lengths.copy_(snap[3])
                sc.use_varlen, sc.sliced_sequence_length, sc.current_batch_size = snap[4:]
            c.num_used_shared_caches = used
        model.shared_bitmaps[:] = bitmaps

    for r in range(1, R + 1):
        # state: the prompt and r - 1 chain levels in use; the unique caches hold the last round's B rows, cached L tokens
        # (round 1) or T (a one-token prompt and T - 1 steps)
        n_cached = L if r == 1 else T
        lens = torch.full((k,), n_cached, dtype=torch.int32, device=dev)
        fed = tokens[rows, :L] if r == 1 else torch.cat([last[:, None], tokens[rows, :L]], dim=1)
        nxt_last = tokens[rows, L]
        used, bitmaps = r, list(model.shared_bitmaps)
        assert model.get_num_used_shared_caches() == used
        path = (r - 1) * T + L if r > 1 else L  # tokens per survivor in the merged level after this fork

        # one layer's launches: the gather into a staging buffer, the promote into the next free slot, the torch definition
        chain = [(c.k_cache, c.v_cache, c.cumsum_lengths, c.current_batch_size) for c in kv.get_used_shared_caches()[1:]]
        stage = torch.empty((2, k * path, hkv, D), dtype=kv.shared_caches[1].k_cache.dtype, device=dev)
        src = (kv.per_completion_k_cache, kv.per_completion_v_cache, rows, lens)
        free = kv.shared_caches[used]
        fns = (("gather", lambda: gather_paths(chain, *src, stage[0], stage[1], old_batch=B, max_len=n_cached, max_path=path, **kv.scales())),
               ("promote", lambda: promote_kv(*src, free.k_cache, free.v_cache, max_len=n_cached, **kv.scales())),
               ("torch", lambda: gather_paths_reference(chain, *src, stage[0], stage[1], old_batch=B, **kv.scales())))
        ms = {name: [] for name, _ in fns}
        for rep in range(a.reps + 1):
            for name, fn in (fns if rep % 2 else fns[::-1]):  # alternating order
                evict.fill_(rep)  # every launch starts cold: the three read the same unique rows, and half of them fit the Infinity Cache
                t = device_ms(fn)
                if rep:
                    ms[name].append(t)
        b_gather = 2 * k * hkv * ((path - n_cached) * 2 * D * esz_s + n_cached * (d * esz_u + D * esz_s))
        b_promote = 2 * k * n_cached * hkv * (d * esz_u + D * esz_s)
        del stage
        emit(part="gather_launch", round=r, survivors=k, path_tokens=path, chain_levels=r - 1, bytes_gather=b_gather, bytes_promote=b_promote,
             us_gather=round(med(ms["gather"]) * 1e3, 1), spread_gather_us=[round(min(ms["gather"]) * 1e3, 1), round(max(ms["gather"]) * 1e3, 1)],
             tb_per_s_gather=round(b_gather / med(ms["gather"]) / 1e9, 2),
             us_promote=round(med(ms["promote"]) * 1e3, 1), spread_promote_us=[round(min(ms["promote"]) * 1e3, 1), round(max(ms["promote"]) * 1e3, 1)],
             tb_per_s_promote=round(b_promote / med(ms["promote"]) / 1e9, 2),
             tb_per_s_promote_spread=[round(b_promote / max(ms["promote"]) / 1e9, 2), round(b_promote / min(ms["promote"]) / 1e9, 2)],
             us_torch_reference=round(med(ms["torch"]) * 1e3, 1), reps=a.reps)

        # the step between two rounds, all layers, host wall time: chain fork against merged fork
        ms = {"chain": [], "merged": []}
        for rep in range(a.reps + 1):
            t = wall_ms(lambda: model.fork(rows, lens, fed, old_batch=B))
            model.truncate_shared_caches(used)
            model.shared_bitmaps[:] = bitmaps
            t2 = wall_ms(lambda: model.fork(rows, lens, fed, old_batch=B, merge_from=1))
            restore(used, bitmaps)
            if rep:
                ms["chain"].append(t)
                ms["merged"].append(t2)

        # the next round's generate(): chain depth r against merged depth 1
        model.fork(rows, lens, fed, old_batch=B)
        if r == 1:
            saved = save_slot1()
        bitmaps_after = list(model.shared_bitmaps)
        nxt = dict(input_ids=nxt_last.repeat_interleave(E, 0)[:, None], num_return_sequences=1, max_new_tokens=T, temperature=1.0, shared_cache_op="preserve")
        model.generate(**nxt)  # (captures the graph of this depth)
        t_chain = [wall_ms(lambda: model.generate(**nxt)) for _ in range(3)]
        # the same paths as ONE level: merge the chain, the new level included, with no unique tokens (every survivor its own row)
        model.fork(torch.arange(k, device=dev), torch.zeros(k, dtype=torch.int32, device=dev), fed[:, :1], old_batch=k, merge_from=1)
        assert model.get_num_used_shared_caches() == 2
        model.generate(**nxt)  # (the two-level graph: captured in round 1, replayed afterwards unless the key changed)
        out = []
        t_merged = [wall_ms(lambda: out.append(model.generate(**nxt))) for _ in range(3)]
        tokens, last = out[-1], nxt_last
        # the gather as a search that merges EVERY round issues it: one chain level that holds the whole path, then the new rows
        one = [(c.k_cache, c.v_cache, c.cumsum_lengths, c.current_batch_size) for c in kv.get_used_shared_caches()[1:]]
        assert len(one) == 1
        lens_t = torch.full((k,), T, dtype=torch.int32, device=dev)
        stage = torch.empty((2, k * (path + T), hkv, D), dtype=kv.shared_caches[1].k_cache.dtype, device=dev)
        t_one = []
        for rep in range(a.reps + 1):
            evict.fill_(rep)
            t = device_ms(lambda: gather_paths(one, kv.per_completion_k_cache, kv.per_completion_v_cache, rows, lens_t, stage[0], stage[1],
                                               old_batch=B, max_len=T, max_path=path + T, **kv.scales()))
            if rep:
                t_one.append(t)
        del stage
        b_one = 2 * k * hkv * (path * 2 * D * esz_s + T * (d * esz_u + D * esz_s))
        emit(part="gather_one_level", round=r + 1, path_tokens=path + T, bytes_gather=b_one, us_gather=round(med(t_one) * 1e3, 1),
             spread_gather_us=[round(min(t_one) * 1e3, 1), round(max(t_one) * 1e3, 1)], tb_per_s_gather=round(b_one / med(t_one) / 1e9, 2),
             tb_per_s_gather_spread=[round(b_one / max(t_one) / 1e9, 2), round(b_one / min(t_one) / 1e9, 2)], reps=a.reps)
        restore(used + 1, bitmaps_after)  # the chain goes on; the unique caches hold the rows of the last generate()
        emit(part="round", round=r, levels_chain=1 + r, levels_merged=2, one_call_operator_chain=(1 + r) <= 8, path_tokens=path,
             ms_chain_fork=round(med(ms["chain"]), 3), spread_chain_fork_ms=[round(min(ms["chain"]), 3), round(max(ms["chain"]), 3)],
             ms_merged_fork=round(med(ms["merged"]), 3), spread_merged_fork_ms=[round(min(ms["merged"]), 3), round(max(ms["merged"]), 3)],
             ms_next_generate_chain=round(med(t_chain), 1), spread_next_generate_chain_ms=[round(min(t_chain), 1), round(max(t_chain), 1)],
             ms_next_generate_merged=round(med(t_merged), 1), spread_next_generate_merged_ms=[round(min(t_merged), 1), round(max(t_merged), 1)],
             reps=a.reps)

    g = [x for x in results if x["part"] == "gather_launch"]
    rd = [x for x in results if x["part"] == "round"]
    faster = [x["round"] for x in rd if x["spread_next_generate_merged_ms"][1] < x["spread_next_generate_chain_ms"][0]]
    slower = [x["round"] for x in rd if x["spread_next_generate_merged_ms"][0] > x["spread_next_generate_chain_ms"][1]]
    short = [x["round"] for x in g if x["tb_per_s_gather"] < x["tb_per_s_promote_spread"][0]]
    lines = [f"# Fork with merged levels: gather paths into one level (tools/fork_bench.py --merge)", "",
             f"{a.model} shell ({cfg.num_hidden_layers} layers, random weights, bf16; unique cache {a.kv_dtype}), one shared prompt of {P} tokens, {B} completions,",
             f"{T}-token rounds, HIP-graph decode, {k} survivors per round, each continued {E} times (the shape of profiles/fork.md).  After round r the chain",
             f"hierarchy holds the prompt and r promoted levels, the merged one the prompt and one level of r x {T} - 1 tokens per survivor.",
             f"Medians over {a.reps} repetitions (generate(): 3), (min .. max) behind them.", "",
             "## One layer: the gather launch (device time)", "",
             "The three launches alternate in order, and a 1 GiB buffer is written before each: they read the same unique rows, of which half would",
             "otherwise still sit in the 256 MiB Infinity Cache for whichever runs second.", "",
             "| round | path tokens | hyd_kv_gather_paths | bytes read + written | TB/s | hyd_kv_promote, same process | TB/s | gather_paths_reference (torch) |",
             "|---|---|---|---|---|---|---|---|"]
    for x in g:
        lines.append(f"| {x['round']} | {x['path_tokens']} | {x['us_gather']} us ({x['spread_gather_us'][0]} .. {x['spread_gather_us'][1]}) | {x['bytes_gather'] / 1e6:.1f} MB | "
                     f"{x['tb_per_s_gather']} | {x['us_promote']} us ({x['spread_promote_us'][0]} .. {x['spread_promote_us'][1]}) | {x['tb_per_s_promote']} "
                     f"({x['tb_per_s_promote_spread'][0]} .. {x['tb_per_s_promote_spread'][1]}) | {x['us_torch_reference']} us |")
    one = [x for x in results if x["part"] == "gather_one_level"]
    lines += ["", ("The gather's rate is inside or above the spread of this run's promote figure in every round." if not short else
                   f"The gather's rate falls below the spread of this run's promote figure in rounds {short}."
                   "  Round 1 has no chain: the launch then runs kv_promote_kernel's body on the same bytes, and repeated runs of this tool put it a few"
                   " percent on either side of the promote figure.  The deep chains are what costs: every workgroup walks the chain twice before its first"
                   " vector load -- once to check every level's offsets, once to copy -- and each step of the walk is a pair of dependent scalar loads; it"
                   " then moves 16 KiB.  The table above gathers r - 1 SHORT levels because this tool keeps the chain alive next to the merged level.  A"
                   " search that merges in every round never builds that chain: its gather reads ONE level that holds the whole path, then the new rows --"
                   " the same bytes without the walk, measured below."), "",
              "| the gather of round | path tokens | chain levels | hyd_kv_gather_paths | bytes read + written | TB/s |", "|---|---|---|---|---|---|"]
    for x in one:
        lines.append(f"| {x['round']} | {x['path_tokens']} | 1 | {x['us_gather']} us ({x['spread_gather_us'][0]} .. {x['spread_gather_us'][1]}) | {x['bytes_gather'] / 1e6:.1f} MB | "
                     f"{x['tb_per_s_gather']} ({x['tb_per_s_gather_spread'][0]} .. {x['tb_per_s_gather_spread'][1]}) |")
    lines += ["",
              "## The step between two rounds (all layers, host wall time) and the next round's generate() (after the call that captures its graph)", "",
              "| round | levels chain / merged | chain fork | merged fork (gather + copy-back of the whole path) | next generate(), chain | next generate(), merged |",
              "|---|---|---|---|---|---|"]
    for x in rd:
        note = "" if x["one_call_operator_chain"] else " (past HYD_MAX_LEVELS: the general form)"
        lines.append(f"| {x['round']} | {x['levels_chain']} / {x['levels_merged']} | {x['ms_chain_fork']} ms ({x['spread_chain_fork_ms'][0]} .. {x['spread_chain_fork_ms'][1]}) | "
                     f"{x['ms_merged_fork']} ms ({x['spread_merged_fork_ms'][0]} .. {x['spread_merged_fork_ms'][1]}) | {x['ms_next_generate_chain']} ms ({x['spread_next_generate_chain_ms'][0]} .. {x['spread_next_generate_chain_ms'][1]}){note} | {x['ms_next_generate_merged']} ms ({x['spread_next_generate_merged_ms'][0]} .. {x['spread_next_generate_merged_ms'][1]}) |")
    lines += ["", (f"The merged hierarchy's generate() is faster than the chain's, beyond the spread of both, in rounds {faster}"
                   + (f", and slower in rounds {slower}." if slower else ", and slower in none.") if faster else
                   "Finding: the merged hierarchy's generate() is not faster than the chain's, beyond the spread, in any round measured."),
              "The merged fork recopies the whole path, so its cost grows with the round; the chain fork's does not.  What a search pays per",
              "round is the fork plus the generate(): " + ", ".join(f"round {x['round']}: chain {x['ms_chain_fork'] + x['ms_next_generate_chain']:.0f} ms, merged "
                                                                    f"{x['ms_merged_fork'] + x['ms_next_generate_merged']:.0f} ms" for x in rd) + ".", ""]
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines))
    print(f"wrote {out_path}")


if a.merge:
    with torch.no_grad():
        merge_leg()
    sys.exit(0)

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
