"""Speculative decoding on a Llama-2-7B shell (random weights, bf16, P = 2048): what a T-token decode step costs and what acceptance
rate pays for it.  Writes the tables of profiles/speculative.md to stdout (markdown) -- nothing here is promised in advance.

    python tools/spec_bench.py [--batches 32,128,1024] [--new 33] [--prefix 2048] [--layers 32] [--no-graph] [--kv-cache-dtype fp8]

--kv-cache-dtype fp8: the unique caches hold e4m3fn bytes with unit scales (setup_caches(kv_cache_dtype=torch.float8_e4m3fn)): the
multi-token preamble quantizes, the causal-tail suffix pass is the fp8 matrix-core kernel (profiles/speculative_fp8.md).

Step time: generate() with GIVEN drafts that are all wrong (every step emits exactly one token, so decode time / steps is the step
time of a T-token step); T = 1 is the plain path.  Break-even acceptance per T: the fraction a of the K drafts that has to be
accepted per step for tokens/s to equal the plain path, (1 + a K) / step_T = 1 / step_1.  Tokens/s at forced acceptance: the tokens
of the all-wrong run at the same T (same kernels, same shapes -- plain decoding's tokens do not serve: a random-weight bf16 model has
near ties in its logits, and a T-token step breaks them differently) are handed back as drafts, each kept with the given rate and
corrupted otherwise; the acceptance a run actually reached is printed beside its tokens/s.  Prompt lookup on random weights
accepts next to nothing by nature (a random model does not copy its prompt): reported as measured, not tuned for."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"


def timed(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def kernel_times(B, T, Hq, Hkv, D, P, S, fp8=False):
    """us per launch of the four new kernels, and of the assembled four-launch attention against the fused causal call.  fp8: the
    unique caches hold e4m3fn bytes with unit scales (the assembled route reads 16-bit rows: timed on the caches they were quantized from)."""
    from hydragen_amd import speculative
    from hydragen_amd.attention import hydragen_attention
    from hydragen_amd.flash import flash_attention_seqlen
    from hydragen_amd.fused_decode import rope_append_multi
    from hydragen_amd.llama import RotaryTable

    dt = torch.bfloat16
    q, k, v = (torch.randn(B, T, h, D, device=DEV, dtype=dt) for h in (Hq, Hkv, Hkv))
    kc, vc = (torch.randn(B, S + 16, Hkv, D, device=DEV, dtype=dt) for _ in range(2))
    sk, sv = (torch.randn(1, P, Hkv, D, device=DEV, dtype=dt) for _ in range(2))
    rot = RotaryTable(D, P + S + 64, 10000.0, device=DEV)
    pos = torch.full((B,), P + S - T, device=DEV, dtype=torch.int64)
    shared = torch.full((B,), P, device=DEV, dtype=torch.int64)
    lens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    ids = torch.randint(0, 32000, (1, P), device=DEV)
    gen = torch.randint(0, 32000, (B, S), device=DEV)
    glen = torch.full((B,), S // 2, device=DEV, dtype=torch.int32)
    fed = torch.randint(0, 32000, (B, T), device=DEV)
    state = speculative.new_state(B, S, 0, DEV)
    live = torch.zeros((1,), dtype=torch.int32, device=DEV)
    start = torch.full((B,), P, device=DEV, dtype=torch.int64)
    lv = dict(shared_ks=[sk], shared_vs=[sv], shared_cu_seq_lens=[None], shared_max_seq_lens=[None], use_varlens=[False])
    sc = {}
    if fp8:
        from hydragen_amd.kv_quant import quantize_kv

        kc16, vc16 = kc, vc
        kc, vc = quantize_kv(kc), quantize_kv(vc)
        sc = dict(k_scale=torch.ones(Hkv, device=DEV), v_scale=torch.ones(Hkv, device=DEV))

    def accept():
        state[1].zero_()
        speculative.draft_accept(fed, fed, *state[:4], live, start, shared, (), 0, S)

    return {
        "hyd_rope_append_multi": timed(lambda: rope_append_multi(q, k, v, rot.cos_cached, rot.sin_cached, pos, shared, kc, vc, **sc)),
        "hyd_suffix_attn_causal_fwd": timed(lambda: flash_attention_seqlen(q, kc, vc, lens, causal_tail=True, **sc)),
        "hyd_draft_lookup": timed(lambda: speculative.draft_lookup([speculative.Segment(ids), speculative.Segment(gen, glen)], B, T - 1)),
        "hyd_draft_accept (+ a memset)": timed(accept),
        "fused causal call (levels + causal tail)": timed(lambda: hydragen_attention(q, kc, vc, **lv, seq_lens=lens, causal_tail=True, **sc)),
        "assembled (level, old keys, causal block, combine)" + (" on 16-bit caches" if fp8 else ""): timed(
            lambda: speculative.assembled_causal_tail_attention(q, kc16 if fp8 else kc, vc16 if fp8 else vc, lens, [sk], [sv])),
    }


def alternating(fns: dict, repeats=7, iters=20):
    """{name: (median, min, max) us per call}: the candidates take turns, `repeats` rounds of `iters` calls each, so that clock and
    cache drift hits them alike; the spread is over the rounds."""
    got = {name: [] for name in fns}
    for r in range(repeats):
        for name, fn in fns.items():
            got[name].append(timed(fn, iters, warm=3 if r == 0 else 1))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in got.items()}


def cell(x):
    return f"{x[0]:.1f} ({x[1]:.1f} - {x[2]:.1f})"


def stop_accept_times():
    """hyd_draft_accept_stop against hyd_draft_accept: us per launch (+ the memset that resets the lengths), random tokens over a
    32000 vocabulary, stop sequences of 16 random tokens -- the common step, where the last token decides."""
    from hydragen_amd import speculative, stopping

    print("## 1. The accept launch\n\nus per launch with the memset that resets the lengths, median (min - max) of 7 alternating rounds of 20 "
          "launches, eager, host-timed back to back.  Stop sequences: 16 random tokens each.\n")
    print("| B | T | hyd_draft_accept | 0 stops + lists | 4 stops | 32 stops | 32 stops + lists |")
    print("|---|---|---|---|---|---|---|")
    S = 64
    for B in (128, 1024):
        for T in (4, 8):
            fed = torch.randint(0, 32000, (B, T), device=DEV)
            state = speculative.new_state(B, S, 0, DEV)
            live = torch.zeros((1,), dtype=torch.int32, device=DEV)
            start = torch.full((B,), 2048, device=DEV, dtype=torch.int64)
            gen, gen_len = torch.zeros((B, S), dtype=torch.int32, device=DEV), torch.zeros((B,), dtype=torch.int32, device=DEV)

            def call(n_stop=None, lists=False):
                kw = {}
                if n_stop is not None:
                    spec = stopping.StopSpec(stops=tuple(tuple(torch.randint(0, 32000, (16,)).tolist()) for _ in range(n_stop)))
                    kw.update(stop=spec, stop_tokens=spec.stop_table(DEV)[0] if n_stop else None)
                if lists:
                    kw.update(gen=gen, gen_len=gen_len)

                def fn():
                    state[1].zero_()
                    if lists:
                        gen_len.zero_()
                    speculative.draft_accept(fed, fed, *state[:4], live, start, start, (2,), 0, S, **kw)
                return fn

            r = alternating({"old": call(), "lists": call(0, True), "4": call(4), "32": call(32), "32l": call(32, True)})
            print(f"| {B} | {T} | {cell(r['old'])} | {cell(r['lists'])} | {cell(r['4'])} | {cell(r['32'])} | {cell(r['32l'])} |")
    print()


def penalized_drafts_times():
    """hyd_sample_tokens_penalized_drafts against hyd_sample_tokens_penalized on the same B * T logits rows with the lists expanded
    on the host beforehand (sampling.draft_row_lists_reference; the expansion itself is not timed)."""
    from hydragen_amd import layer_ops, sampling

    print("## 2. The penalised draw of a step\n\nus per launch, median (min - max) of 7 alternating rounds of 20 launches; bf16 logits, top-p 0.95, "
          "temperature 1, repetition 1.1 / frequency 0.1 / presence 0.1, 64 generated tokens per sequence, B = 128.  The existing call "
          "reads lists expanded to one per logits row beforehand (the expansion is not timed).\n")
    print("| V | T | rows | hyd_sample_tokens_penalized, expanded lists | hyd_sample_tokens_penalized_drafts | ratio |")
    print("|---|---|---|---|---|---|")
    B = 128
    for V in (32000, 128256):
        for T in (4, 8):
            x = (torch.randn(B * T, V, device=DEV) * 3).to(torch.bfloat16)
            gen = torch.randint(0, V, (B, 64), dtype=torch.int32, device=DEV)
            gen_len = torch.full((B,), 64, dtype=torch.int32, device=DEV)
            fed = torch.randint(0, V, (B, T), device=DEV)
            lists, lens = sampling.draft_row_lists_reference(gen.cpu(), gen_len.cpu(), fed.cpu())
            seq = layer_ops.Penalties(1.1, 0.1, 0.1, gen=gen, gen_len=gen_len)
            row = layer_ops.Penalties(1.1, 0.1, 0.1, gen=lists.to(torch.int32).to(DEV).contiguous(), gen_len=lens.to(DEV))
            r = alternating({"old": lambda: layer_ops.sample_tokens_penalized(x, 1.0, (1, 0), penalties=row, top_p=0.95),
                             "new": lambda: layer_ops.sample_tokens_penalized(x, 1.0, (1, 0), penalties=seq, top_p=0.95, drafts=fed)})
            print(f"| {V} | {T} | {B * T} | {cell(r['old'])} | {cell(r['new'])} | {r['new'][0] / r['old'][0]:.3f} |")
    print()


def stop_penalties_report(args):
    """The tables of profiles/speculative_stop_penalties.md, from one process."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    print("# Speculative decoding with stop sequences and penalties: measurements\n\nOne process on one MI355X; every comparison alternates its "
          "candidates and reports the spread.\n")
    stop_accept_times()
    penalized_drafts_times()
    cfg = LlamaConfig.llama2_7b()
    cfg.num_hidden_layers = args.layers
    cfg.max_position_embeddings = max(cfg.max_position_embeddings, args.prefix + args.new + 32)
    model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
    model.graph(not args.no_graph)
    prompt = torch.randint(1, cfg.vocab_size, (1, args.prefix), device=DEV)
    N, steps, K = args.new, args.new - 1, 3
    print(f"## 3. The T-token step with penalties\n\nLlama-2-7B shell ({args.layers} layers, random weights, bf16), P = {args.prefix}, {N} new tokens, "
          f"{'eager' if args.no_graph else 'HIP-graph'} decode, T = {K + 1}, all-wrong given drafts (every step emits one token: decode time / steps is "
          "the step time), temperature 0.  Penalties: repetition 1.1, frequency 0.1.  ms per step, median (min - max) of 3 alternating runs.\n")
    print("| B | without penalties | with penalties | with penalties and 4 stop sequences | penalties cost per step |")
    print("|---|---|---|---|---|")
    for B in (int(b) for b in args.batches.split(",")):
        model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=N + 16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[args.prefix])

        def run(n, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=n, temperature=0.0, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        run(4)
        pre = min(run(1)[0] for _ in range(2))
        wrong = (run(N)[1] + 1) % cfg.vocab_size
        pen = dict(repetition_penalty=1.1, frequency_penalty=0.1)
        stops = [torch.randint(1, cfg.vocab_size, (16,)).tolist() for _ in range(4)]
        variants = {"plain": {}, "pen": pen, "pen+stop": dict(pen, stop=stops)}
        for kw in variants.values():
            run(4, draft_tokens=K, draft=wrong[:, :4], **kw)
        got = {name: [] for name in variants}
        for _ in range(3):
            for name, kw in variants.items():
                got[name].append((run(N, draft_tokens=K, draft=wrong, **kw)[0] - pre) / steps * 1e3)
        med = {name: (sorted(v)[1], min(v), max(v)) for name, v in got.items()}
        c = lambda x: f"{x[0]:.3f} ({x[1]:.3f} - {x[2]:.3f})"  # noqa: E731
        print(f"| {B} | {c(med['plain'])} | {c(med['pen'])} | {c(med['pen+stop'])} | {(med['pen'][0] - med['plain'][0]) * 1e3:.0f} us |")
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,128,1024")
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--kv-cache-dtype", choices=("16-bit", "fp8"), default="16-bit")
    ap.add_argument("--stop-penalties", action="store_true",
                    help="write the tables of profiles/speculative_stop_penalties.md instead: the accept launch with stop sequences and "
                         "lists, the penalised draw of a step, the T-token step with penalties (--batches 32,128)")
    args = ap.parse_args()
    if args.stop_penalties:
        return stop_penalties_report(args)
    fp8 = args.kv_cache_dtype == "fp8"
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig.llama2_7b()
    cfg.num_hidden_layers = args.layers
    cfg.max_position_embeddings = max(cfg.max_position_embeddings, args.prefix + args.new + 32)
    model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
    model.graph(not args.no_graph)
    prompt = torch.randint(1, cfg.vocab_size, (1, args.prefix), device=DEV)
    N, steps = args.new, args.new - 1
    print(f"# Speculative decoding: measurements\n\nLlama-2-7B shell ({args.layers} layers, random weights, bf16), P = {args.prefix}, {N} new tokens, "
          f"{'eager' if args.no_graph else 'HIP-graph'} decode, temperature 0, {'fp8 (e4m3fn, unit scales)' if fp8 else '16-bit'} unique caches.\n")
    for B in (int(b) for b in args.batches.split(",")):
        model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=N + 16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[args.prefix],
                           **(dict(kv_cache_dtype=torch.float8_e4m3fn) if fp8 else {}))

        def run(n, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=n, temperature=0.0, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        run(4)
        pre = min(run(1)[0] for _ in range(2))
        full, G = min((run(N) for _ in range(2)), key=lambda r: r[0])
        step1 = (full - pre) / steps
        wrong = (G + 1) % cfg.vocab_size
        print(f"## B = {B}\n\nplain path (T = 1): {step1 * 1e3:.3f} ms per step, {B / step1:.0f} tokens/s\n")
        print("| T | ms per step | x plain | break-even acceptance | tokens/s at 0 % | drafts kept 50 %: tokens/s (accepted / proposed) | "
              "drafts kept 100 % | prompt lookup |")
        print("|---|---|---|---|---|---|---|---|")
        for T in range(2, 9):
            K = T - 1
            kw = dict(draft_tokens=K, return_draft_stats=True)
            run(4, **dict(kw, draft=wrong[:, :4]))
            t_wrong, (W, _) = min((run(N, draft=wrong, **kw) for _ in range(2)), key=lambda r: r[0])
            step_t = (t_wrong - pre) / steps
            # the tokens of the all-wrong run come from the same kernels at the same shapes as the runs below: handed back as
            # drafts they are accepted as long as the run reproduces them (the acceptance it reached is printed beside the rate)
            cells = []
            for rate in (0.5, 1.0):
                keep = torch.rand(W.shape, device=DEV) < rate
                d = torch.where(keep, W, (W + 1) % cfg.vocab_size)
                t, (_, st) = min((run(N, draft=d, **kw) for _ in range(2)), key=lambda r: r[0])
                cells.append(f"{B * steps / (t - pre):.0f} ({int(st.accepted.sum())} / {int(st.proposed.sum())})")
            t_pl, (_, st) = min((run(N, **kw) for _ in range(2)), key=lambda r: r[0])
            print(f"| {T} | {step_t * 1e3:.3f} | {step_t / step1:.2f} | {(step_t / step1 - 1) / K * 100:.0f} % | {B / step_t:.0f} | {cells[0]} | {cells[1]} | "
                  f"{B * steps / (t_pl - pre):.0f} ({int(st.accepted.sum())} / {int(st.proposed.sum())}) |")
        print()
        model.graph(False)
        kt = kernel_times(B, 4, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads, args.prefix, 64, fp8)
        model.graph(not args.no_graph)
        print("per launch at T = 4, suffix 64 (us, eager, host-timed back to back):\n")
        for name, us in kt.items():
            print(f"- {name}: {us:.1f}")
        print()


if __name__ == "__main__":
    main()
