"""fp8 linear-layer weights: what hyd_linear_w8 costs against the 16-bit GEMM it replaces, and what it does to a decode step.
Writes the tables of profiles/weight_fp8.md (markdown, to --out or stdout) -- nothing here is promised in advance.

    python tools/weight_fp8_bench.py [--out profiles/weight_fp8.md] [--rows 1,8,16,32,64,128,256,512] [--batches 32,128]
                                     [--layers 32] [--prefix 2048] [--new 33] [--skip-model]

Part 1 -- per weight shape (Llama-2-7B: q|k|v, o, gate|up, down, lm_head), bf16, per row count M: hyd_linear_w8, F.linear on the
16-bit weight (hipBLASLt: the path of a model that is not quantized) and hyd_weight_widen + F.linear (the route of a quantized
model above W8_MAX_ROWS).  Every variant walks a ring of distinct weight buffers that together exceed the 256 MB Infinity Cache
(the fp8 ring does; the 16-bit ring of the same length is twice that), so every call streams its weight from HBM as it does inside
a 32-layer model.  One pass over the ring is captured in a HIP graph per variant (device time, no launch gaps) and the variants'
replays alternate in one process; the figure is the median over the rounds, per call.  TB/s counts the weight bytes a variant has to
read (N x K for fp8, 2 N x K for 16-bit; the widen route is quoted in 16-bit bytes, like the GEMM it ends in).
Part 2 -- the Llama-2-7B shell (random weights, bf16, P = 2048, graph decode): ms per decode step with 16-bit and with fp8 weights,
alternating in one process, plain and with draft_tokens=3 (given drafts that are all wrong: every step emits one token, so decode time
/ steps is the step time), the resident weight bytes of both models, and the relative L2 of the fp8 model's logits against the 16-bit
model's on the same tokens (information, not a gate: three mantissa bits per weight)."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
SHAPES = [("q|k|v", 12288, 4096), ("o", 4096, 4096), ("gate|up", 22016, 4096), ("down", 4096, 11008), ("lm_head", 32000, 4096)]
MODEL_SHAPES = SHAPES[:4]
RING_BYTES = 320 << 20  # fp8 bytes of a ring: beyond the 256 MB Infinity Cache


def graph_of(fn):
    """One pass of fn captured in a HIP graph (after a warm-up pass on a side stream, as torch asks)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def replay_us(g, calls, reps=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * calls)


def shape_table(name, N, K, rows, rounds, out):
    from hydragen_amd import weight_quant as wq

    n = RING_BYTES // (N * K) + 2
    gen = torch.Generator(device=DEV).manual_seed(N + K)
    w16 = [torch.randn((N, K), device=DEV, dtype=torch.bfloat16, generator=gen) * 0.02 for _ in range(n)]
    pairs = [wq.quantize_weight(w) for w in w16]
    scratch = torch.empty((N, K), device=DEV, dtype=torch.bfloat16)
    ws = torch.empty((max(wq.max_workspace_bytes(max(rows), N, K), 16),), dtype=torch.uint8, device=DEV)
    x8 = torch.randn((8, K), device=DEV, dtype=torch.bfloat16, generator=gen)
    got = wq.linear_w8(x8, *pairs[0]).double()
    want = torch.nn.functional.linear(x8, wq.dequantize_weight(*pairs[0], torch.bfloat16)).double()
    out(f"### {name}: N = {N}, K = {K} ({n} weight buffers per ring)\n")
    out(f"Same product: relative L2 of hyd_linear_w8 against F.linear on the dequantized weight at M = 8: {float((got - want).norm() / want.norm()):.2e}; "
        f"the quantization itself, F.linear on the dequantized against the original weight: "
        f"{float((want - torch.nn.functional.linear(x8, w16[0]).double()).norm() / torch.nn.functional.linear(x8, w16[0]).double().norm()):.2e}.\n")
    out("| M | hyd_linear_w8 us | TB/s | F.linear 16-bit us | TB/s | widen + F.linear us | TB/s | w8 / 16-bit | w8 / widen |")
    out("|---|---|---|---|---|---|---|---|---|")
    res = {}
    for M in rows:
        x = torch.randn((M, K), device=DEV, dtype=torch.bfloat16, generator=gen)
        y = torch.empty((M, N), device=DEV, dtype=torch.bfloat16)

        def run_w8():
            for w8, s in pairs:
                wq.linear_w8(x, w8, s, out=y, workspace=ws)

        def run_16():
            for w in w16:
                torch.mm(x, w.t(), out=y)

        def run_widen():
            for w8, s in pairs:
                torch.mm(x, wq.weight_widen(w8, s, scratch).t(), out=y)

        graphs = {k: graph_of(f) for k, f in (("w8", run_w8), ("16", run_16), ("widen", run_widen))}
        for g in graphs.values():
            replay_us(g, n, 1)
        t = {k: [] for k in graphs}
        for _ in range(rounds):  # alternate the variants
            for k, g in graphs.items():
                t[k].append(replay_us(g, n))
        us = {k: statistics.median(v) for k, v in t.items()}
        tb = {"w8": N * K / us["w8"] * 1e-6, "16": 2 * N * K / us["16"] * 1e-6, "widen": 2 * N * K / us["widen"] * 1e-6}
        out(f"| {M} | {us['w8']:.1f} | {tb['w8']:.2f} | {us['16']:.1f} | {tb['16']:.2f} | {us['widen']:.1f} | {tb['widen']:.2f} | "
            f"{us['w8'] / us['16']:.2f} | {us['w8'] / us['widen']:.2f} |")
        res[M] = us
        del graphs
    out("")
    return res


def weight_bytes(model):
    from hydragen_amd.weight_quant import Fp8Linear

    return sum(t.numel() * t.element_size() for m in model.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Embedding, Fp8Linear))
               for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)))


def model_part(args, out):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig.llama2_7b()
    cfg.num_hidden_layers = args.layers
    cfg.max_position_embeddings = max(cfg.max_position_embeddings, args.prefix + args.new + 32)
    m16 = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
    m8 = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
    m8.quantize_weights()
    torch.cuda.empty_cache()
    models = {"16-bit": m16, "fp8": m8}
    out(f"## The Llama-2-7B shell ({args.layers} layers, random weights std 0.02, bf16), P = {args.prefix}, graph decode, temperature 0\n")
    out(f"Resident weight bytes (embedding, projections and scales, lm_head): 16-bit {weight_bytes(m16) / 2**30:.2f} GiB, "
        f"fp8 {weight_bytes(m8) / 2**30:.2f} GiB (the embedding and lm_head stay 16-bit).\n")
    prompt = torch.randint(1, cfg.vocab_size, (1, args.prefix), device=DEV)
    N, steps, l2 = args.new, args.new - 1, float("nan")
    out("| B | draft_tokens | rows per step | 16-bit ms per step | fp8 ms per step | fp8 / 16-bit |")
    out("|---|---|---|---|---|---|")
    for B in (int(b) for b in args.batches.split(",")):
        for m in models.values():
            m.setup_caches(max_unique_batch_size=B, max_unique_seq_length=N + 16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[args.prefix])
            m.graph(True)

        def run(m, n, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = m.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=n, temperature=0.0, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, o

        wrong = {}
        for k, m in models.items():
            run(m, 4)
            wrong[k] = (run(m, N)[1] + 1) % cfg.vocab_size
        for K in (0, 3):
            kw = {k: (dict(draft_tokens=K, draft=wrong[k]) if K else {}) for k in models}
            for k, m in models.items():
                run(m, 4, **(dict(draft_tokens=K, draft=wrong[k][:, :4]) if K else {}))
            pre, full = {k: [] for k in models}, {k: [] for k in models}
            for _ in range(3):  # alternate the two models
                for k, m in models.items():
                    pre[k].append(run(m, 1)[0])
                    full[k].append(run(m, N, **kw[k])[0])
            step = {k: (min(full[k]) - min(pre[k])) / steps * 1e3 for k in models}
            out(f"| {B} | {K or 'none'} | {B * (K + 1)} | {step['16-bit']:.3f} | {step['fp8']:.3f} | {step['fp8'] / step['16-bit']:.2f} |")
        if B == 32:
            G, l16 = m16.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=9, temperature=0.0, return_logits=True)
            _, l8 = m8.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=9, temperature=0.0, return_logits=True, token_overrides=G)
            st = lambda l: (l if isinstance(l, torch.Tensor) else torch.stack(list(l), 1)).double()  # noqa: E731
            l2 = float((st(l8) - st(l16)).norm() / st(l16).norm())
        for m in models.values():
            m.graph(False)
    out("")
    out(f"Relative L2 of the fp8 model's logits against the 16-bit model's (B = 32, 9 decode steps on the 16-bit model's tokens): {l2:.3e}.\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1,8,16,32,64,128,256,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_fp8_bench.py measures on the GPU: no device found")
    lines = []

    def out(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            Path(args.out).write_text("\n".join(lines) + "\n")

    rows = [int(r) for r in args.rows.split(",")]
    out("# fp8 linear-layer weights: measurements\n")
    if not args.skip_shapes:
        out("## hyd_linear_w8 against the 16-bit GEMM and against widen + GEMM (bf16 activations, per call, weights streamed from HBM)\n")
        res = {}
        for name, N, K in SHAPES:
            res[name] = shape_table(name, N, K, rows, args.rounds, out)
            torch.cuda.empty_cache()
        four = [n for n, _, _ in MODEL_SHAPES]
        beats_widen = [M for M in rows if all(res[n][M]["w8"] < res[n][M]["widen"] for n in four)]
        crossover = 0
        for M in rows:  # the largest M up to which the kernel wins at every smaller measured M as well
            if M not in beats_widen:
                break
            crossover = M
        out(f"Crossover against widen + F.linear on all four decoder shapes: the kernel is faster at every measured M up to {crossover} "
            f"(W8_MAX_ROWS is set from this).\n")
        for n in four:
            lost = [M for M in rows if M <= 64 and res[n][M]["w8"] >= res[n][M]["16"]]
            out(f"- {n}: against the 16-bit F.linear the kernel " + (f"does NOT win at M = {lost} (of M <= 64)" if lost else "wins at every measured M <= 64")
                + f"; it wins at M = {[M for M in rows if res[n][M]['w8'] < res[n][M]['16']]}.")
        out("")
    if not args.skip_model:
        model_part(args, out)


if __name__ == "__main__":
    main()
