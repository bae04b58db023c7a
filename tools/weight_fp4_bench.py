"""4-bit (e2m1) linear-layer weights: what hyd_linear_w4 costs against the fp8 kernel, the 16-bit GEMM and widen + GEMM, and what it
does to a decode step.  Writes the tables of profiles/weight_fp4.md (markdown, to --out or stdout); the protocol is
tools/weight_fp8_bench.py's: rings of distinct weights larger than the Infinity Cache (sized in 4-bit bytes, so the fp8 and 16-bit
rings of the same length are two and four times that), one HIP graph per variant, the variants' replays alternating in one process,
the median over the rounds per call.  The first variant is measured twice ("again"): the spread of a variant's own repeats.

    python tools/weight_fp4_bench.py [--out profiles/weight_fp4.md] [--rows 1,8,16,32,64,128,256] [--batches 32,128] [--layers 32]
                                     [--skip-model] [--skip-shapes]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from weight_fp8_bench import DEV, MODEL_SHAPES, RING_BYTES, SHAPES, graph_of, replay_us, weight_bytes  # noqa: E402

FP4 = torch.float4_e2m1fn_x2


def shape_table(name, N, K, rows, rounds, out):
    from hydragen_amd import weight_quant as wq

    n = RING_BYTES // (N * K // 2) + 2
    gen = torch.Generator(device=DEV).manual_seed(N + K)
    w4s = []
    for _ in range(n):  # random codes and shifts: the kernel's time does not depend on the values
        w4 = torch.randint(0, 256, (N, K // 2), device=DEV, generator=gen, dtype=torch.int32).to(torch.uint8)
        shift = torch.randint(0, 4, (N, K // 32), device=DEV, generator=gen, dtype=torch.int32).to(torch.uint8)
        w4s.append((w4, shift, torch.full((N,), 2.0 ** -7, device=DEV)))
    w16 = [wq.dequantize_weight_fp4(*t, torch.bfloat16) for t in w4s]
    w8s = [wq.quantize_weight(w) for w in w16]
    scratch = torch.empty((N, K), device=DEV, dtype=torch.bfloat16)
    ws = torch.empty((max(wq.max_workspace_bytes_w4(max(rows), N, K), wq.max_workspace_bytes(max(rows), N, K), 16),), dtype=torch.uint8, device=DEV)
    x8 = torch.randn((8, K), device=DEV, dtype=torch.bfloat16, generator=gen)
    got, want = wq.linear_w4(x8, *w4s[0]).double(), torch.nn.functional.linear(x8, w16[0]).double()
    out(f"### {name}: N = {N}, K = {K} ({n} weight buffers per ring)\n")
    out(f"Same product: relative L2 of hyd_linear_w4 against F.linear on the dequantized weight at M = 8: {float((got - want).norm() / want.norm()):.2e}.\n")
    out("| M | w4 us | w4 again us | TB/s | w8 us | 16-bit us | widen + F.linear us | w4 / w8 | w4 / 16-bit | w4 / widen |")
    out("|---|---|---|---|---|---|---|---|---|---|")
    res = {}
    for M in rows:
        x = torch.randn((M, K), device=DEV, dtype=torch.bfloat16, generator=gen)
        y = torch.empty((M, N), device=DEV, dtype=torch.bfloat16)

        def run_w4():
            for t in w4s:
                wq.linear_w4(x, *t, out=y, workspace=ws)

        def run_w8():
            for w8, s in w8s:
                wq.linear_w8(x, w8, s, out=y, workspace=ws)

        def run_16():
            for w in w16:
                torch.mm(x, w.t(), out=y)

        def run_widen():
            for t in w4s:
                torch.mm(x, wq.weight_widen_fp4(*t, scratch).t(), out=y)

        graphs = {k: graph_of(f) for k, f in (("w4", run_w4), ("w8", run_w8), ("16", run_16), ("widen", run_widen))}
        graphs["again"] = graphs["w4"]
        for g in graphs.values():
            replay_us(g, n, 1)
        t = {k: [] for k in graphs}
        for _ in range(rounds):  # alternate the variants
            for k, g in graphs.items():
                t[k].append(replay_us(g, n))
        us = {k: statistics.median(v) for k, v in t.items()}
        out(f"| {M} | {us['w4']:.1f} | {us['again']:.1f} | {N * K / 2 / us['w4'] * 1e-6:.2f} | {us['w8']:.1f} | {us['16']:.1f} | {us['widen']:.1f} | "
            f"{us['w4'] / us['w8']:.2f} | {us['w4'] / us['16']:.2f} | {us['w4'] / us['widen']:.2f} |")
        res[M] = us
        del graphs
    out("")
    return res


def model_part(args, out):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig.llama2_7b()
    cfg.num_hidden_layers = args.layers
    cfg.max_position_embeddings = max(cfg.max_position_embeddings, args.prefix + args.new + 32)
    models = {}
    for k, dt in (("16-bit", None), ("fp8", torch.float8_e4m3fn), ("e2m1", FP4)):
        models[k] = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0)
        if dt is not None:
            models[k].quantize_weights(dtype=dt)
        torch.cuda.empty_cache()
    out(f"## The Llama-2-7B shell ({args.layers} layers, random weights std 0.02, bf16), P = {args.prefix}, graph decode, temperature 0\n")
    out("Resident weight bytes (embedding, projections, shifts and scales, lm_head; the embedding and lm_head stay 16-bit): "
        + ", ".join(f"{k} {weight_bytes(m) / 2**30:.2f} GiB" for k, m in models.items()) + ".\n")
    prompt = torch.randint(1, cfg.vocab_size, (1, args.prefix), device=DEV)
    N, steps = args.new, args.new - 1
    out("| B | 16-bit ms per step | fp8 ms per step | e2m1 ms per step | e2m1 / 16-bit | e2m1 / fp8 |")
    out("|---|---|---|---|---|---|")
    for B in (int(b) for b in args.batches.split(",")):
        for m in models.values():
            m.setup_caches(max_unique_batch_size=B, max_unique_seq_length=N + 16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[args.prefix])
            m.graph(True)

        def run(m, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=n, temperature=0.0)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for m in models.values():
            run(m, 4)
        pre, full = {k: [] for k in models}, {k: [] for k in models}
        for _ in range(3):  # alternate the models
            for k, m in models.items():
                pre[k].append(run(m, 1))
                full[k].append(run(m, N))
        step = {k: (min(full[k]) - min(pre[k])) / steps * 1e3 for k in models}
        out(f"| {B} | {step['16-bit']:.3f} | {step['fp8']:.3f} | {step['e2m1']:.3f} | {step['e2m1'] / step['16-bit']:.2f} | {step['e2m1'] / step['fp8']:.2f} |")
        for m in models.values():
            m.graph(False)
    out("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1,8,16,32,64,128,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prefix", type=int, default=2048)
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_fp4_bench.py measures on the GPU: no device found")
    lines = []

    def out(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            Path(args.out).write_text("\n".join(lines) + "\n")

    rows = [int(r) for r in args.rows.split(",")]
    out("# 4-bit (e2m1) linear-layer weights: measurements\n")
    if not args.skip_shapes:
        out("## hyd_linear_w4 against hyd_linear_w8, the 16-bit GEMM and widen + GEMM (bf16 activations, us per call, weights streamed from HBM)\n")
        res = {name: shape_table(name, N, K, rows, args.rounds, out) for name, N, K in SHAPES}
        four = [n for n, _, _ in MODEL_SHAPES]
        crossover = 0
        for M in rows:  # the largest M up to which the kernel wins at every smaller measured M as well
            if M > 128 or not all(res[n][M]["w4"] < res[n][M]["widen"] for n in four):
                break
            crossover = M
        out(f"Crossover against widen + F.linear on all four decoder shapes: the kernel is faster at every measured M up to {crossover} "
            f"(W4_MAX_ROWS; at most 128, the extent of the rows form).\n")
        for n in four:
            for other, label in (("16", "the 16-bit F.linear"), ("w8", "hyd_linear_w8")):
                lost = [M for M in rows if res[n][M]["w4"] >= res[n][M][other]]
                out(f"- {n}: against {label} the kernel LOSES at M = {lost} and wins at M = {[M for M in rows if M not in lost]}.")
        out("")
    if not args.skip_model:
        model_part(args, out)


if __name__ == "__main__":
    main()
