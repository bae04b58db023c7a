"""Mixture-of-experts MLP: what one layer's moe_mlp (router GEMM + hyd_moe_mlp's five launches) costs at decode sizes, against the
time to stream the weights it has to read and against transformers' own block.  Writes the tables of profiles/moe.md (markdown, to
--out or stdout) -- nothing here is promised in advance.

    python tools/moe_bench.py [--out profiles/moe.md] [--rows 1,8,32,128] [--rounds 5] [--skip-eager]
    python tools/moe_bench.py --experts fp8 --out profiles/moe.md     (appends the fp8 section to the file)
    python tools/moe_bench.py --experts fp4 --rows 1,8,16,32,64,128 --out profiles/moe.md     (appends the 4-bit section)
    python tools/moe_bench.py --experts grouped --out profiles/moe.md     (appends the large-call section)
    python tools/moe_bench.py --experts grouped_fp8 --out profiles/moe.md     (appends the large-call section for fp8 experts)

Per shape -- a Mixtral-8x7B layer (E 8, k 2, H 4096, I 14336) and a Qwen3-30B-A3B layer (E 128, k 8, H 2048, I 768), bf16, random
weights -- and per row count T: a ring of distinct layers whose ACTIVATED experts together exceed the 256 MB Infinity Cache, so every
call streams its weights from HBM as it does inside a model; one pass over the ring is captured in a HIP graph (device time, no launch
gaps), the figure is the median over the rounds, per layer.  Beside it: the floor -- the bytes of the distinct activated experts of a
layer (mean over the ring: 3 H I 2 bytes each) at 8 TB/s -- and transformers' sparse block on the same weights, run eagerly (it
synchronises with the host to loop over the experts that were hit, so it cannot be captured; wall time per layer with a device
synchronisation at the end of the ring).
--experts fp8: the same rings with their experts quantized (moe.quantize_experts, hyd_moe_mlp_w8) beside the 16-bit originals, both
captured, replayed alternately round by round in this one process; the fp8 floor is half the bytes.
--experts fp4: three forms of the same rings -- 16-bit, fp8 and 4-bit (moe.quantize_experts_fp4, hyd_moe_mlp_w4) -- alternated the same
way; the 4-bit floor is the codes, shifts and scales of the activated experts (4.25 bits per weight and 4 bytes per channel).
--experts grouped: large calls (default rows 256,512,1024,2048) -- the grouped call (moe.moe_rows_grouped, hyd_moe_mlp_grouped) beside
the chunked route (moe.moe_rows per 128 rows), both behind the same router GEMM, alternated the same way; two floors: the activated
experts' bytes at 8 TB/s and the two products' FLOPs at the dense bf16 peak.
--experts grouped_fp8: the same rows and rings with their experts quantized -- the chunked fp8 route (moe.moe_rows_w8 per 128 rows), the
grouped fp8 call (moe.moe_rows_grouped_w8, hyd_moe_mlp_grouped_w8) and the grouped 16-bit call on the originals, alternated the same
way; the byte floor is the activated experts' code bytes."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"
SHAPES = [("Mixtral-8x7B layer", "mixtral", 8, 2, 4096, 14336), ("Qwen3-30B-A3B layer", "qwen3_moe", 128, 8, 2048, 768)]
RING_BYTES = 320 << 20  # activated bytes of a ring: beyond the 256 MB Infinity Cache
HBM_TBS = 8.0
BF16_PFLOPS = 2.5  # dense bf16 matrix peak


def graph_of(fn):
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


def hf_blocks(kind, layers, E, k, H, I):
    """transformers' sparse block per ring layer, its parameters the ring's own tensors (no copy)."""
    import transformers as tf

    kw = dict(hidden_size=H, num_experts_per_tok=k, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=32)
    if kind == "mixtral":
        from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock as Block
        cfg = tf.MixtralConfig(num_local_experts=E, intermediate_size=I, **kw)
    else:
        from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeSparseMoeBlock as Block
        cfg = tf.Qwen3MoeConfig(num_experts=E, moe_intermediate_size=I, intermediate_size=I, norm_topk_prob=True, **kw)
    blocks = []
    for router, gate_up, down in layers:
        with torch.device("meta"):
            b = Block(cfg).to(torch.bfloat16).eval()
        b.load_state_dict({"gate.weight": router, "experts.gate_up_proj": gate_up, "experts.down_proj": down}, assign=True)
        blocks.append(b)
    return blocks


def shape_table(name, kind, E, k, H, I, rows, rounds, eager, out):
    from hydragen_amd import moe

    expert_bytes = 3 * H * I * 2
    n = max(2, RING_BYTES // (min(E, k * min(rows)) * expert_bytes) + 2)
    gen = torch.Generator(device=DEV).manual_seed(E + H)
    mk = lambda *s, sd: torch.randn(s, device=DEV, dtype=torch.bfloat16, generator=gen) * sd  # noqa: E731
    layers = [(mk(E, H, sd=0.05), mk(E, 2 * I, H, sd=0.02), mk(E, H, I, sd=0.02)) for _ in range(n)]
    blocks, why = None, "skipped"
    if eager:
        try:
            blocks = hf_blocks(kind, layers, E, k, H, I)
        except Exception as e:  # the comparison is information: say why it is missing
            why = f"failed: {type(e).__name__}"
    out(f"### {name}: E = {E}, k = {k}, H = {H}, I = {I} ({n} layers per ring, {E * expert_bytes / 2**20:.0f} MiB of experts per layer)\n")
    out("| T | moe_mlp us | distinct experts hit | floor us (8 TB/s) | moe_mlp / floor | TB/s | transformers eager us | moe_mlp / eager |")
    out("|---|---|---|---|---|---|---|---|")
    for T in rows:
        x = torch.randn((T, H), device=DEV, dtype=torch.bfloat16, generator=gen)
        hit = statistics.mean(int(moe.moe_mlp(x, *l, k, True, return_routing=True)[1].unique().numel()) for l in layers)

        def run():
            for l in layers:
                moe.moe_mlp(x, *l, k, True)

        g = graph_of(run)
        replay_us(g, n, 1)
        us = statistics.median(replay_us(g, n) for _ in range(rounds))
        floor = hit * expert_bytes / (HBM_TBS * 1e6)
        eager_us = None
        if blocks is not None:
            try:
                ts = []
                with torch.no_grad():
                    for _ in range(rounds + 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for b in blocks:
                            b(x[None])
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e6 / n)
                eager_us = statistics.median(ts[1:])
            except Exception as e:
                blocks, why = None, f"failed: {type(e).__name__}"
        out(f"| {T} | {us:.1f} | {hit:.1f} | {floor:.1f} | {us / floor:.2f} | {hit * expert_bytes / us * 1e-6:.2f} | "
            + (f"{eager_us:.0f} | {us / eager_us:.3f} |" if eager_us else f"{why} | - |"))
        del g
    out("")


def fp8_table(name, E, k, H, I, rows, rounds, out):
    from hydragen_amd import moe

    expert_bytes = 3 * H * I * 2
    n = max(2, RING_BYTES // (min(E, k * min(rows)) * expert_bytes // 2) + 2)  # the fp8 ring, too, exceeds the Infinity Cache
    gen = torch.Generator(device=DEV).manual_seed(E + H)
    mk = lambda *s, sd: torch.randn(s, device=DEV, dtype=torch.bfloat16, generator=gen) * sd  # noqa: E731
    layers = [(mk(E, H, sd=0.05), mk(E, 2 * I, H, sd=0.02), mk(E, H, I, sd=0.02)) for _ in range(n)]
    quant = [moe.quantize_experts(gate_up, down) for _, gate_up, down in layers]
    out(f"### {name}: E = {E}, k = {k}, H = {H}, I = {I} ({n} layers per ring)\n")
    out("| T | 16-bit us (min .. max) | fp8 us (min .. max) | fp8 / 16-bit | distinct experts hit | fp8 floor us (8 TB/s) | fp8 / floor | fp8 TB/s |")
    out("|---|---|---|---|---|---|---|---|")
    for T in rows:
        x = torch.randn((T, H), device=DEV, dtype=torch.bfloat16, generator=gen)
        hit = statistics.mean(int(moe.moe_mlp(x, *l, k, True, return_routing=True)[1].unique().numel()) for l in layers)

        def run16():
            for l in layers:
                moe.moe_mlp(x, *l, k, True)

        def run8():
            for (router, _, _), q in zip(layers, quant):
                moe.moe_mlp(x, router, q[0], q[2], k, True, gate_up_scale=q[1], down_scale=q[3])

        graphs = [graph_of(run16), graph_of(run8)]
        ts = ([], [])
        for r in range(rounds + 1):
            for i, g in enumerate(graphs):
                t = replay_us(g, n, 1 if r == 0 else 20)
                if r:
                    ts[i].append(t)
        us16, us8 = (statistics.median(t) for t in ts)
        floor = hit * expert_bytes / 2 / (HBM_TBS * 1e6)
        out(f"| {T} | {us16:.1f} ({min(ts[0]):.1f} .. {max(ts[0]):.1f}) | {us8:.1f} ({min(ts[1]):.1f} .. {max(ts[1]):.1f}) | {us8 / us16:.2f} | {hit:.1f} | {floor:.1f} | "
            f"{us8 / floor:.2f} | {hit * expert_bytes / 2 / us8 * 1e-6:.2f} |")
        del graphs
    out("")


def fp4_table(name, E, k, H, I, rows, rounds, out):
    from hydragen_amd import moe

    expert_bytes = 3 * H * I * 2
    expert4_bytes = 3 * H * I * 17 // 32 + 4 * (2 * I + H)  # codes + shifts, and the channels' scales
    n = max(2, RING_BYTES // (min(E, k * min(rows)) * expert4_bytes) + 2)  # the 4-bit ring, too, exceeds the Infinity Cache
    gen = torch.Generator(device=DEV).manual_seed(E + H)
    mk = lambda *s, sd: torch.randn(s, device=DEV, dtype=torch.bfloat16, generator=gen) * sd  # noqa: E731
    layers = [(mk(E, H, sd=0.05), mk(E, 2 * I, H, sd=0.02), mk(E, H, I, sd=0.02)) for _ in range(n)]
    quant8 = [moe.quantize_experts(gate_up, down) for _, gate_up, down in layers]
    # (expert by expert: the quantizer's float64 temporaries of a whole Mixtral layer would not be small)
    quant4 = [tuple(torch.cat(t) for t in zip(*(moe.quantize_experts_fp4(gate_up[e:e + 1], down[e:e + 1]) for e in range(E)))) for _, gate_up, down in layers]
    out(f"### {name}: E = {E}, k = {k}, H = {H}, I = {I} ({n} layers per ring; resident experts per layer: {E * expert_bytes / 2**20:.0f} MiB in 16 bits, "
        f"{E * expert_bytes / 2**21:.0f} MiB in fp8, {E * expert4_bytes / 2**20:.0f} MiB in 4 bits)\n")
    out("| T | 16-bit us (min .. max) | fp8 us (min .. max) | 4-bit us (min .. max) | 4-bit / fp8 | 4-bit / 16-bit | distinct experts hit | 4-bit floor us (8 TB/s) | 4-bit / floor | 4-bit TB/s |")
    out("|---|---|---|---|---|---|---|---|---|---|")
    for T in rows:
        x = torch.randn((T, H), device=DEV, dtype=torch.bfloat16, generator=gen)
        hit = statistics.mean(int(moe.moe_mlp(x, *l, k, True, return_routing=True)[1].unique().numel()) for l in layers)

        def run16():
            for l in layers:
                moe.moe_mlp(x, *l, k, True)

        def run8():
            for (router, _, _), q in zip(layers, quant8):
                moe.moe_mlp(x, router, q[0], q[2], k, True, gate_up_scale=q[1], down_scale=q[3])

        def run4():
            for (router, _, _), q in zip(layers, quant4):
                moe.moe_mlp(x, router, q[0], q[3], k, True, gate_up_shift=q[1], gate_up_scale=q[2], down_shift=q[4], down_scale=q[5])

        graphs = [graph_of(run16), graph_of(run8), graph_of(run4)]
        ts = ([], [], [])
        for r in range(rounds + 1):
            for i, g in enumerate(graphs):
                t = replay_us(g, n, 1 if r == 0 else 20)
                if r:
                    ts[i].append(t)
        us16, us8, us4 = (statistics.median(t) for t in ts)
        floor = hit * expert4_bytes / (HBM_TBS * 1e6)
        spread = lambda i: f"({min(ts[i]):.1f} .. {max(ts[i]):.1f})"  # noqa: E731
        out(f"| {T} | {us16:.1f} {spread(0)} | {us8:.1f} {spread(1)} | {us4:.1f} {spread(2)} | {us4 / us8:.2f} | {us4 / us16:.2f} | {hit:.1f} | {floor:.1f} | "
            f"{us4 / floor:.2f} | {hit * expert4_bytes / us4 * 1e-6:.2f} |")
        del graphs
    out("")


def grouped_table(name, E, k, H, I, rows, rounds, out):
    from hydragen_amd import moe

    expert_bytes = 3 * H * I * 2
    n = max(2, RING_BYTES // (min(E, k * min(rows)) * expert_bytes) + 2)
    gen = torch.Generator(device=DEV).manual_seed(E + H)
    mk = lambda *s, sd: torch.randn(s, device=DEV, dtype=torch.bfloat16, generator=gen) * sd  # noqa: E731
    layers = [(mk(E, H, sd=0.05), mk(E, 2 * I, H, sd=0.02), mk(E, H, I, sd=0.02)) for _ in range(n)]
    out(f"### {name}: E = {E}, k = {k}, H = {H}, I = {I} ({n} layers per ring, {E * expert_bytes / 2**20:.0f} MiB of experts per layer)\n")
    out("| T | chunked us (min .. max) | grouped us (min .. max) | chunked / grouped | distinct experts hit | byte floor us (8 TB/s) | FLOP floor us (2.5 PFLOP/s) | "
        "grouped / byte floor | grouped / FLOP floor |")
    out("|---|---|---|---|---|---|---|---|---|")
    for T in rows:
        x = torch.randn((T, H), device=DEV, dtype=torch.bfloat16, generator=gen)
        y = torch.empty_like(x)
        hit = statistics.mean(int(moe.moe_mlp(x, *l, k, True, return_routing=True)[1].unique().numel()) for l in layers)

        def run_chunked():
            for router, gate_up, down in layers:
                logits = torch.nn.functional.linear(x, router)
                for r in range(0, T, moe.MOE_MAX_ROWS):
                    moe.moe_rows(x[r:r + moe.MOE_MAX_ROWS], logits[r:r + moe.MOE_MAX_ROWS], gate_up, down, k, True, y[r:r + moe.MOE_MAX_ROWS])

        def run_grouped():
            for router, gate_up, down in layers:
                moe.moe_rows_grouped(x, torch.nn.functional.linear(x, router), gate_up, down, k, True, y)

        graphs = [graph_of(run_chunked), graph_of(run_grouped)]
        ts = ([], [])
        for r in range(rounds + 1):
            for i, g in enumerate(graphs):
                t = replay_us(g, n, 1 if r == 0 else 10)
                if r:
                    ts[i].append(t)
        usc, usg = (statistics.median(t) for t in ts)
        floor_b, floor_f = hit * expert_bytes / (HBM_TBS * 1e6), 2 * T * k * 3 * H * I / (BF16_PFLOPS * 1e9)
        spread = lambda i: f"({min(ts[i]):.1f} .. {max(ts[i]):.1f})"  # noqa: E731
        out(f"| {T} | {usc:.1f} {spread(0)} | {usg:.1f} {spread(1)} | {usc / usg:.2f} | {hit:.1f} | {floor_b:.1f} | {floor_f:.1f} | {usg / floor_b:.2f} | "
            f"{usg / floor_f:.2f} |")
        del graphs
    out("")


def grouped_fp8_table(name, E, k, H, I, rows, rounds, out):
    from hydragen_amd import moe

    expert_bytes = 3 * H * I  # codes
    n = max(2, RING_BYTES // (min(E, k * min(rows)) * expert_bytes) + 2)  # the fp8 ring, too, exceeds the Infinity Cache
    gen = torch.Generator(device=DEV).manual_seed(E + H)
    mk = lambda *s, sd: torch.randn(s, device=DEV, dtype=torch.bfloat16, generator=gen) * sd  # noqa: E731
    layers = [(mk(E, H, sd=0.05), mk(E, 2 * I, H, sd=0.02), mk(E, H, I, sd=0.02)) for _ in range(n)]
    quant = [moe.quantize_experts(gate_up, down) for _, gate_up, down in layers]
    out(f"### {name}: E = {E}, k = {k}, H = {H}, I = {I} ({n} layers per ring, {E * expert_bytes / 2**20:.0f} MiB of fp8 experts per layer)\n")
    out("| T | chunked fp8 us (min .. max) | grouped fp8 us (min .. max) | grouped 16-bit us (min .. max) | chunked fp8 / grouped fp8 | grouped 16-bit / grouped fp8 | "
        "distinct experts hit | fp8 byte floor us (8 TB/s) | FLOP floor us (2.5 PFLOP/s) | grouped fp8 / FLOP floor |")
    out("|---|---|---|---|---|---|---|---|---|---|")
    for T in rows:
        x = torch.randn((T, H), device=DEV, dtype=torch.bfloat16, generator=gen)
        y = torch.empty_like(x)
        hit = statistics.mean(int(moe.moe_mlp(x, *l, k, True, return_routing=True)[1].unique().numel()) for l in layers)

        def run_chunked8():
            for (router, _, _), q in zip(layers, quant):
                logits = torch.nn.functional.linear(x, router)
                for r in range(0, T, moe.MOE_MAX_ROWS):
                    moe.moe_rows_w8(x[r:r + moe.MOE_MAX_ROWS], logits[r:r + moe.MOE_MAX_ROWS], *q, k, True, y[r:r + moe.MOE_MAX_ROWS])

        def run_grouped8():
            for (router, _, _), q in zip(layers, quant):
                moe.moe_rows_grouped_w8(x, torch.nn.functional.linear(x, router), *q, k, True, y)

        def run_grouped16():
            for router, gate_up, down in layers:
                moe.moe_rows_grouped(x, torch.nn.functional.linear(x, router), gate_up, down, k, True, y)

        graphs = [graph_of(run_chunked8), graph_of(run_grouped8), graph_of(run_grouped16)]
        ts = ([], [], [])
        for r in range(rounds + 1):
            for i, g in enumerate(graphs):
                t = replay_us(g, n, 1 if r == 0 else 10)
                if r:
                    ts[i].append(t)
        usc, us8, us16 = (statistics.median(t) for t in ts)
        floor_b, floor_f = hit * expert_bytes / (HBM_TBS * 1e6), 2 * T * k * 3 * H * I / (BF16_PFLOPS * 1e9)
        spread = lambda i: f"({min(ts[i]):.1f} .. {max(ts[i]):.1f})"  # noqa: E731
        out(f"| {T} | {usc:.1f} {spread(0)} | {us8:.1f} {spread(1)} | {us16:.1f} {spread(2)} | {usc / us8:.2f} | {us16 / us8:.2f} | {hit:.1f} | {floor_b:.1f} | "
            f"{floor_f:.1f} | {us8 / floor_f:.2f} |")
        del graphs
    out("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default=None, help="default 1,8,32,128; --experts grouped / grouped_fp8: 256,512,1024,2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--experts", choices=["16bit", "fp8", "fp4", "grouped", "grouped_fp8"], default="16bit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench.py measures on the GPU: no device found")
    fp8, fp4, grouped, grouped8 = args.experts == "fp8", args.experts == "fp4", args.experts == "grouped", args.experts == "grouped_fp8"
    args.rows = args.rows or ("256,512,1024,2048" if grouped or grouped8 else "1,8,32,128")
    lines = Path(args.out).read_text().rstrip("\n").split("\n") + [""] if (fp8 or fp4 or grouped or grouped8) and args.out and Path(args.out).exists() else []

    def out(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            Path(args.out).write_text("\n".join(lines) + "\n")

    if grouped8:
        out("## Large calls on fp8 experts: the grouped call (`hyd_moe_mlp_grouped_w8`) against the chunked fp8 route and the 16-bit grouped call\n")
        out("`moe_rows_w8` per 128 rows, `moe_rows_grouped_w8` once, and `moe_rows_grouped` once on the 16-bit originals, each behind the router GEMM, all "
            "captured and replayed alternately in one process on a ring of distinct layers, bf16 activations; median (min .. max) over the rounds, per layer.  "
            "Floors: the activated experts' code bytes at 8 TB/s, and 2 T k 3 H I FLOPs at the dense bf16 peak.\n")
        for name, _, E, k, H, I in SHAPES:
            grouped_fp8_table(name, E, k, H, I, [int(r) for r in args.rows.split(",")], args.rounds, out)
            torch.cuda.empty_cache()
        return
    if grouped:
        out("## Large calls: the grouped call (`hyd_moe_mlp_grouped`) against the chunked route of the same build\n")
        out("`moe_rows_grouped` once and `moe_rows` per 128 rows, each behind the router GEMM, both captured and replayed alternately in one process on a "
            "ring of distinct layers, bf16; median (min .. max) over the rounds, per layer.  Floors: the activated experts' bytes at 8 TB/s, and "
            "2 T k 3 H I FLOPs at the dense bf16 peak.\n")
        for name, _, E, k, H, I in SHAPES:
            grouped_table(name, E, k, H, I, [int(r) for r in args.rows.split(",")], args.rounds, out)
            torch.cuda.empty_cache()
        return
    if fp4:
        out("## 4-bit experts (`hyd_moe_mlp_w4`) against the fp8 and the 16-bit kernels of the same build\n")
        out("The same rings in three forms (`moe.quantize_experts`, `moe.quantize_experts_fp4`), all captured and replayed alternately in one process, bf16 "
            "activations; median (min .. max) over the rounds, per layer.  The 4-bit floor is the activated experts' codes, shifts and scales at 8 TB/s.\n")
        for name, _, E, k, H, I in SHAPES:
            fp4_table(name, E, k, H, I, [int(r) for r in args.rows.split(",")], args.rounds, out)
            torch.cuda.empty_cache()
        return
    if fp8:
        out("## fp8 experts (`hyd_moe_mlp_w8`) against the 16-bit kernels of the same build\n")
        out("The same rings with their experts quantized (`moe.quantize_experts`), both forms captured and replayed alternately in one process, bf16 "
            "activations; median (min .. max) over the rounds, per layer.  The fp8 floor is the activated experts' code bytes at 8 TB/s.\n")
        for name, _, E, k, H, I in SHAPES:
            fp8_table(name, E, k, H, I, [int(r) for r in args.rows.split(",")], args.rounds, out)
            torch.cuda.empty_cache()
        return
    out("# Mixture-of-experts MLP: measurements\n")
    out("One layer's `moe_mlp` (router GEMM, then route / group / gate|up + SwiGLU / down / combine) under a HIP graph, bf16, per layer of a ring "
        "of distinct layers; the floor is the bytes of the distinct activated experts at 8 TB/s.\n")
    for name, kind, E, k, H, I in SHAPES:
        shape_table(name, kind, E, k, H, I, [int(r) for r in args.rows.split(",")], args.rounds, not args.skip_eager, out)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
