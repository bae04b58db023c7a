"""A/B of bf16 against fp8 (e4m3fn) unique K/V caches: one process, the same arenas' shapes, alternating repeats.

    python tools/fp8_kv_ab.py [--reps 5] [--iters 20] [--out profiles/fp8_kv_ab.md]

For every shape it times (device events around the replay of a HIP graph holding `iters` calls -- no host work in the timed
window -- median of `reps` alternating repeats):
  suffix  the suffix pass alone (flash_attention_seqlen): the kernel fp8 replaces;
  TB/s    the bytes that pass actually streams (K + V rows up to each length, q, out, lse) over its time;
  step    the whole decode-step operator (hydragen_attention_nopad) with a 16-bit shared prefix of P rows.
Rows: C2 (B 1024, 32 / 32 heads, D 128, P 2048) at S 1 / 16 / 64 / 128 and averaged over bench.suffix_schedule, the TP = 8
shard (4 / 4 heads), D 64 and D 256, a 2176-row cache without a shared prefix, and few (sequence, head) units with long caches
(B = 1 and B = 8 at 2048 rows: the fp8 kernel has one wave per 4 heads of a sequence there).  The unique caches are arenas of the
model's layout and placement policy (placement.place_kv_arenas), bf16 and fp8 alike.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from bench import suffix_schedule  # noqa: E402
from hydragen_amd import placement  # noqa: E402
from hydragen_amd.attention import hydragen_attention_nopad  # noqa: E402
from hydragen_amd.flash import flash_attention_seqlen  # noqa: E402
from hydragen_amd.kv_quant import quantize_kv  # noqa: E402

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn


def _graph(fn, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # warm-up outside the capture (library load, cached shape queries)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    return g


def _time(g, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def run_shape(name, B, H, D, cap, lens, P, reps, iters):
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    q = torch.randn((B, 1, H, D), generator=g, device=DEV).to(torch.bfloat16)
    (a16,), _ = placement.place_kv_arenas(1, (B, cap, H, D), torch.bfloat16, DEV, H, zero=False)
    (a8,), _ = placement.place_kv_arenas(1, (B, cap, H, D), FP8, DEV, H, zero=False, q_dtype=torch.bfloat16)
    for i in range(2):
        x = torch.randn((B, cap, H, D), generator=g, device=DEV).to(torch.bfloat16)
        a16[i].copy_(x)
        a8[i].view(torch.uint8).copy_(quantize_kv(x).view(torch.uint8))
        del x
    k16, v16, k8, v8 = a16[0], a16[1], a8[0], a8[1]
    ks = torch.ones(H, device=DEV)
    vs = torch.ones(H, device=DEV)
    sk = torch.randn((1, P, H, D), generator=g, device=DEV).to(torch.bfloat16) if P else None
    sv = torch.randn((1, P, H, D), generator=g, device=DEV).to(torch.bfloat16) if P else None
    res = {"bf16": {"suffix": [], "step": []}, "fp8": {"suffix": [], "step": []}}
    for S in lens:
        sl = torch.full((B,), S, dtype=torch.int32, device=DEV)
        variants = {
            "bf16": (lambda: flash_attention_seqlen(q, k16, v16, sl),
                     lambda: hydragen_attention_nopad(q, k16, v16, [sk], [sv], sl)),
            "fp8": (lambda: flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs),
                    lambda: hydragen_attention_nopad(q, k8, v8, [sk], [sv], sl, k_scale=ks, v_scale=vs)),
        }
        t = {v: {"suffix": [], "step": []} for v in variants}
        graphs = {v: (_graph(suf, iters), _graph(step, iters) if P else None) for v, (suf, step) in variants.items()}
        for _ in range(reps):
            for v, (gs, gt) in graphs.items():  # alternating
                t[v]["suffix"].append(_time(gs, iters))
                if P:
                    t[v]["step"].append(_time(gt, iters))
        del graphs
        for v in variants:
            res[v]["suffix"].append(statistics.median(t[v]["suffix"]))
            res[v]["step"].append(statistics.median(t[v]["step"]) if P else float("nan"))
    rows = []
    mean_len = sum(lens) / len(lens)
    for v, esz in (("bf16", 2), ("fp8", 1)):
        suf = sum(res[v]["suffix"]) / len(lens)
        step = sum(res[v]["step"]) / len(lens)
        streamed = B * H * D * (2 * mean_len * esz + 2 * 2) + B * H * 4
        rows.append((name, v, suf, streamed / (suf * 1e-6) / 1e12, step))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fp8_kv_ab.py measures on the GPU"
    sched = suffix_schedule(16, 128)
    shapes = [(f"C2 S={S}", 1024, 32, 128, 128, [S], 2048) for S in (1, 16, 64, 128)]
    shapes += [("C2 bench schedule (mean S %.1f)" % (sum(sched) / len(sched)), 1024, 32, 128, 128, sched, 2048),
               ("TP=8 shard 4/4 heads S=64", 1024, 4, 128, 128, [64], 2048),
               ("TP=8 shard 4/4 heads S=16", 1024, 4, 128, 128, [16], 2048),
               ("D=64 32 heads S=16", 1024, 32, 64, 128, [16], 2048),
               ("D=64 32 heads S=64", 1024, 32, 64, 128, [64], 2048),
               ("D=256 16 heads S=64", 1024, 16, 256, 128, [64], 2048),
               ("2176-row cache, no sharing", 64, 32, 128, 2176, [2176], 0),
               ("few units: B=1, 32 heads, 2048 rows", 1, 32, 128, 2048, [2048], 0),
               ("few units: B=8, 32 heads, 2048 rows", 8, 32, 128, 2048, [2048], 0)]
    lines = ["| shape | cache | suffix us | TB/s streamed | step us | fp8 speed-up (suffix) |", "|---|---|---|---|---|---|"]
    for sh in shapes:
        rows = run_shape(*sh, a.reps, a.iters)
        sp = rows[0][2] / rows[1][2]
        for r in rows:
            lines.append(f"| {r[0]} | {r[1]} | {r[2]:.1f} | {r[3]:.2f} | {r[4]:.1f} | {sp:.2f}x |" if r[1] == "fp8" else
                         f"| {r[0]} | {r[1]} | {r[2]:.1f} | {r[3]:.2f} | {r[4]:.1f} | |")
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
