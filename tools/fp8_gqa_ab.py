"""A/B of fp8 (e4m3fn) unique K/V caches on grouped-query heads: one process, placed arenas, graph replays, alternating repeats.

    python tools/fp8_gqa_ab.py [--reps 7] [--iters 20] [--out profiles/fp8_gqa_ab.md]

For every shape and suffix length S (all sequences S keys long) it times the suffix pass (flash_attention_seqlen) in three variants
-- device events around the replay of a HIP graph holding `iters` calls, median of `reps` repeats, the variants alternating:
  (a) the 16-bit grouped-query kernel on 16-bit caches;
  (b) what fp8 caches cost before the fp8 grouped-query kernel: dequantize_kv of both caches, then the 16-bit kernel;
  (c) the fp8 grouped-query kernel (csrc/suffix_attn_gqa_fp8.hip) on the fp8 caches.
It prints (a)'s run-to-run spread (min .. max of the repeats) as the margin of the comparison, the TB/s of fp8 K/V bytes (c)
streams, and the peak device memory one call of (b) and of (c) adds.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from hydragen_amd import placement  # noqa: E402
from hydragen_amd.flash import flash_attention_seqlen, fp8_native  # noqa: E402
from hydragen_amd.kv_quant import dequantize_kv, quantize_kv  # noqa: E402
from tools.fp8_kv_ab import _graph, _time  # noqa: E402

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
LENS = (32, 64, 128, 256)
# the C5 whole job is bench.py --workload c5's own batch and heads
SHAPES = [("C5 whole job", 2048, 64, 8, 128), ("C5 TP=8 slice", 2048, 8, 1, 128), ("C3", 64, 32, 8, 128),
          ("D=64, 8/2 heads", 1024, 8, 2, 64), ("D=256, 8/1 heads", 2048, 8, 1, 256)]


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run_shape(name, B, Hq, Hkv, D, reps, iters):
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    cap = max(LENS)
    q = torch.randn((B, 1, Hq, D), generator=g, device=DEV).to(torch.bfloat16)
    (a16,), _ = placement.place_kv_arenas(1, (B, cap, Hkv, D), torch.bfloat16, DEV, Hq, zero=False)
    (a8,), _ = placement.place_kv_arenas(1, (B, cap, Hkv, D), FP8, DEV, Hq, zero=False, q_dtype=torch.bfloat16)
    ks = (0.5 + torch.rand(Hkv, generator=g, device=DEV)).float()
    vs = (0.5 + torch.rand(Hkv, generator=g, device=DEV)).float()
    for i, sc in enumerate((ks, vs)):
        x = torch.randn((B, cap, Hkv, D), generator=g, device=DEV).to(torch.bfloat16)
        a16[i].copy_(x)
        a8[i].view(torch.uint8).copy_(quantize_kv(x, sc).view(torch.uint8))
        del x
    k16, v16, k8, v8 = a16[0], a16[1], a8[0], a8[1]
    assert fp8_native(q, k8, v8), name
    lines = []
    for S in LENS:
        sl = torch.full((B,), S, dtype=torch.int32, device=DEV)
        variants = {
            "a": lambda: flash_attention_seqlen(q, k16, v16, sl),
            "b": lambda: flash_attention_seqlen(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), sl),
            "c": lambda: flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs),
        }
        graphs = {v: _graph(fn, iters) for v, fn in variants.items()}
        t = {v: [] for v in variants}
        for _ in range(reps):
            for v, gr in graphs.items():  # alternating
                t[v].append(_time(gr, iters))
        del graphs
        med = {v: statistics.median(t[v]) for v in variants}
        tbs = 2.0 * B * Hkv * S * D / (med["c"] * 1e-6) / 1e12
        verdict = "ok" if med["c"] < med["b"] and med["c"] <= max(t["a"]) else "FAILS"
        lines.append(f"| {name} | {B} | {Hq}/{Hkv} | {D} | {S} | {med['a']:.1f} ({min(t['a']):.1f} .. {max(t['a']):.1f}) | {med['b']:.1f} | "
                     f"{med['c']:.1f} | {med['b'] / med['c']:.2f}x | {med['a'] / med['c']:.2f}x | {tbs:.2f} | {verdict} |")
        print(lines[-1], flush=True)
    sl = torch.full((B,), max(LENS), dtype=torch.int32, device=DEV)
    pb = _peak(lambda: flash_attention_seqlen(q, dequantize_kv(k8, ks, q.dtype), dequantize_kv(v8, vs, q.dtype), sl))
    pc = _peak(lambda: flash_attention_seqlen(q, k8, v8, sl, k_scale=ks, v_scale=vs))
    mem = f"| {name} | {a8.numel() / 2**20:.0f} | {pb / 2**20:.0f} | {pc / 2**20:.0f} |"
    print(mem, flush=True)
    return lines, mem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fp8_gqa_ab.py measures on the GPU"
    head = ["| shape | B | Hq/Hkv | D | S | (a) 16-bit us (min .. max) | (b) dequantize + 16-bit us | (c) fp8 kernel us | (b)/(c) | (a)/(c) | "
            "(c) TB/s of fp8 K/V | (c) < (b) and (c) <= max (a) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    mems = ["| shape | fp8 arena MiB (K + V) | (b) peak MiB added by one call | (c) peak MiB added by one call |", "|---|---|---|---|"]
    for sh in SHAPES:
        lines, mem = run_shape(*sh, a.reps, a.iters)
        head += lines
        mems.append(mem)
        torch.cuda.empty_cache()
    text = "\n".join(head) + "\n\n" + "\n".join(mems) + "\n"
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
