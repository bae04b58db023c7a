#!/usr/bin/env python3
"""Time one sampling call over [B, V] logits with HIP events after warm-up: the plain sampler (hyd_sample_tokens), the
filtered sampler (hyd_sample_tokens_filtered) with each cut and with all three, and the torch top-p path the model shell
used before it (the reference's apply_top_p over fp32 logits + hyd_sample_tokens).

    python tools/sampler_bench.py [--batches 1,128,1024] [--vocabs 32000,128256] [--dtypes bf16,fp32] [--iters 20]
--penalties adds the penalised legs at top-p 0.95 (a 2048-token shared context, 64 generated tokens per row, a 16-entry bias):
hyd_sample_tokens_penalized with neutral penalties (what the fp32 keys and the LDS prologue cost alone), with the penalties
on, and the torch route of the model shell with fused_sampling_penalties off (sampling.penalize_logits, then the fused cuts).
--only NAME[,NAME] restricts the paths.
Prints one JSON line per (B, V, dtype, path): median and min microseconds per call."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from hydragen_amd import layer_ops
from hydragen_amd.sampling import apply_top_p  # the path with fused_sampling_filters off

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,128,1024")
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--dtypes", default="bf16,fp32")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--penalties", action="store_true")
ap.add_argument("--only", default="")
a = ap.parse_args()
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
dev = "cuda:0"


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


T = 0.7
for V in map(int, a.vocabs.split(",")):
    for B in map(int, a.batches.split(",")):
        for dn in a.dtypes.split(","):
            g = torch.Generator(device=dev).manual_seed(B + V)
            x = (torch.randn(B, V, device=dev, generator=g) * 3).to(DT[dn])
            paths = {
                "plain": lambda: layer_ops.sample_tokens(x, T),
                "fused_top_k50": lambda: layer_ops.sample_tokens(x, T, top_k=50),
                "fused_top_p0.95": lambda: layer_ops.sample_tokens(x, T, top_p=0.95),
                "fused_min_p0.05": lambda: layer_ops.sample_tokens(x, T, min_p=0.05),
                "fused_logprobs": lambda: layer_ops.sample_tokens(x, T, return_logprobs=True),
                "fused_all3_logprobs": lambda: layer_ops.sample_tokens(x, T, top_k=50, top_p=0.95, min_p=0.05, return_logprobs=True),
                # the model shell before: fp32 logits (a 16-bit row is widened first, as forward(raw_logits=False) did)
                "torch_top_p0.95": lambda: layer_ops.sample_tokens(apply_top_p(x.float(), 0.95), T),
            }
            if a.penalties:
                from hydragen_amd import sampling

                ctx_ids = torch.randint(0, V, (1, 2048), device=dev, generator=g)
                bias = sampling.normalize_logit_bias((torch.randperm(V)[:16], torch.randn(16)), dev)

                def pen(on=True):
                    return layer_ops.Penalties(
                        1.3 if on else None, 0.2 if on else None, 0.2 if on else None, bias if on else None,
                        [(layer_ops.token_bitmap(ctx_ids, None, V), B)] if on else [],
                        torch.randint(0, V, (B, 64), device=dev, generator=g).to(torch.int32),
                        torch.full((B,), 64 if on else 0, dtype=torch.int32, device=dev))

                p_on, p_off = pen(), pen(False)
                paths.update({
                    "penalized_neutral_top_p0.95": lambda: layer_ops.sample_tokens_penalized(x, T, penalties=p_off, top_p=0.95),
                    "penalized_top_p0.95": lambda: layer_ops.sample_tokens_penalized(x, T, penalties=p_on, top_p=0.95),
                    "torch_penalized_top_p0.95": lambda: layer_ops.sample_tokens(p_on.apply(x).float(), T, top_p=0.95),
                })
            if a.only:
                paths = {k: v for k, v in paths.items() if k in a.only.split(",")}
            for name, fn in paths.items():
                med, best = timed(fn)
                print(json.dumps({"B": B, "V": V, "dtype": dn, "path": name, "us_median": round(med, 1), "us_min": round(best, 1),
                                  "iters": a.iters}), flush=True)
            del x
            torch.cuda.empty_cache()
