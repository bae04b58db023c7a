#!/usr/bin/env python3
"""Scoring benchmarks, in one process.

  kernel:  hyd_token_logprobs over [R, V] bf16 logits against the torch route it replaces (log_softmax(x.float()) + gather +
           argmax + topk), HIP events after warm-up, the two forms alternating per shape.
  model:   score() on Llama-2-7B random weights: a shared 2048-token prefix (batch 1) and B unique 16-token continuations with
           ragged target_lens 1..16; against the same call with disable_hydragen=True (at --base-batch sequences: its
           per-sequence prefix copy takes 0.5 MB per token and layer) and the teacher-forced generate(token_overrides=,
           return_logits=True) route + log_softmax; in target tokens scored per second.

    python tools/score_bench.py [--part kernel,model] [--rows 1024,8192] [--vocabs 32000,128256] [--tops 0,5,20]
Prints one JSON line per measurement."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from hydragen_amd import layer_ops

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="kernel,model")
ap.add_argument("--rows", default="1024,8192")
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--tops", default="0,5,20")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--base-batch", type=int, default=64)
ap.add_argument("--prefix", type=int, default=2048)
ap.add_argument("--layers", type=int, default=32)
a = ap.parse_args()
dev = "cuda:0"


def timed(fn, iters=None):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters or a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def torch_route(x, t, n):
    lp = torch.log_softmax(x.float(), -1)
    out = (lp.gather(1, t[:, None]), lp.argmax(-1) == t)
    return out + (torch.topk(lp, n, -1),) if n else out


if "kernel" in a.part:
    for V in map(int, a.vocabs.split(",")):
        for R in map(int, a.rows.split(",")):
            g = torch.Generator(device=dev).manual_seed(R + V)
            x = (torch.randn(R, V, device=dev, generator=g) * 3).to(torch.bfloat16)
            t = torch.randint(0, V, (R,), device=dev, generator=g)
            for n in map(int, a.tops.split(",")):
                res = {}
                for rep in range(2):  # alternate the two forms
                    for name, fn in (("hip", lambda: layer_ops.token_logprobs(x, t, n)), ("torch", lambda: torch_route(x, t, n))):
                        res.setdefault(name, []).append(timed(fn))
                for name, v in res.items():
                    med = min(m for m, _ in v)
                    best = min(b for _, b in v)
                    print(json.dumps({"part": "kernel", "rows": R, "V": V, "top_n": n, "path": name, "us_median": round(med, 1),
                                      "us_min": round(best, 1), "logit_GB": round(R * V * 2 / 1e9, 3),
                                      "GBps_of_16bit_logits": round(R * V * 2 / med / 1e3, 1)}), flush=True)
            del x
            torch.cuda.empty_cache()

if "model" in a.part:
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig.llama2_7b(num_hidden_layers=a.layers)
    model = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=dev, seed=0)
    B, L, P = a.batch, 16, a.prefix
    g = torch.Generator(device=dev).manual_seed(1)
    prefix = torch.randint(1, cfg.vocab_size, (1, P), device=dev, generator=g)
    uids = torch.randint(1, cfg.vocab_size, (B, L), device=dev, generator=g)
    tl = torch.randint(1, L + 1, (B,), device=dev, generator=g).clamp(max=L - 1)  # >= 1 context token for the decode route

    def run_score(b, **kw):
        return model.score([prefix, uids[:b]], tl[:b], **kw)

    def run_teacher(b):
        ctx_len = L - tl[:b]
        ctx = uids[:b, : int(ctx_len.max())]
        T = int(tl[:b].max())
        over = torch.zeros((b, T), dtype=torch.long, device=dev)
        for i in range(b):
            c, n = int(ctx_len[i]), int(tl[i])
            over[i, :n] = uids[i, c : c + n]
        _, logits = model.generate(input_ids=[prefix, ctx], seq_lens=[torch.tensor([P], device=dev), ctx_len], max_new_tokens=T,
                                   temperature=0.0, token_overrides=over, return_logits=True)
        return [torch.log_softmax(lg, -1).gather(1, over[:, j : j + 1]) for j, lg in enumerate(logits)]

    def wall(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    # (cache batch, cache rows): the hydragen forms keep only the continuations per sequence; the no-sharing form copies the
    # prefix into every sequence's cache, so it runs at --base-batch
    legs = [((B, 2 * L), [("score", B, lambda: run_score(B)), ("score_top5", B, lambda: run_score(B, top_logprobs=5)),
                          ("teacher_forced_generate", B, lambda: run_teacher(B))]),
            ((a.base_batch, P + 2 * L), [("score", a.base_batch, lambda: run_score(a.base_batch)),
                                         ("score_disable_hydragen", a.base_batch, lambda: run_score(a.base_batch, disable_hydragen=True))])]
    for (cb, rows), runs in legs:
        model.setup_caches(max_unique_batch_size=cb, max_unique_seq_length=rows, max_shared_batch_sizes=[1], max_shared_seq_lengths=[P])
        for name, b, fn in runs:
            s = wall(fn)
            toks = int(tl[:b].sum())
            print(json.dumps({"part": "model", "path": name, "batch": b, "prefix": P, "layers": a.layers, "target_tokens": toks,
                              "seconds": round(s, 4), "tokens_per_s": round(toks / s, 1)}), flush=True)
