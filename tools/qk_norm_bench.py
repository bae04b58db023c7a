"""Per-head q/k RMSNorm inside the decode preamble: what it costs against the plain preamble and against doing the norm in torch.
Writes the table of profiles/qk_norm.md (markdown, to --out or stdout) -- nothing here is promised in advance.

    python tools/qk_norm_bench.py [--out profiles/qk_norm.md] [--batch 1024] [--rounds 15] [--layers 32]

Shape: B = 1024 sequences, 32 query / 8 kv heads, D = 128, bf16; q / k / v are views into one fused q|k|v projection buffer, as in
the model.  Three candidates, each one decode step's preambles of `--layers` layers (distinct projection buffers and caches per
layer) captured in a HIP graph (device time, no launch gaps); the graphs' replays alternate in one process, round after round:
  (a) hyd_rope_append_decode                                           -- the existing preamble, no norm;
  (b) hyd_rope_append_decode_qkn                                       -- the norm inside the preamble;
  (c) F.rms_norm over the q view, F.rms_norm over the k view, then (a) -- the norm as two torch launches in front of it.
The figure is microseconds per layer: median over the rounds, with the rounds' minimum and maximum as the spread."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEV = "cuda:0"


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


def replay_us(g, calls, reps=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qk_norm_bench.py measures on the GPU; none is visible")
    from hydragen_amd.fused_decode import rope_append_decode
    from hydragen_amd.llama import RotaryTable

    B, Hq, Hkv, D, S, dtype, eps = a.batch, 32, 8, 128, 16, torch.bfloat16, 1e-6
    g = torch.Generator(device=DEV).manual_seed(0)
    rot = RotaryTable(D, 4096, 10000.0, device=DEV)
    cos, sin = rot.cos_cached, rot.sin_cached
    shared = torch.full((B,), 2048, dtype=torch.int64, device=DEV)
    pos = (shared + torch.randint(0, S, (B,), device=DEV, generator=g))[:, None].contiguous()
    qw = (1 + 0.3 * torch.randn(D, device=DEV, generator=g)).to(dtype)
    kw = (1 + 0.3 * torch.randn(D, device=DEV, generator=g)).to(dtype)
    layers = []
    for _ in range(a.layers):
        qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, device=DEV, dtype=dtype, generator=g)
        layers.append((qkv[..., : Hq * D].view(B, 1, Hq, D), qkv[..., Hq * D: (Hq + Hkv) * D].view(B, 1, Hkv, D),
                       qkv[..., (Hq + Hkv) * D:].view(B, 1, Hkv, D), torch.zeros(B, S, Hkv, D, device=DEV, dtype=dtype),
                       torch.zeros(B, S, Hkv, D, device=DEV, dtype=dtype)))

    def plain():
        for q, k, v, kc, vc in layers:
            rope_append_decode(q, k, v, cos, sin, pos, shared, kc, vc)

    def fused():
        for q, k, v, kc, vc in layers:
            rope_append_decode(q, k, v, cos, sin, pos, shared, kc, vc, q_norm=qw, k_norm=kw, norm_eps=eps)

    def torch_norm():
        for q, k, v, kc, vc in layers:
            qn = torch.nn.functional.rms_norm(q, (D,), qw, eps)
            kn = torch.nn.functional.rms_norm(k, (D,), kw, eps)
            rope_append_decode(qn, kn, v, cos, sin, pos, shared, kc, vc)

    cands = [("(a) existing preamble, no norm", plain), ("(b) norm inside the preamble", fused), ("(c) 2 x F.rms_norm, then (a)", torch_norm)]
    # the candidates that compute the norm agree (the torch form rounds the normalised row to bf16 before the rotation: 1 ulp apart)
    q, k, v, kc, vc = layers[0]
    qb, _ = rope_append_decode(q, k, v, cos, sin, pos, shared, kc, vc, q_norm=qw, k_norm=kw, norm_eps=eps)
    qc, _ = rope_append_decode(torch.nn.functional.rms_norm(q, (D,), qw, eps), torch.nn.functional.rms_norm(k, (D,), kw, eps), v, cos, sin, pos,
                               shared, kc.clone(), vc.clone())
    agree = float((qb.float() - qc.float()).abs().max())
    graphs = [(name, graph_of(fn)) for name, fn in cands]
    for _, gr in graphs:  # warm
        replay_us(gr, a.layers, reps=3)
    times = {name: [] for name, _ in graphs}
    for _ in range(a.rounds):
        for name, gr in graphs:
            times[name].append(replay_us(gr, a.layers))
    moved = B * ((2 * Hq + 3 * Hkv) * D * 2 + Hkv * D * 2)  # q in + out, k in + out, v in + out (bf16)
    lines = [f"Shape: B = {B}, {Hq} / {Hkv} heads, D = {D}, bf16, {a.layers} layers per graph replay, {a.rounds} alternating rounds of 5 replays; "
             f"{moved / 1e6:.1f} MB moved per layer by (a) and (b).  {torch.cuda.get_device_name(0)}.", "",
             "| candidate | us / layer (median) | min | max | vs (a) |", "|---|---|---|---|---|"]
    base = statistics.median(times[graphs[0][0]])
    for name, _ in graphs:
        t = times[name]
        m = statistics.median(t)
        lines.append(f"| {name} | {m:.2f} | {min(t):.2f} | {max(t):.2f} | {m / base:.2f}x |")
    lines += ["", f"max |q_out of (b) - q_out of (c)| on the first layer: {agree:.4g} (the torch form rounds the normalised row to bf16 before the rotation, (b) rounds once: a bf16 ulp apart at the largest values)."]
    text = "\n".join(lines) + "\n"
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
