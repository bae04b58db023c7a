"""The RoPE + append preamble, one candidate per kernel family, measured for a comparison of two builds of the library.  Writes the
table of profiles/rope_append_body.md -- nothing here is promised in advance.

    python tools/rope_append_bench.py --json RUN.json [--batch 1024] [--rounds 15] [--layers 32]     one run, one library
    python tools/rope_append_bench.py --ab PARENT_LIB NEW_LIB [--out TABLE.md] [--keep DIR]            six runs and the table

Shape: B = 1024 sequences, 32 query / 8 kv heads, D = 128, bf16; q / k / v are views into one fused q|k|v projection buffer, as in
the model.  Seven candidates -- plain, fp8 caches, narrow rows (d = 96), T = 4 tokens, q/k norm, q/k norm + fp8 caches, q/k norm +
T = 4 tokens --, each one decode step's preambles of `--layers` layers (distinct projection buffers and caches per layer) captured
in a HIP graph (device time, no launch gaps); the graphs' replays alternate in one process, round after round.  The figure of a
run is microseconds per layer: the median over the rounds.

--ab starts six such runs one after another as fresh processes, in the order parent, new, parent, new, parent, new, each with its
library in HYDRAGEN_HIP_LIB (two different directories), and nothing else on the card.  Per family: the middle one of the three
run medians on each side; the new side's minus the parent's must not exceed the parent's own spread, the largest minus the
smallest of its three run medians.  --ab ends with status 2 when a family misses that."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

DEV = "cuda:0"
FAMILIES = ("plain", "fp8", "narrow d=96", "multi T=4", "norm", "norm + fp8", "norm + multi T=4")


def graph_of(torch, fn):
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


def replay_us(torch, g, calls, reps=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * calls)


def one_run(a) -> dict:
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rope_append_bench.py measures on the GPU; none is visible")
    from hydragen_amd import _lib
    from hydragen_amd.fused_decode import rope_append_decode, rope_append_multi
    from hydragen_amd.llama import RotaryTable

    B, Hq, Hkv, D, S, dtype, eps = a.batch, 32, 8, 128, 8, torch.bfloat16, 1e-6
    g = torch.Generator(device=DEV).manual_seed(0)
    shared = torch.full((B,), 2048, dtype=torch.int64, device=DEV)
    pos = (shared + torch.randint(0, S - 3, (B,), device=DEV, generator=g))[:, None].contiguous()  # (T = 4 tokens fit the cache)
    ks, vs = (0.5 + torch.rand(Hkv, device=DEV, generator=g) for _ in range(2))

    def family(name):
        d = 96 if "narrow" in name else D
        T = 4 if "multi" in name else 1
        rot = RotaryTable(d, 4096, 10000.0, device=DEV)
        cos, sin = rot.cos_cached, rot.sin_cached
        cdtype = torch.float8_e4m3fn if "fp8" in name else dtype
        kw = dict(k_scale=ks, v_scale=vs) if "fp8" in name else {}
        if "norm" in name:
            kw.update(q_norm=(1 + 0.3 * torch.randn(d, device=DEV, generator=g)).to(dtype),
                      k_norm=(1 + 0.3 * torch.randn(d, device=DEV, generator=g)).to(dtype), norm_eps=eps)
        layers = []
        for _ in range(a.layers):
            qkv = torch.randn(B, T, (Hq + 2 * Hkv) * d, device=DEV, dtype=dtype, generator=g)
            layers.append((qkv[..., : Hq * d].view(B, T, Hq, d), qkv[..., Hq * d: (Hq + Hkv) * d].view(B, T, Hkv, d),
                           qkv[..., (Hq + Hkv) * d:].view(B, T, Hkv, d), torch.zeros(B, S, Hkv, d, device=DEV, dtype=dtype).to(cdtype),
                           torch.zeros(B, S, Hkv, d, device=DEV, dtype=dtype).to(cdtype)))
        op = rope_append_multi if T > 1 else rope_append_decode

        def step():
            for q, k, v, kc, vc in layers:
                op(q, k, v, cos, sin, pos, shared, kc, vc, **kw)

        # the graph holds addresses, not tensors: capturing the next family empties the allocator's cache (torch.cuda.graph does on
        # entry), so a family whose tensors had been dropped would replay on memory that is no longer mapped
        return graph_of(torch, step), (layers, cos, sin, kw)

    kept = {name: family(name) for name in FAMILIES}
    graphs = [(name, kept[name][0]) for name in FAMILIES]
    for _, gr in graphs:  # warm
        replay_us(torch, gr, a.layers, reps=3)
    times = {name: [] for name in FAMILIES}
    for _ in range(a.rounds):
        for name, gr in graphs:
            times[name].append(replay_us(torch, gr, a.layers))
    return dict(library=str(_lib.lib_path()), device=torch.cuda.get_device_name(0), batch=B, layers=a.layers, rounds=a.rounds,
                median_us={name: statistics.median(t) for name, t in times.items()},
                min_us={name: min(t) for name, t in times.items()}, max_us={name: max(t) for name, t in times.items()})


def table(parent: list, new: list) -> tuple:
    """-> (markdown, the families whose new side is slower than the parent's by more than the parent's own spread)"""
    r0 = parent[0]
    lines = [f"Shape: B = {r0['batch']}, 32 / 8 heads, D = 128, bf16, {r0['layers']} layers per graph replay, {r0['rounds']} alternating rounds of 5 "
             f"replays per run; microseconds per layer, the median of each run.  {r0['device']}.", "",
             "| family | parent 1 | parent 2 | parent 3 | new 1 | new 2 | new 3 | parent spread | new median - parent median | within the spread |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    missed = []
    for name in FAMILIES:
        p, n = [r["median_us"][name] for r in parent], [r["median_us"][name] for r in new]
        spread, diff = max(p) - min(p), statistics.median(n) - statistics.median(p)
        if diff > spread:
            missed.append(name)
        lines.append(f"| {name} | " + " | ".join(f"{x:.3f}" for x in p + n) + f" | {spread:.3f} | {diff:+.3f} | {'NO' if diff > spread else 'yes'} |")
    lines += ["", f"families: {len(FAMILIES)}; new slower than the parent by more than the parent's own spread: {len(missed)}"]
    return "\n".join(lines) + "\n", missed


def ab(a) -> int:
    libs = [Path(p).resolve() for p in a.ab]
    if libs[0].parent == libs[1].parent or not all(p.exists() for p in libs):
        raise SystemExit("--ab takes two existing libraries in two different directories")
    keep = Path(a.keep) if a.keep else Path(tempfile.mkdtemp(prefix="rope_append_bench_"))
    keep.mkdir(parents=True, exist_ok=True)
    runs = ([], [])
    for i in range(6):  # parent, new, parent, new, parent, new: one process at a time, each a fresh one
        out = keep / f"{'parent' if i % 2 == 0 else 'new'}{i // 2 + 1}.json"
        cmd = [sys.executable, str(Path(__file__).resolve()), "--json", str(out), "--batch", str(a.batch), "--rounds", str(a.rounds), "--layers", str(a.layers)]
        rc = subprocess.run(cmd, env=dict(os.environ, HYDRAGEN_HIP_LIB=str(libs[i % 2])), timeout=300).returncode
        if rc != 0:  # nothing more is started on the card after a run that failed
            print(f"run {i + 1} ({out.stem}) ended with status {rc}: stopping", file=sys.stderr)
            return rc or 1
        run = json.loads(out.read_text())
        assert run["library"] == str(libs[i % 2]), run["library"]
        runs[i % 2].append(run)
    text, missed = table(*runs)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    print(text)
    if missed:
        print("SLOWER THAN THE PARENT BY MORE THAN ITS OWN SPREAD: " + ", ".join(missed), file=sys.stderr)
    return 2 if missed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="one run: write its medians here")
    ap.add_argument("--ab", nargs=2, metavar=("PARENT_LIB", "NEW_LIB"), help="six runs, parent and new alternating, and the table")
    ap.add_argument("--out", help="--ab: write the table here as well")
    ap.add_argument("--keep", help="--ab: keep the six runs' JSON files in this directory")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    if a.ab:
        raise SystemExit(ab(a))
    run = one_run(a)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(run, indent=1) + "\n")
    print(json.dumps(run))


if __name__ == "__main__":
    main()
