#!/usr/bin/env python3
"""Suffix pass on head dims 80 / 96 / 112 / 192 (GPU box): narrow unique caches against the two ways to run them zero-padded.

One process, the legs alternating inside every repeat, three repeats (their spread is printed next to every figure):

    narrow   k / v rows of the true width d, read as they are (hyd_suffix_params.kv_dim)     -- not on trees without it
    copy     pad_head_dim on q, k and v, the D-wide call under the true dim's scale, the slice: what the operators did
             for these head dims before narrow caches existed (and still do for shapes without a narrow kernel)
    padded   D-wide caches kept zero-padded by the caller, D-wide q: no copy, D / d times the bytes

C2 heads (B = 1024 sequences, 32 / 32 heads; 16 / 16 at d = 192), 128-row caches in the model's arena layout, S keys per
sequence.  TB/s counts the algorithmic bytes of the pass, 2 tensors x 2 bytes x Hkv x d x B x S, whatever a leg really moves.
`copy` and `padded` use nothing new: the tool runs unchanged on an older tree, which gives the same legs' figures there.

    python tools/head_dim_bench.py [--out FILE] [--quick] [--shapes 96:32,192:16] [--suffix 16,64,128]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from hydragen_amd import flash as F, placement  # noqa: E402

DEV, DT = "cuda:0", torch.bfloat16
HAS_NARROW = hasattr(F, "narrow_kv_native")


def timed_us(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    evs[0].record()
    for i in range(iters):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="few iterations (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="80:32,96:32,112:32,192:16", help="d:heads,...")
    ap.add_argument("--suffix", default="16,64,128")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("head_dim_bench needs the GPU: there is nothing to time without one")
    iters = 5 if a.quick else 40
    B, cap = a.batch, 128
    lines = [f"narrow kernel in this tree: {HAS_NARROW}; B = {B}, {cap}-row caches, bf16, median of {iters} launches per repeat, "
             f"{a.repeats} repeats, legs alternating",
             "", "| d | D | heads | S | leg | us (median of repeats) | repeats | spread | TB/s (algorithmic) |", "|---|---|---|---|---|---|---|---|---|"]
    records = []
    for spec in a.shapes.split(","):
        d, H = (int(x) for x in spec.split(":"))
        D = F.padded_head_dim(d)
        g = torch.Generator(device=DEV).manual_seed(d)
        qd = torch.randn(B, 1, H, d, device=DEV, dtype=DT, generator=g)
        qD = F.pad_head_dim(qd, D)
        narrow = placement.kv_arena((B, cap, H, d), DT, DEV, zero=False)
        narrow.normal_()
        wide = placement.kv_arena((B, cap, H, D), DT, DEV, zero=True)
        wide[..., :d] = narrow
        for S in (int(x) for x in a.suffix.split(",")):
            lens = torch.full((B,), S, dtype=torch.int32, device=DEV)

            def leg_copy():
                with F.true_head_dim_scale(d):
                    o, _ = F.flash_attention_seqlen(F.pad_head_dim(qd, D), F.pad_head_dim(narrow[0], D), F.pad_head_dim(narrow[1], D), lens)
                return o[..., :d].contiguous()

            def leg_padded():
                with F.true_head_dim_scale(d):
                    return F.flash_attention_seqlen(qD, wide[0], wide[1], lens)[0]

            legs = {"copy": leg_copy, "padded": leg_padded}
            if HAS_NARROW:
                assert F.narrow_kv_native(qd, narrow[0], narrow[1]), (d, H)
                legs = {"narrow": lambda: F.flash_attention_seqlen(qd, narrow[0], narrow[1], lens)[0], **legs}
            # same seeded inputs, same answers: the legs differ in bytes moved, not in what they compute
            outs = {n: f() for n, f in legs.items()}
            ref = outs["copy"]
            for n, o in outs.items():
                assert (o[..., :d].float() - ref.float()).abs().max() < 2e-2, (n, d, S)
            same = {n: bool(torch.equal(o[..., :d], ref)) for n, o in outs.items()}
            del outs
            times = {n: [] for n in legs}
            for _ in range(a.repeats):
                for n, f in legs.items():
                    times[n].append(timed_us(f, iters))
            algo = 2 * 2 * H * d * B * S
            for n in legs:
                med = statistics.median(times[n])
                spread = (max(times[n]) - min(times[n])) / med
                rec = dict(d=d, D=D, heads=H, S=S, leg=n, us=round(med, 1), repeats=[round(t, 1) for t in times[n]], spread=round(spread, 4),
                           tbps=round(algo / med / 1e6, 2), bit_equal_to_copy=same[n])
                records.append(rec)
                lines.append(f"| {d} | {D} | {H} / {H} | {S} | {n} | {med:.1f} | {' / '.join(f'{t:.1f}' for t in times[n])} | {100 * spread:.1f} % | {rec['tbps']:.2f} |")
                print(lines[-1], flush=True)
        del narrow, wide
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
