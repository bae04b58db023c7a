"""Per-row sampling launch next to the scalar one (profiles/per_row_sampling.md).

    python tools/sampling_rows_bench.py [--parent-lib PATH] [--rows 1024] [--iters 200] [--repeats 5] [--out FILE]

B = 1024 bf16 rows of randn * 3 at V = 32000 and V = 128256, top-p 0.95, temperature 0.8:
  scalar   hyd_sample_tokens_filtered, one set of values for all rows;
  per-row  hyd_sample_tokens_rows with 8 distinct (temperature, top_k, top_p, min_p) combinations spread over the rows and a seed
           per row -- reported against the scalar launch of the same build, no target of its own;
  parent   (--parent-lib: a libhydragen_hip.so built from the parent commit) the scalar launch of that build, alternated with this
           build's in one process, A B A B ..., so that both see the same clocks; the spread of the parent's own repeats is what a
           difference is read against.  The scalar kernels of this build are, instruction for instruction, the parent's (the per-row
           forms are instantiations of their own), so the table is a check, not a tuning aid.
Each figure: the median over `repeats` of (`iters` launches between two events) / iters, in microseconds, after a warm-up."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from hydragen_amd import _lib, layer_ops  # noqa: E402
from hydragen_amd.layer_ops import Penalties  # noqa: E402

COMBOS = [(0.0, 0, 1.0, 0.0), (0.7, 0, 0.95, 0.0), (1.3, 40, 1.0, 0.0), (0.8, 0, 0.9, 0.05), (1.0, 1, 1.0, 0.0), (0.7, 50, 0.5, 0.0),
          (1.3, 0, 1.0, 0.05), (0.8, 1000, 0.99, 0.0)]


def _time(fn, iters, repeats):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def _parent_scalar(path, x, out, lp, kept):
    """The parent build's hyd_sample_tokens_filtered on the same tensors (its own ctypes handle; the struct layout is unchanged)."""
    lib = C.CDLL(str(path))
    lib.hyd_sample_tokens_filtered.restype = C.c_int
    lib.hyd_sample_tokens_filtered.argtypes = [C.POINTER(_lib.SampleFilterParams), C.c_void_p]
    p = _lib.SampleFilterParams()
    layer_ops._fill_rows(p, x, (out, lp, kept), 0.8, (1, 4), None, 0.95, None)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        rc = lib.hyd_sample_tokens_filtered(C.byref(p), stream)
        assert rc == 0, rc
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    res = {}
    for V in (32000, 128256):
        x = (torch.randn(a.rows, V, device=dev, generator=torch.Generator(device=dev).manual_seed(V)) * 3.0).to(torch.bfloat16)
        cols = [torch.tensor([COMBOS[r % 8][i] for r in range(a.rows)], dtype=dt, device=dev)
                for i, dt in enumerate((torch.float32, torch.int32, torch.float32, torch.float32))]
        seeds = torch.arange(1, a.rows + 1, dtype=torch.int64, device=dev)
        pen = Penalties()
        scalar = lambda: layer_ops.sample_tokens_filtered(x, 0.8, (1, 4), top_p=0.95)  # noqa: E731
        rows = lambda: layer_ops.sample_tokens_penalized(x, cols[0], (1, 4), penalties=pen, top_k=cols[1], top_p=cols[2], min_p=cols[3],  # noqa: E731
                                                          seed=seeds)
        rec = {}
        if a.parent_lib:
            outs = layer_ops._draw_outputs(x, stats=True)
            parent = _parent_scalar(a.parent_lib, x, *outs)
            this, that = [], []
            for _ in range(a.repeats):  # A B A B: one repeat of each, alternated
                that += _time(parent, a.iters, 1)
                this += _time(scalar, a.iters, 1)
            rec["parent_scalar_us"], rec["scalar_us"] = that, this
        else:
            rec["scalar_us"] = _time(scalar, a.iters, a.repeats)
        rec["per_row_us"] = _time(rows, a.iters, a.repeats)
        res[V] = {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in rec.items()}
        print(json.dumps({"V": V, "rows": a.rows, **res[V]}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
