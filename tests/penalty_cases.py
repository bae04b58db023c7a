"""Inputs shared by tests/test_sampling_penalties.py (the CPU tie census) and tests/test_sampling_penalties_gpu.py: every case is
built on the CPU from its seed, so that the census runs the float64 definition on the very rows the kernel is given."""
import math

import torch

from hydragen_amd import sampling

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

# rows, n, dtype, context levels as (groups, tokens per group), gen stride and how it is filled, bias entries, the scalars.
# r is never a power of two: with 16-bit logits that manufactures exact ties between a penalised and an untouched token.
CASES = {
    "bf16_128k_1024": dict(rows=1024, n=128256, dtype="bf16", levels=[(1, 2048), (8, 300), (1024, 48)], stride=64, fill="ragged",
                           K=16, r=1.3, f=0.7, a=-0.4, seed=101),
    "bf16_32k_1024": dict(rows=1024, n=32000, dtype="bf16", levels=[(4, 500)], stride=64, fill="ragged", K=0, r=1.15, f=0.3, a=0.6,
                          seed=102),
    "f16_32k_7": dict(rows=7, n=32000, dtype="f16", levels=[(1, 700)], stride=8, fill="one", K=0, r=1.7, f=0.0, a=0.0, seed=103),
    "f32_odd_1": dict(rows=1, n=31997, dtype="f32", levels=[], stride=4, fill="none", K=5, r=1.0, f=0.0, a=0.0, seed=104),
    "f32_128k_7": dict(rows=7, n=128256, dtype="f32", levels=[(1, 4000), (7, 100), (7, 9)], stride=2048, fill="full", K=1024,
                       r=1.25, f=0.05, a=0.9, seed=105),
    "f16_odd_7": dict(rows=7, n=128253, dtype="f16", levels=[(1, 64), (7, 33)], stride=33, fill="ragged", K=3, r=0.8, f=-0.2, a=0.3,
                      seed=106),
    "f32_wide_2": dict(rows=2, n=300001, dtype="f32", levels=[(1, 3000), (2, 50)], stride=16, fill="ragged", K=7, r=1.4, f=0.5, a=0.1,
                       seed=107),  # wider than the bitmap the kernel keeps in LDS
    "bf16_small_1024": dict(rows=1024, n=1000, dtype="bf16", levels=[(2, 200)], stride=32, fill="ragged", K=20, r=1.9, f=1.1, a=0.7,
                            seed=108),
    "bf16_nogen_7": dict(rows=7, n=32000, dtype="bf16", levels=[(7, 600)], stride=0, fill="none", K=0, r=1.3, f=0.0, a=0.0, seed=109),
}


def build(name):
    """-> dict(logits [rows, n] (CPU, the case's dtype), r, f, a, bias (ids, values) or None, context [(bits, rows_per_group)],
    gen int32 [rows, stride] or None, gen_len int32 [rows] or None).  Half of the generated tokens and a quarter of the context
    and bias ids come from the row's 32 largest logits: penalties that never reach the top of a row test nothing at T = 0."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    rows, n = c["rows"], c["n"]
    logits = (torch.randn(rows, n, generator=g) * 3.0).to(DT[c["dtype"]])
    top = torch.topk(logits.float(), 32, dim=-1).indices  # [rows, 32]

    def mixed(owner_rows, count, share):
        """[len(owner_rows), count] ids: `share` of them from the owner row's top tokens, the rest uniform."""
        uni = torch.randint(0, n, (len(owner_rows), count), generator=g)
        pick = top[owner_rows].gather(1, torch.randint(0, 32, (len(owner_rows), count), generator=g))
        return torch.where(torch.rand(len(owner_rows), count, generator=g) < share, pick, uni)

    context = []
    for groups, L in c["levels"]:
        rpg = rows // groups
        ids = mixed(torch.arange(groups) * rpg, L, 0.25)
        lens = torch.randint(max(L // 2, 1), L + 1, (groups,), generator=g)
        context.append((sampling.token_bitmap_reference(ids, lens, n), rpg, ids, lens))
    gen = gen_len = None
    if c["stride"]:
        gen = mixed(torch.arange(rows), c["stride"], 0.5).to(torch.int32)
        gen_len = {"ragged": torch.randint(0, c["stride"] + 1, (rows,), generator=g), "one": torch.ones(rows, dtype=torch.int64),
                   "full": torch.full((rows,), c["stride"]), "none": torch.zeros(rows, dtype=torch.int64)}[c["fill"]].to(torch.int32)
        if c["fill"] == "ragged":
            gen_len[0], gen_len[-1] = 0, c["stride"]
            gen[rows // 2, 0] = -1  # an entry outside [0, n) is ignored
    bias = None
    if c["K"]:
        ids = torch.cat([top[0, : c["K"] // 4 + 1], torch.randperm(n, generator=g)[: c["K"]]]).unique()[: c["K"]]
        values = torch.randn(ids.numel(), generator=g) * 2.0
        values[0] = -math.inf
        bias = (ids.to(torch.int64), values.to(torch.float32))
    return dict(logits=logits, r=c["r"], f=c["f"], a=c["a"], bias=bias, context=[(b, k) for b, k, _, _ in context],
                context_ids=[(i, l, k) for _, k, i, l in context], gen=gen, gen_len=gen_len)


def penalised(case, rows=slice(None)):
    """The float64 definition on (a slice of) the case's rows, in chunks of rows that keep the [rows, n] tables small."""
    lg = case["logits"][rows]
    first = rows.start or 0
    out = []
    for s in range(0, lg.shape[0], 64):
        e = min(s + 64, lg.shape[0])
        ctx = []
        for bits, rpg in case["context"]:
            idx = (torch.arange(first + s, first + e) // rpg)
            ctx.append((bits[idx], 1))
        out.append(sampling.penalize_logits(
            lg[s:e], case["r"], case["a"], case["f"], case["bias"], ctx,
            None if case["gen"] is None else case["gen"][rows][s:e], None if case["gen"] is None else case["gen_len"][rows][s:e]))
    return torch.cat(out)


def margin_rows(x):
    """Rows a temperature-0 comparison may leave out: best and second-best x (float64) differ, by less than 4 fp32 ulps of the
    larger one.  (Equal x are no excuse: equal doubles round to equal floats and the lowest index wins on both sides.)"""
    v = torch.topk(torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x), 2, dim=-1).values
    ulp = torch.abs(torch.nextafter(v[:, 0].float(), torch.tensor(math.inf, device=x.device)) - v[:, 0].float()).double()
    gap = v[:, 0] - v[:, 1]
    return (gap > 0) & (gap < 4 * ulp)


def greedy(x):
    """Lowest-index maximum of every row of x (NaN never wins)."""
    xm = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    is_max = xm == xm.amax(-1, keepdim=True)
    n = x.shape[-1]
    return torch.where(is_max, torch.arange(n, device=x.device), torch.full((1,), n, device=x.device)).amin(-1)
