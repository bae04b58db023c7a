"""The cases of tests/test_moe_stress.py (their conditions, on the CPU) and tests/test_moe_stress_gpu.py (the four expert calls on the
device): deep products, route shapes, hard routing rows, and an fp32 emulation of a kernel for any shape.  Plain torch on the CPU."""
import math
from functools import lru_cache
from typing import NamedTuple

import torch

from hydragen_amd import moe
from tests.test_moe_gpu import crafted_logits

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
# k per unit of a wave's share of a product: kStepK of moe.hip / moe_w8.hip, kUnitK (a half step) of moe_w4.hip; None: moe_grouped.hip's waves
# split the tile, not K -- each runs all ceil(K / 64) steps into one accumulator
STEP = {"rows": 64, "grouped": None, "w8": 128, "w4": 128}
MAX_ROWS = {"rows": moe.MOE_MAX_ROWS, "grouped": moe.MOE_GROUPED_MAX_ROWS, "w8": moe.MOE_MAX_ROWS, "w4": moe.MOE_MAX_ROWS}
DEEP = {"rows": [(512, 288), (576, 544)], "grouped": [(576, 544)], "w8": [(704, 544)], "w4": [(1344, 1056)]}  # (H, I)
SHALLOW = [(64, 32), (192, 96)]
ROUTE_SHAPES = [(1, 1), (8, 1), (8, 8), (256, 1), (256, 8)]  # (E, k)
HARD_ROUTES = [(8, 2), (65, 8), (129, 8), (193, 8), (256, 8)]  # (E, k): one chunk of a lane, and a last chunk of one, one, one and 64 experts


def waves_steps(K, step):
    """The steps each of a workgroup's four waves takes of a K-deep product: the kernels' s0 = wave * steps / 4 with steps = ceil(K / step)."""
    steps = -(-K // step)
    return [(w + 1) * steps // 4 - w * steps // 4 for w in range(4)]


class Case(NamedTuple):
    call: str  # rows (moe_rows), grouped (moe_rows_grouped), w8, w4
    dtype: str
    T: int
    E: int
    k: int
    H: int
    I: int
    variant: object  # random, same, last, one_each, or the number of rows on expert 1
    renorm: bool = True

    @property
    def id(self):
        return f"{self.call}-{self.dtype}-T{self.T}-E{self.E}k{self.k}-{self.H}x{self.I}-{self.variant}-{'renorm' if self.renorm else 'plain'}"


def deep_cases(call, dtype, H, I):
    """Waves with several steps, combined with second passes over `red` and partly filled tiles (rows, w8, w4: 32 slots a pass; 33 = a pass
    and one row, 48 = a pass and a half-filled one, 49 = and a second tile of one row) and with full and one-row row tiles (grouped)."""
    E, k = (4, 2) if call == "w4" else (8, 2)  # (w4: its buffers test's E, and a quarter of a GB of float64 less)
    if call == "grouped":
        tv = [(130, 64, True), (130, 65, True), (130, "last", True), (130, "random", False)]
    elif call == "rows":
        tv = [(33, "random", True), (33, "random", False)] + [(128, v, True) for v in ("same", 32, 33, 48, 49)]
    else:
        tv = [(128, "same", True), (128, 33, True), (128, 33, False)]
    return [Case(call, dtype, T, E, k, H, I, v, r) for T, v, r in tv]


def route_cases(call, dtype, E, k):
    """k = 1, k = E, E = 1 and E = 256 under scattered slots, every slot on the highest experts, and one slot on every expert (for rows, on
    the first 128 / k)."""
    T = 130 if call == "grouped" else 33
    return [Case(call, dtype, min(E // k, MAX_ROWS[call]) if v == "one_each" else T, E, k, H, I, v) for H, I in SHALLOW for v in ("random", "last", "one_each")]


def boundary_cases(dtype):
    """moe_rows' choice of MT: T k <= 16 is one tile a pass.  16 slots on one expert where k = 1, else T on each of k: MT = 1; 17 / 24: MT = 2."""
    return [Case("rows", dtype, T, 8, k, 192, 96, "same") for T, k in ((16, 1), (8, 2), (2, 8), (17, 1), (3, 8))]


def quantized_route_cases(call, dtype):
    return [Case(call, dtype, 33, 8, 2, 192, 96, "last"), Case(call, dtype, 33, 8, 1, 192, 96, "random")]


def all_mlp_cases():
    out = []
    for dtype in DTYPES:
        for call, shapes in DEEP.items():
            for H, I in shapes:
                out += deep_cases(call, dtype, H, I)
        for call in ("rows", "grouped"):
            for E, k in ROUTE_SHAPES:
                out += route_cases(call, dtype, E, k)
        out += boundary_cases(dtype)
        for call in ("w8", "w4"):
            out += quantized_route_cases(call, dtype)
    return out


def route_logits(logits, variant, k):
    """`random`: as they are; `same`: crafted_logits'; a number n: exactly the first n rows choose expert 1 (crafted_logits' 16 / 17 for any
    n); `last`: every row chooses experts E - k .. E - 1; `one_each`: row t chooses experts k t .. k t + k - 1 (T k <= E)."""
    T, E = logits.shape
    if variant == "same":
        return crafted_logits(logits, variant, k)
    logits = logits.clone()
    if isinstance(variant, int):
        logits[:, 1] = -50
        logits[:variant, 1] = 50
    elif variant == "last":
        for j in range(k):
            logits[:, E - k + j] = 50 - j
    elif variant == "one_each":
        assert T * k <= E
        for j in range(k):
            logits[torch.arange(T), k * torch.arange(T) + j] = 50 - j
    else:
        assert variant == "random", variant
    return logits


@lru_cache(maxsize=4)
def _weights(E, H, I, dtype):
    """router, gate_up, down of tests.test_moe_gpu.inputs' distributions; past H = 192 the router's and the gate / up rows' standard
    deviations are scaled by sqrt(64 / H): pre-activations stay of order 2 (inputs' docstring has the reason) and logits of std 4, below
    the 50 of the crafted routes; everything stays far inside float16.
    Every eighth output channel (h % 8 == 5) is a PROBE: its down row holds one weight, +-0.25 at column 7 h % I, in every expert.  A dense
    row's output adds I products, and the bound adds their ABSOLUTE values: it grows like I where the output, and what a wrong act does to
    it, grow like sqrt(I), so on dense rows alone a gate/up swap that is 1000 bounds away at I = 32 is a few tens away at I = 1056.  A
    probe channel is one act element times a constant: its bound is that element's own, at any depth."""
    g, sc = torch.Generator().manual_seed(1000 + E + H + I), math.sqrt(64 / H) if H > 192 else 1.0
    router, gate_up, down = ((torch.randn(s, generator=g) * sd).to(DTYPES[dtype]) for s, sd in (((E, H), 0.5 * sc), ((E, 2 * I, H), 0.3 * sc), ((E, H, I), 0.1)))
    probe = torch.arange(5, H, 8)
    col = (7 * probe) % I
    val = torch.where(down[:, probe, col] < 0, -0.25, 0.25).to(down.dtype)
    down[:, probe] = 0
    down[:, probe, col] = val
    return router, gate_up, down


@lru_cache(maxsize=2)
def _quantized(call, E, H, I, dtype):
    """(the call's weight tensors, their dequantized float64 values: the weights of the definition)"""
    _, gate_up, down = _weights(E, H, I, dtype)
    if call == "w8":
        q = moe.quantize_experts(gate_up, down)
        return q, moe.dequantize_experts(*q)
    q = moe.quantize_experts_fp4(gate_up, down)
    return q, moe.dequantize_experts_fp4(*q)


class Built(NamedTuple):
    x: torch.Tensor
    router: torch.Tensor
    logits: torch.Tensor
    weights: tuple  # what the call takes after x and logits
    gate_up: torch.Tensor  # the definition's weights
    down: torch.Tensor


def build(c):
    router, gate_up, down = _weights(c.E, c.H, c.I, c.dtype)
    x = torch.randn((c.T, c.H), generator=torch.Generator().manual_seed(7 * c.T + c.E)).to(DTYPES[c.dtype])
    logits = route_logits(torch.nn.functional.linear(x, router), c.variant, c.k)
    if c.call in ("rows", "grouped"):
        return Built(x, router, logits, (gate_up, down), gate_up, down)
    q, (gu, dn) = _quantized(c.call, c.E, c.H, c.I, c.dtype)
    return Built(x, router, logits, q, gu, dn)


@lru_cache(maxsize=2)
def _definition_weights(call, E, H, I, dtype):
    """(gate_up, |gate_up|, down, |down|, sum_i |down|) of the definition in float64, converted once for all the cases that share them"""
    _, gate_up, down = _weights(E, H, I, dtype) if call in ("rows", "grouped") else (None, *_quantized(call, E, H, I, dtype)[1])
    gate_up, down = gate_up.double(), down.double()
    return gate_up, gate_up.abs(), down, down.abs(), down.abs().sum(2)


def reference_and_bound(c, b, swapped=False):
    """(moe.moe_reference, moe.moe_error_bound) routed by b.logits: the terms of moe._slot_terms and the sums of moe_error_bound, formula for
    formula, but walked once for both, per EXPERT over all its slots (not per route position and expert), on weights converted to float64
    once per weight set.  At E = 256, k = 8 that is a fifth of the time of the two calls.  Only the grouping of rows into matrix products
    differs, so the results agree to float64 rounding: tests/test_moe_stress.py holds them to the two functions within 1e-12 relative.
    `swapped`: with every expert's up rows in front of its gate rows."""
    ids, w = moe.route_reference(b.logits, c.k, c.renorm)
    gu, agu, dn, adn, swd = _definition_weights(c.call, c.E, c.H, c.I, c.dtype)
    (T, H), I, k = b.x.shape, c.I, c.k
    u16, tiny = (2.0 ** -8, 0.0) if b.x.dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    xd, flat = b.x.double(), ids.flatten()  # slot t k + j
    xa = xd.abs()
    y, s_act, s_gu, s_wd = (xd.new_zeros((T * k, H)) for _ in range(4))
    for e in flat.unique().tolist():
        slots = (flat == e).nonzero()[:, 0]
        rows = slots // k
        wgu, awgu = (gu[e].roll(I, 0), agu[e].roll(I, 0)) if swapped else (gu[e], agu[e])
        g, u = (xd[rows] @ wgu.T).split(I, dim=1)
        ag, au = (xa[rows] @ awgu.T).split(I, dim=1)
        silu = torch.nn.functional.silu(g)
        act = (silu * u).to(b.x.dtype).double()
        y[slots] = act @ dn[e].T
        s_act[slots] = act.abs() @ adn[e].T
        s_gu[slots] = (ag * u.abs() * 1.1 + au * silu.abs()) @ adn[e].T
        s_wd[slots] = swd[e]
    out, bound = (xd.new_zeros((T, H)) for _ in range(2))
    for j in range(k):
        wj, yj = w[:, j, None], y[j::k]
        out += wj * yj
        bound += wj * ((I * 2.0 ** -23 + u16) * s_act[j::k] + H * 2.0 ** -23 * s_gu[j::k] + (k + 5) * 2.0 ** -23 * yj.abs() + tiny * s_wd[j::k])
    return out, bound + u16 * out.abs() + tiny


def swapped_reference(c, b):
    """The canary: the definition with up rows in front of gate rows."""
    return reference_and_bound(c, b, swapped=True)[0]


def emulate_fp32(x, logits, gate_up, down, k, renorm, step=64):
    """tests/test_moe.py's _emulate_fp32 for any shape and given logits: what a kernel computes, in its order and precisions -- the route
    of the 16-bit logits, fp32 softmax weights, both products in fp32 as four partial sums over the waves' K ranges (waves_steps) added in
    wave order (`step` None, the grouped call: one sum over K), act rounded once to x's dtype, the weighted rows added in j order, one rounding.  gate_up / down: 16-bit, or the float64
    dequantized weights (exact in fp32)."""
    ids = moe.route_reference(logits, k, renorm)[0]
    w = torch.softmax(logits.float(), dim=1).gather(1, ids)
    w = w / w.sum(1, keepdim=True) if renorm else w
    I = down.shape[2]

    def product(a, wt):
        if step is None:
            return a @ wt.T
        K, first, acc = a.shape[1], 0, torch.zeros((a.shape[0], wt.shape[0]))
        for n in waves_steps(K, step):
            k0, k1 = min(K, first * step), min(K, (first + n) * step)
            acc = acc + a[:, k0:k1] @ wt[:, k0:k1].T
            first += n
        return acc

    out = torch.zeros(x.shape)
    for j in range(k):
        yj = torch.zeros(x.shape)
        for e in ids[:, j].unique().tolist():
            rows = (ids[:, j] == e).nonzero()[:, 0]
            gu = product(x[rows].float(), gate_up[e].float())
            act = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]).to(x.dtype).float()
            yj[rows] = product(act, down[e].float())
        out = yj * w[:, j, None] if j == 0 else out + yj * w[:, j, None]
    return out.to(x.dtype).double()


def _bits(patterns, dtype):
    return torch.tensor(patterns, dtype=torch.int32).to(torch.int16).view(dtype)


def hard_rows(E, k, dtype):
    """(names, logits [rows, E]) of one 16-bit dtype: rows the route kernel's keys, its `v - top` and its exponentials can get wrong.
    masked             -inf on E - k - 1 experts (k + 1 stay finite, so no chosen logit is -inf)
    max_finite         the largest finite value on k - 1 experts, zeros on two, its negative elsewhere: `v - top` overflows fp32 to -inf (bfloat16; -2^17 in float16); the last
                       chosen logit is a zero, whose weight is exactly 0
    masked_max_finite  the same with -inf in place of the negative
    denormal_gap       the winner (expert E - 1) at 0, the others chosen 88 to 104 below it, the rest 120 below: exponentials in and below fp32's
                       denormal range; in plain mode their weights are below 2^-126
    subnormal          signed multiples 0 .. 5 of the dtype's smallest subnormal: ties between +0 and -0 and between equal subnormals
    ties_one_lane      (E > 64) the maxima tied on experts l, l + 64, ..., all of lane l = (E - 1) % 64, a second tie 64 apart from expert l + 1 on
    last_chunk_winner  random, with expert E - 1 above all
    A row without a finite maximum (all -inf) is left out: the header says nothing about it, and the definition gives NaN."""
    dt = DTYPES[dtype]
    top = float(torch.finfo(dt).max)
    g = torch.Generator().manual_seed(E)
    rnd = lambda: (torch.randn(E, generator=g) * 2).to(dt)  # noqa: E731
    perm = torch.randperm(E, generator=g)
    rows = {}
    r = rnd()
    r[perm[: E - k - 1]] = float("-inf")
    rows["masked"] = r
    for name, low in (("max_finite", -top), ("masked_max_finite", float("-inf"))):
        r = torch.full((E,), low, dtype=dt)
        r[perm[: k - 1]] = top
        r[perm[k - 1: k + 1]] = 0.0
        rows[name] = r
    r = torch.full((E,), -120.0, dtype=dt)
    r[E - 1] = 0.0
    gaps = [88, 90, 92, 96, 100, 102, 104][: k - 1]  # (exact in both dtypes)
    r[perm[perm != E - 1][: len(gaps)]] = -torch.tensor(gaps, dtype=dt)
    rows["denormal_gap"] = r
    e = torch.arange(E)
    rows["subnormal"] = _bits((e % 6 + 0x8000 * ((e // 6) % 2)).tolist(), dt)
    if E > 64:
        r = (torch.randn(E, generator=g) * 0.5).clamp(max=1.5).to(dt)
        r[(E - 1) % 64:: 64] = 3.0
        r[(E - 1) % 64 + 1:: 64] = 2.0
        rows["ties_one_lane"] = r
    r = rnd()
    r[E - 1] = float(r.float().max()) + 1
    rows["last_chunk_winner"] = r
    return list(rows), torch.stack(list(rows.values()))
