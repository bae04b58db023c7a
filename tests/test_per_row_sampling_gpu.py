"""-m gpu: hyd_sample_tokens_rows (csrc/sample_rows.hip) and hyd_stop_update_rows against the scalar entry points, bit for bit.
A row of a per-row launch IS that row of a scalar launch with the row's values: nothing here has a tolerance.  The one
exception is the host noise mirror of the seeded draw (tests/sampler_mirror.py), which leaves out the rows whose winning margin
is inside the mirror's own error bound, as the existing stress tests do."""
import math

import numpy as np
import pytest
import torch

from hydragen_amd import _lib, layer_ops, sampling, stopping
from hydragen_amd.constraint import TokenDFA
from hydragen_amd.layer_ops import Penalties
from tests import sampler_mirror as M
from tests.per_row_cases import F32, NAMES, TABLE, mirror_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ROWS = 24
KEY = (11, 6)
S = 4  # automaton states


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _logits(n, dtype, pad=0):
    g = torch.Generator(device=DEV).manual_seed(n)
    x = (torch.randn(ROWS, n + pad, device=DEV, generator=g) * 3.0).to(dtype)[:, :n]
    x[5] = -math.inf              # no valid logit
    x[6] = 1.25                   # an all-equal plateau
    x[7, ::2] = -math.inf         # -inf and NaN entries
    x[7, 1::3] = math.nan
    x[19] = x[7]                  # (the same row under another combination)
    return x


def _columns(rows=ROWS):
    """The table dealt over the rows: {name: list of `rows` values}"""
    return {name: [TABLE[r % len(TABLE)][i] for r in range(rows)] for i, name in enumerate(NAMES)}


def _penalties(n, combo=None, cols=None):
    """Fresh Penalties over 6 context groups of 4 rows and a list of generated tokens per row (the sampler appends its draw)."""
    g = torch.Generator().manual_seed(n + 1)
    ctx = layer_ops.token_bitmap(torch.randint(0, n, (ROWS // 4, 12), generator=g).to(DEV), None, n)
    gen = torch.randint(0, min(n, 64), (ROWS, 16), generator=g).to(torch.int32).to(DEV)
    gen_len = (torch.arange(ROWS) % 9).to(torch.int32).to(DEV)
    src = cols if combo is None else dict(zip(NAMES, combo))
    return Penalties(src["repetition_penalty"], src["presence_penalty"], src["frequency_penalty"], None, [(ctx, 4)], gen, gen_len, append=True)


def _automaton(n):
    g = torch.Generator().manual_seed(n + 2)
    nxt = torch.randint(0, S, (S, n), generator=g)
    nxt = torch.where(torch.rand(S, n, generator=g) < 0.4, torch.full_like(nxt, sampling.DFA_REJECT), nxt)
    nxt[0, 0] = 1  # (state 0 allows something)
    return TokenDFA(nxt.to(torch.int32)).to(DEV)


def _launch(family, x, dfa, values, **kw):
    """One launch of `family` with `values` = {name: scalar or per-row list} -> every output, as a tuple of tensors."""
    n = x.shape[1]
    cuts = dict(top_k=values["top_k"], top_p=values["top_p"], min_p=values["min_p"])
    state = ((torch.arange(ROWS, device=DEV) % (S + 2)) - 1).to(torch.int32)  # -1 and S: unconstrained rows
    con = (dfa, state, True)
    if family == "filtered":
        if any(sampling.is_per_row(v) for v in values.values()) or "seed" in kw:
            return layer_ops.sample_tokens_penalized(x, values["temperature"], KEY, penalties=Penalties(), **cuts, **kw)
        return layer_ops.sample_tokens_filtered(x, values["temperature"], KEY, **cuts)
    pen = Penalties() if family == "constrained" else _penalties(n, cols=values)
    if family == "penalized":
        out = layer_ops.sample_tokens_penalized(x, values["temperature"], KEY, penalties=pen, **cuts, **kw)
        return out + (pen.gen, pen.gen_len)
    out = layer_ops.sample_tokens_constrained(x, values["temperature"], KEY, constraint=con, penalties=pen, **cuts, **kw)
    return out + (state,) + (() if pen.gen is None else (pen.gen, pen.gen_len))


@pytest.mark.parametrize("n, pad", [(5, 0), (1000, 0), (8200, 8), (32003, 0)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["filtered", "penalized", "constrained", "constrained_penalized"])
def test_a_row_of_a_per_row_launch_is_that_row_of_a_scalar_launch(family, dtype, n, pad):
    x = _logits(n, dtype, pad)
    assert x.stride(0) == n + pad
    dfa = _automaton(n)
    cols = _columns()
    if family in ("filtered", "constrained"):  # no penalty anywhere in the call: the kernels with the row's own key width
        for name in NAMES[4:]:
            cols[name] = [None] * ROWS
    got = _launch(family, x, dfa, cols)
    for j, combo in enumerate(TABLE):
        values = dict(zip(NAMES, combo))
        if family in ("filtered", "constrained"):
            values.update(repetition_penalty=None, frequency_penalty=None, presence_penalty=None)
        want = _launch(family, x, dfa, values)
        rows = torch.arange(j, ROWS, len(TABLE), device=DEV)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(_bits(a)[rows], _bits(b)[rows]), (family, j, combo, k)


def test_values_outside_their_range_are_replaced_as_the_header_says():
    """Plain floats read by value; the launch with the documented replacement gives the same bits."""
    n = 1000
    x = _logits(n, torch.bfloat16)
    dfa = _automaton(n)
    nan, inf = math.nan, math.inf
    bad = dict(temperature=[nan, -1.0, 0.7], top_k=[-5, -(2 ** 31), 40], top_p=[0.0, 1.5, nan, -0.1, 0.9], min_p=[-0.1, 1.5, nan, 0.05],
               repetition_penalty=[0.0, -1.0, inf, nan, F32(1.3)], frequency_penalty=[inf, nan, -inf, 0.5], presence_penalty=[-inf, nan, 0.25])
    good = dict(temperature=[0.0, 0.0, 0.7], top_k=[0, 0, 40], top_p=[1.0, 1.0, 1.0, 1.0, 0.9], min_p=[0.0, 0.0, 0.0, 0.05],
                repetition_penalty=[1.0, 1.0, 1.0, 1.0, F32(1.3)], frequency_penalty=[0.0, 0.0, 0.0, 0.5], presence_penalty=[0.0, 0.0, 0.25])
    dt = {name: dtype for name, dtype, _ in layer_ops.ROW_FIELDS}

    def spread(table):  # tensors: the host checks nothing of them
        return {k: torch.tensor([v[r % len(v)] for r in range(ROWS)], dtype=dt[k], device=DEV) for k, v in table.items()}

    for family in ("penalized", "constrained_penalized"):
        got, want = _launch(family, x, dfa, spread(bad)), _launch(family, x, dfa, spread(good))
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(_bits(a), _bits(b)), (family, k)


@pytest.mark.parametrize("family", ["filtered", "penalized"])
def test_a_seeded_row_draws_as_row_zero_of_a_launch_with_its_seed(family):
    n = 8200
    x = _logits(n, torch.float16)
    cols = _columns()
    seeds = [(0x9E3779B97F4A7C15 * (r + 1)) & 0xFFFFFFFFFFFFFFFF for r in range(ROWS)]  # both halves of the key in use
    got = _launch(family, x, None, cols, seed=seeds)
    if family == "filtered":
        for r in range(ROWS):
            v = dict(zip(NAMES, TABLE[r % len(TABLE)]))
            tok, lp, kept = layer_ops.sample_tokens_filtered(x[r : r + 1], v["temperature"], (seeds[r], KEY[1]), top_k=v["top_k"],
                                                             top_p=v["top_p"], min_p=v["min_p"])
            assert torch.equal(got[0][r : r + 1], tok) and torch.equal(_bits(got[1][r : r + 1]), _bits(lp)) and torch.equal(got[2][r : r + 1], kept), r
    # over permuted rows: the permuted outputs (a row's draw does not know its place in the batch)
    perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(3))
    xp = x[perm.to(DEV)]
    colp = {k: [v[int(i)] for i in perm] for k, v in cols.items()}
    if family == "filtered":
        gotp = layer_ops.sample_tokens_penalized(xp, colp["temperature"], KEY, penalties=Penalties(), top_k=colp["top_k"], top_p=colp["top_p"],
                                                 min_p=colp["min_p"], seed=[seeds[int(i)] for i in perm])
    else:  # the rows' contexts and generated tokens travel with them
        pen = _penalties(n, cols=cols)
        ctx_rows = sampling.context_mask(pen.context, ROWS, n)[perm.to(DEV)]
        bits = layer_ops.token_bitmap(torch.where(ctx_rows, torch.arange(n, device=DEV)[None, :], torch.full((1, 1), -1, device=DEV)), None, n)
        penp = Penalties(colp["repetition_penalty"], colp["presence_penalty"], colp["frequency_penalty"], None, [(bits, 1)],
                         pen.gen[perm.to(DEV)].contiguous(), pen.gen_len[perm.to(DEV)].contiguous(), append=True)
        gotp = layer_ops.sample_tokens_penalized(xp, colp["temperature"], KEY, penalties=penp, top_k=colp["top_k"], top_p=colp["top_p"],
                                                 min_p=colp["min_p"], seed=[seeds[int(i)] for i in perm])
    for k in range(3):
        assert torch.equal(_bits(gotp[k]), _bits(got[k])[perm.to(DEV)]), (family, k)
    # and the seeds reach the noise: another seed, other tokens on the sampled rows
    other = _launch(family, x, None, cols, seed=[s ^ 1 for s in seeds])
    assert (other[0] != got[0]).float().mean() > 0.2


def test_seeded_rows_draw_the_host_mirrors_token():
    """256 bf16 rows of randn * 3 at n = 32003, each at its own T and seed, against tests/sampler_mirror.mirror_draw called per row
    as ROW 0 of a launch with the row's seed.  The case's generator seed (tests/per_row_cases.MIRROR_SEED) was chosen with the
    mirror alone, on the CPU: it leaves 0 of the 256 rows uncompared (0 < margin <= EPS); the cap is the stress tests' 1 %."""
    xc, temps, seeds, offset = mirror_case()
    x = xc.to(DEV)
    x64 = xc.double().numpy()
    tok = layer_ops.sample_tokens_penalized(x, temps, (0, offset), penalties=Penalties(), seed=seeds)[0][:, 0].cpu().numpy()
    skipped = 0
    for r in range(x.shape[0]):
        _, margin, lowest = M.mirror_draw(x64[r : r + 1], temps[r], seeds[r], offset, rows=[0])
        if margin[0] > M.eps(M.max_abs(x64[r : r + 1]), temps[r]):
            assert tok[r] == lowest[0], (r, tok[r], lowest[0], margin[0])
        else:
            skipped += 1
    print(f"rows not compared (0 < margin <= EPS) of {x.shape[0]}: {skipped}")
    assert skipped <= 0.01 * x.shape[0]


# ---- the stop kernel with a limit per row ----------------------------------------------------------------------------------------
def _stop_case():
    g = torch.Generator().manual_seed(5)
    rows, steps = 64, 12
    toks = torch.randint(0, 10, (rows, steps), generator=g)
    spec = stopping.check_stop([7, 3], [[5], [1, 2, 4]], pad_token_id=11, include_stop=False, vocab_size=12)
    toks[3, 2:5] = torch.tensor([1, 2, 4])
    toks[4, 9:12] = torch.tensor([1, 2, 4])
    max_len = (torch.arange(rows) % steps + 1).to(torch.int32)
    start = torch.randint(5, 40, (rows,), generator=g)
    shared = torch.randint(1, 5, (rows,), generator=g)
    return toks, spec, max_len, start, shared


@pytest.mark.parametrize("limited", [True, False])
def test_stop_update_rows_is_the_reference_step_by_step(limited, monkeypatch):
    toks, spec, max_len, start, shared = _stop_case()
    if not limited:  # a NULL max_len must be hyd_stop_update: route the plain call through the new export
        lib = _lib.load()
        monkeypatch.setattr(lib, "hyd_stop_update", lambda p, s: lib.hyd_stop_update_rows(p, None, s), raising=False)
    rows, steps = toks.shape
    ref = stopping.new_state(rows, steps, spec)
    dev = stopping.new_state(rows, steps, spec, DEV)
    ml = max_len if limited else None
    for t in range(steps):
        fr, pr = stopping.stop_update_reference(toks[:, t], t, spec, *ref, start, shared, True, ml)
        fd, pd = layer_ops.stop_update(toks[:, t].to(DEV), t, spec, *dev, start.to(DEV), shared.to(DEV), True,
                                       max_len=None if ml is None else ml.to(DEV))
        for k, (a, b) in enumerate(zip((fr, pr) + ref, (fd, pd) + dev)):
            assert torch.equal(a, b.cpu()), (t, k)
    if limited:
        assert (ref[2] == stopping.LIMIT).any() and (ref[2] == stopping.EOS).any() and (ref[2] == stopping.STOP).any()
        out, length, reason, index = stopping.truncate_reference(toks, spec, max_len)
        assert all(torch.equal(a, b) for a, b in zip((out, length, reason, index), ref[:4]))


# ---- generate() ---------------------------------------------------------------------------------------------------------------------
NEW = 8
LEAF_T = [0.0, 0.8, 0.0, 1.3]          # per prompt of the innermost level (repeated for the two samples of each)
LEAF_K = [None, 40, 5, None]
LEAF_P = [0.9, None, None, 0.5]
LEAF_REP = [None, 1.3, None, 1.1]
LEAF_SEED = [11, 2 ** 63 + 5, 7, 2 ** 40]
LIMITS = [1, 8, 3, 5, 8, 2, 6, 4]      # per row of the batch


def _model(mode):
    from hydragen_amd.kv_quant import FP8_DTYPE
    from tests.test_model_gpu import make_model

    fp8 = mode == "fp8"
    model = make_model(torch.float16, head_dim=128 if fp8 else 64, kv_heads=4 if fp8 else 2)
    model.graph(mode != "eager")
    model.setup_caches(max_unique_batch_size=8, max_unique_seq_length=8 + NEW, max_shared_batch_sizes=[1, 4], max_shared_seq_lengths=[24, 8],
                       kv_cache_dtype=FP8_DTYPE if fp8 else None)
    return model


def _levels(perm=None):
    g = torch.Generator(device=DEV).manual_seed(21)
    ids = [torch.randint(1, 512, (1, 20), device=DEV, generator=g), torch.randint(1, 512, (4, 8), device=DEV, generator=g)]
    lens = [torch.tensor([20], device=DEV), torch.tensor([8, 5, 8, 3], device=DEV)]
    if perm is not None:
        ids[1], lens[1] = ids[1][perm], lens[1][perm]
    return dict(input_ids=ids, seq_lens=lens, num_return_sequences=2, max_new_tokens=NEW)


@pytest.mark.parametrize("mode", ["eager", "graph", "fp8"])
def test_generate_per_row(mode):
    model = _model(mode)
    kw = _levels()

    def gen(torch_seed=3, **more):
        torch.manual_seed(torch_seed)
        return model.generate(**dict(kw, **more))

    # 1. lists whose rows are all equal: the scalar call's tokens under the same torch.manual_seed
    scalar = gen(temperature=0.8, top_k=40, top_p=0.9, repetition_penalty=1.2)
    assert scalar.shape == (8, NEW)
    assert torch.equal(gen(temperature=[0.8] * 4, top_k=[40] * 8, top_p=torch.tensor([0.9] * 4), repetition_penalty=[1.2] * 8), scalar)
    # 2. the greedy rows of a mixed call are the rows of an all-greedy call
    cuts = dict(top_k=LEAF_K, top_p=LEAF_P, repetition_penalty=LEAF_REP)
    mixed, greedy = gen(temperature=LEAF_T, **cuts), gen(temperature=0.0, **cuts)
    zero = torch.tensor([t == 0 for t in LEAF_T]).repeat_interleave(2)
    assert torch.equal(mixed[zero], greedy[zero]) and not torch.equal(mixed[~zero], greedy[~zero])
    # 3. seed=: permuting the prompts permutes the outputs, and torch's generator plays no part
    seeded = gen(temperature=LEAF_T, seed=LEAF_SEED, **cuts)
    assert torch.equal(gen(torch_seed=99, temperature=LEAF_T, seed=LEAF_SEED, **cuts), seeded)
    perm = [2, 0, 3, 1]
    pick = lambda v: [v[i] for i in perm]  # noqa: E731
    torch.manual_seed(5)
    permuted = model.generate(**dict(_levels(torch.tensor(perm, device=DEV)), temperature=pick(LEAF_T), top_k=pick(LEAF_K), top_p=pick(LEAF_P),
                                     repetition_penalty=pick(LEAF_REP), seed=pick(LEAF_SEED)))
    rows = torch.tensor([2 * i + s for i in perm for s in (0, 1)], device=DEV)
    assert torch.equal(permuted, seeded[rows])
    # a seed per row of the batch: the two samples of a prompt differ where they sample
    per_row = gen(temperature=LEAF_T, seed=list(range(100, 108)), **cuts)
    assert not torch.equal(per_row[2::4], per_row[3::4]) and torch.equal(per_row[zero], seeded[zero])
    # 4. a limit per row: lengths == limits, reason 3, pad behind, the columns before the limit those of the unlimited call
    free, fin0 = gen(temperature=LEAF_T, seed=LEAF_SEED, pad_token_id=0, return_finish=True, **cuts)
    assert torch.equal(free, seeded) and (fin0.reasons == 0).all()
    out, fin = gen(temperature=LEAF_T, seed=LEAF_SEED, pad_token_id=0, return_finish=True, max_new_tokens=LIMITS, **cuts)
    lim = torch.tensor(LIMITS, device=DEV)
    assert out.shape == (8, max(LIMITS)) and torch.equal(fin.lengths.long(), lim)
    assert (fin.reasons == stopping.LIMIT).all() and (fin.stop_index == -1).all()
    before = torch.arange(NEW, device=DEV)[None, :] < lim[:, None]
    assert torch.equal(out, torch.where(before, free, torch.zeros_like(free)))
    # ... and an EOS id still ends a row first
    eos = int(free[1, 2])
    out2, fin2 = gen(temperature=LEAF_T, seed=LEAF_SEED, eos_token_id=[eos], pad_token_id=0, return_finish=True, max_new_tokens=LIMITS, **cuts)
    want = stopping.truncate_reference(free.cpu(), stopping.check_stop([eos], None, 0, False, 512), torch.tensor(LIMITS))
    assert torch.equal(out2.cpu(), want[0][:, : int(want[1].max())]) and torch.equal(fin2.lengths.cpu(), want[1]) and torch.equal(fin2.reasons.cpu(), want[2])
    assert (want[2] == stopping.EOS).any()
