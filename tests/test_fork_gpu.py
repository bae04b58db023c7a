"""-m gpu: fork completions on the device -- hyd_kv_promote against its torch definition (exact), the model's fork through the
kernel and through torch (bit-identical logits), a forked hierarchy against the same tokens decoded without a fork (the
decomposition bound of tests/test_model_gpu.py), graph replay across two forks, the beam-search driver, and the refusals."""
import pytest
import torch

from tests.test_model_gpu import make_model, rdiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = torch.float8_e4m3fn


# ---- 1. the kernel against promote_kv_reference -----------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8)


def _source(dtype, Hkv, d, seed):
    """K and V views of a real arena of batch 6 and 48 rows (the batch stride is the arena's), filled with random BYTES: NaNs of
    every payload for the 16-bit copy, every e4m3fn code for the widening."""
    from hydragen_amd import placement

    arena = placement.kv_arena((6, 48, Hkv, d), dtype, DEV, zero=True)
    g = torch.Generator(device=DEV).manual_seed(seed)
    raw = _bits(arena)
    if dtype == FP8:
        raw.copy_(torch.randint(0, 256, tuple(raw.shape), device=DEV, generator=g).to(torch.uint8))
    else:
        raw.copy_((torch.randint(0, 65536, tuple(raw.shape), device=DEV, generator=g) - 32768).to(torch.int16))
    k, v = arena[0], arena[1]
    assert k.stride(0) == 2 * 48 * Hkv * d and v.data_ptr() != k.data_ptr()
    if dtype == FP8:  # NaN (both signs) and +-448 in chosen places of rows that are promoted
        special = torch.tensor([0x7F, 0xFF, 0x7E, 0xFE, 0x00, 0x80, 0x01, 0x81], dtype=torch.uint8, device=DEV)
        for t in (k, v):
            t.view(torch.uint8)[4, 0, :, :8] = special
            t.view(torch.uint8)[2, 14, -1, -8:] = special
    return k, v


CONFIGS = ([(dt, dt, h, d, d) for dt in (torch.bfloat16, torch.float16) for h in (1, 4, 8) for d in (64, 128, 256)]
           + [(torch.bfloat16, torch.bfloat16, 8, 80, 128), (torch.bfloat16, torch.bfloat16, 8, 96, 128),
              (torch.bfloat16, torch.bfloat16, 4, 192, 256)]
           + [(FP8, dt, 8, d, d, sc) for dt in (torch.bfloat16, torch.float16) for d in (64, 128) for sc in (True, False)])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(str(x).replace("torch.", "") for x in c))
def test_promote_kernel_equals_reference_bit_for_bit(cfg):
    from hydragen_amd.fork import promote_kv, promote_kv_reference

    src_dtype, dtype, Hkv, d, D = cfg[:5]
    scaled = len(cfg) > 5 and cfg[5]
    k, v = _source(src_dtype, Hkv, d, seed=Hkv * 1000 + d)
    kw = {}
    if scaled:  # non-power-of-two per-head scales
        kw = dict(k_scale=(torch.arange(Hkv, device=DEV).float() * 0.37 + 0.11), v_scale=(torch.arange(Hkv, device=DEV).float() * 0.053 + 1.3))
    rows = torch.tensor([4, 0, 5, 2], device=DEV)
    g = torch.Generator().manual_seed(d + Hkv)
    choices = torch.tensor([1, 15, 16, 17, 48])
    draws = [choices[torch.randint(0, 5, (4,), generator=g)].tolist() for _ in range(2)] + [[15, 48, 1, 17], [17, 17, 17, 17]]
    for lens_l in draws:
        lens = torch.tensor(lens_l, device=DEV)
        total, cap = sum(lens_l), sum(lens_l) + 9
        outs = []
        for fn, extra in ((promote_kv, dict(max_len=max(lens_l))), (promote_kv, {}), (promote_kv_reference, {})):
            kd = torch.empty((cap, Hkv, D), dtype=dtype, device=DEV)
            vd = torch.empty_like(kd)
            _bits(kd).fill_(0x5A5A)
            _bits(vd).fill_(0x3C3C)
            cu = fn(k, v, rows, lens, kd, vd, **kw, **extra)
            assert cu.dtype == torch.int32 and cu.tolist() == [0] + torch.tensor(lens_l).cumsum(0).tolist()
            outs.append((kd, vd))
        (k1, v1), (k2, v2), (kr, vr) = outs
        for got in ((k1, v1), (k2, v2)):
            for a, b, fill in ((got[0], kr, 0x5A5A), (got[1], vr, 0x3C3C)):
                assert torch.equal(_bits(a), _bits(b)), (cfg, lens_l, (_bits(a) != _bits(b)).nonzero()[:4].tolist())
                assert bool((_bits(a[total:]) == fill).all())        # rows at or past cu[n] keep the sentinel
                assert not _bits(a[:total, :, d:]).any()              # pad columns of written rows are zero
        if src_dtype != FP8:  # the 16-bit route is a byte copy of the source rows
            at = 0
            for r, n in zip([4, 0, 5, 2], lens_l):
                assert torch.equal(_bits(k1[at : at + n, :, :d]), _bits(k[r, :n])) and torch.equal(_bits(v1[at : at + n, :, :d]), _bits(v[r, :n]))
                at += n


def test_promote_kernel_skips_sequences_with_bad_device_data():
    """rows outside [0, B), a length over the source's rows (or over max_len), an offset past the capacity: the sequence is
    skipped, the others are copied, nothing outside the destination is written (a guard tensor behind it stays intact)."""
    import ctypes as C

    from hydragen_amd import _lib
    from hydragen_amd.flash import _stream

    k, v = _source(torch.bfloat16, 4, 64, seed=9)
    pool = torch.full((2, 40 + 8, 4, 64), 3.0, dtype=torch.bfloat16, device=DEV)  # 40 destination tokens + 8 guard tokens each
    kd, vd = pool[0, :40], pool[1, :40]
    rows = torch.tensor([1, 6, -1, 2, 3, 5], dtype=torch.int32, device=DEV)
    lens = torch.tensor([5, 4, 4, 49, 7, 20], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 5, 9, 13, 17, 24, 44], dtype=torch.int32, device=DEV)     # the last one: 24 + 20 > 40
    p = _lib.KvPromoteParams()
    p.k_src, p.v_src, p.k_dst, p.v_dst = k.data_ptr(), v.data_ptr(), kd.data_ptr(), vd.data_ptr()
    p.rows, p.lens, p.cu = rows.data_ptr(), lens.data_ptr(), cu.data_ptr()
    p.k_batch_stride, p.k_tok_stride, p.k_head_stride = k.stride(0), k.stride(1), k.stride(2)
    p.v_batch_stride, p.v_tok_stride, p.v_head_stride = v.stride(0), v.stride(1), v.stride(2)
    p.src_dtype = p.dst_dtype = _lib.HYD_BF16
    p.n, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst, p.capacity, p.max_len = 6, 6, 48, 4, 64, 64, 40, 0
    _lib.check(_lib.load().hyd_kv_promote(C.byref(p), _stream()))
    torch.cuda.synchronize()
    want = torch.full_like(pool, 3.0)
    want[0, 0:5], want[1, 0:5] = k[1, :5], v[1, :5]
    want[0, 17:24], want[1, 17:24] = k[3, :7], v[3, :7]
    assert torch.equal(_bits(pool), _bits(want))


# ---- 2. / 3. the model ------------------------------------------------------------------------------------------------------
def _set_scales(model):
    for i, layer in enumerate(model.model.layers):
        kv = layer.self_attn.kv_cache
        n = kv.k_scale.numel()
        kv.k_scale.copy_(torch.arange(n, device=DEV).float() * 0.21 + 0.6 + 0.1 * i)
        kv.v_scale.copy_(torch.arange(n, device=DEV).float() * 0.13 + 0.45 + 0.1 * i)


def _fork_and_continue(model, prefix, ov, n, m, rows, lens, expand, use_kernel=True, wipe=True):
    """generate n tokens (teacher-forced) with "extend", fork `rows` with `lens` promoted tokens, then m teacher-forced steps of
    `expand` children per row -> list of m logits [len(rows) * expand, V]."""
    B = ov.shape[0]
    model.generate(input_ids=prefix, num_return_sequences=B, max_new_tokens=n, temperature=0.0, token_overrides=ov[:, :n],
                   shared_cache_op="wipe" if wipe else "extend")
    # ("wipe" empties the levels first and keeps what the call adds, like "extend")
    r = torch.tensor(rows, device=DEV)
    L = torch.tensor(lens, device=DEV)
    ids = ov[r, : max(lens)]
    used = model.fork(rows, lens, ids, old_batch=B, use_kernel=use_kernel)
    first = ov[r, L].repeat_interleave(expand, 0)[:, None]                       # the first token not promoted
    cont = torch.stack([ov[ri, li + 1 : li + 1 + m] for ri, li in zip(rows, lens)]).repeat_interleave(expand, 0)
    _, logits = model.generate(input_ids=first, num_return_sequences=1, max_new_tokens=m, temperature=0.0, return_logits=True,
                               token_overrides=cont, shared_cache_op="extend")
    return used, ids, L, logits


@pytest.mark.parametrize("kind", ["fp16", "bf16", "bf16-fp8kv"])
def test_model_fork_kernel_route_equals_torch_route(kind):
    from hydragen_amd import layer_ops

    dtype = torch.float16 if kind == "fp16" else torch.bfloat16
    model = make_model(dtype, head_dim=128, kv_heads=4) if kind != "fp16" else make_model(dtype, head_dim=64, kv_heads=2)
    g = torch.Generator(device=DEV).manual_seed(11)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    prefix, n, m, B = rnd(1, 50), 8, 6, 6
    ov = rnd(B, n + m)
    model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=16, max_shared_batch_sizes=[1, 3], max_shared_seq_lengths=[50, n],
                       kv_cache_dtype=FP8 if kind.endswith("fp8kv") else None)
    if kind.endswith("fp8kv"):
        _set_scales(model)
    rows, lens = [5, 0, 3], [n - 1, n - 3, n - 2]
    results = []
    for use_kernel in (True, False):
        used, ids, L, logits = _fork_and_continue(model, prefix, ov, n, m, rows, lens, 2, use_kernel=use_kernel)
        assert used == model.get_num_used_shared_caches() == 2
        assert len(model.shared_bitmaps) == 2
        assert torch.equal(model.shared_bitmaps[1], layer_ops.token_bitmap(ids.long(), L.long(), model.vocab_size))
        sc = model.model.layers[-1].self_attn.kv_cache.shared_caches[1]
        assert sc.use_varlen and sc.current_batch_size == 3 and sc.seq_lens[:3].tolist() == lens
        results.append((torch.stack(logits), sc.k_cache.clone(), sc.v_cache.clone()))
    (la, ka, va), (lb, kb, vb) = results
    assert torch.equal(_bits(ka), _bits(kb)) and torch.equal(_bits(va), _bits(vb))   # the same level buffers ...
    assert torch.equal(la, lb)                                                    # ... into the same launches: the same logits


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("geom", [(128, 4), (64, 2)])
def test_forked_hierarchy_against_unforked_decode(dtype, geom):
    """The decomposition check: a row's logits after a fork (prefix level + promoted level + the children's own keys) against the
    same tokens decoded in one generate() (prefix level + unique keys), under the bound test_hydragen_vs_nosharing_and_flat_hierarchy
    uses for "same math, other decomposition"; the children of one row are bit-identical to each other."""
    bound = 0.02 if dtype == torch.float16 else 0.08
    model = make_model(dtype, head_dim=geom[0], kv_heads=geom[1])
    g = torch.Generator(device=DEV).manual_seed(5)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    prefix, n, m, B, expand = rnd(1, 50), 8, 6, 6, 2
    ov = rnd(B, n + m)
    model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=16, max_shared_batch_sizes=[1, 3], max_shared_seq_lengths=[50, n])
    _, a = model.generate(input_ids=prefix, num_return_sequences=B, max_new_tokens=n + m, temperature=0.0, return_logits=True,
                          token_overrides=ov, shared_cache_op="wipe")
    a = torch.stack(a)  # [n + m, B, V]; a[j] is the distribution after ov[:, :j]
    model.empty_shared_cache()
    rows = [5, 0, 3]
    for lens in ([n - 1] * 3, [n - 1, n - 3, n - 2]):
        used, _, _, b = _fork_and_continue(model, prefix, ov, n, m, rows, lens, expand)
        assert used == 2
        b = torch.stack(b)  # [m, 3 * expand, V]
        assert torch.equal(b[:, 0::2], b[:, 1::2])     # the two children of one row
        want = torch.stack([a[li + 1 : li + 1 + m, ri] for ri, li in zip(rows, lens)], dim=1)   # [m, 3, V]
        err = rdiff(b[:, 0::2], want).mean()
        print(f"forked vs unforked {dtype} {geom} lens {lens}: mean rdiff {float(err):.5f} (bound {bound})")
        assert err < bound
        model.empty_shared_cache()


# ---- 4. graph replay ------------------------------------------------------------------------------------------------------
def test_second_fork_replays_the_captured_graph():
    """Two fork-and-continue rounds with the same k and different ragged lengths on a graphed model: the second round REPLAYS the
    graph the first one captured (same key: batch sizes, varlen flags, sliced lengths; the level's buffers are static), and each
    round's logits are bit-identical to the same round on an eager model with the same weights.  The forked rows are cached by a
    unique prefill (max_new_tokens=1: no decode step), so nothing re-captures the graph between the rounds.  (Eager and graphed
    decode steps are bitwise equal without a fork too: asserted first, on an unforked pair.)"""
    eager, graphed = make_model(torch.bfloat16, head_dim=128, kv_heads=4), make_model(torch.bfloat16, head_dim=128, kv_heads=4)
    graphed.graph(True)
    g = torch.Generator(device=DEV).manual_seed(21)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    prefix, B, n, m = rnd(1, 50), 6, 10, 5
    uniq, ov = rnd(B, n), rnd(B, n + m)
    for mdl in (eager, graphed):
        mdl.setup_caches(max_unique_batch_size=B, max_unique_seq_length=32, max_shared_batch_sizes=[1, 3], max_shared_seq_lengths=[50, n])
    # the unforked pair
    kw = dict(input_ids=prefix, num_return_sequences=B, max_new_tokens=m, temperature=0.0, return_logits=True, token_overrides=ov[:, :m])
    assert torch.equal(torch.stack(eager.generate(**kw)[1]), torch.stack(graphed.generate(**kw)[1]))

    rows = [4, 1, 2]
    captured = None
    for lens in ([9, 4, 7], [3, 10, 6]):
        out = []
        for mdl in (eager, graphed):
            mdl.generate(input_ids=[prefix, uniq], num_return_sequences=1, max_new_tokens=1, temperature=0.0, shared_cache_op="wipe")
            r, L = torch.tensor(rows, device=DEV), torch.tensor(lens, device=DEV)
            assert mdl.fork(r, L, uniq[r, : max(lens)], old_batch=B) == 2
            first = torch.where(L < n, uniq[r, L.clamp(max=n - 1)], ov[r, 0]).repeat_interleave(2, 0)[:, None]
            _, logits = mdl.generate(input_ids=first, num_return_sequences=1, max_new_tokens=m, temperature=0.0, return_logits=True,
                                     token_overrides=ov[r, 1 : 1 + m].repeat_interleave(2, 0), shared_cache_op="extend")
            out.append(torch.stack(logits))
        assert torch.equal(out[0], out[1]), lens
        cd = graphed.graphed_model.capture_data
        assert cd is not None
        if captured is None:
            captured = cd
        assert cd is captured, "the second fork re-captured the decode graph"


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2])
def test_stepwise_beam_search_is_consistent_with_its_trace(G):
    from hydragen_amd.fork import select_beams, stepwise_beam_search

    width, expand, T, steps = 2, 3, 4, 3
    model = make_model(torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(31 + G)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    levels = rnd(1, 20) if G == 1 else [rnd(1, 20), rnd(2, 7)]
    sb = [1, 2, 2] if G == 1 else [1, 2, 4, 4]
    sl = [20, T, T] if G == 1 else [20, 7, T, T]
    model.setup_caches(max_unique_batch_size=G * width * expand, max_unique_seq_length=16, max_shared_batch_sizes=sb, max_shared_seq_lengths=sl)
    before = model.get_num_used_shared_caches()
    tokens, scores, trace = stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=steps,
                                                 return_trace=True, temperature=1.0)
    assert model.get_num_used_shared_caches() == before == len(model.shared_bitmaps)
    assert tokens.shape == (G * width, steps * T) and scores.shape == (G * width,) and len(trace) == steps
    paths = lps = None
    for s, t in enumerate(trace):
        group, keep = (width * expand, width) if s == 0 else (expand, 1)
        assert (t["group_size"], t["width"]) == (group, keep) and t["candidate_scores"].shape == (G * width * expand,)
        assert t["rows"].tolist() == select_beams(t["candidate_scores"], group, keep).tolist()
        assert t["parents"].tolist() == (t["rows"] // group).tolist()
        assert t["tokens"].shape == (G * width, T) and t["logprobs"].shape == (G * width, T)
        paths = t["tokens"] if s == 0 else torch.cat([paths[t["parents"]], t["tokens"]], dim=1)
        lps = t["logprobs"] if s == 0 else torch.cat([lps[t["parents"]], t["logprobs"]], dim=1)
        kept = {tuple(p) for p in paths.tolist()}
        for p in tokens.cpu().tolist():  # every returned path's step-s prefix is one of round s's kept beams
            assert tuple(p[: (s + 1) * T]) in kept
        # the candidates' scores are the cumulative log-probs: the kept ones are the sums of their paths' per-round log-probs
        assert torch.allclose(t["candidate_scores"][t["rows"]], lps.sum(1), atol=1e-4, rtol=1e-5)
    assert torch.equal(tokens.cpu(), paths)
    assert torch.allclose(scores.cpu(), lps.sum(1), atol=1e-4, rtol=1e-5)
    assert bool((lps <= 0).all()) and bool(lps.isfinite().all())

    calls = []

    def failing(tok, lp):
        calls.append(tok.shape)
        if len(calls) == 2:
            raise RuntimeError("scorer failed")
        return lp.sum(1)

    with pytest.raises(RuntimeError, match="scorer failed"):
        stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=steps, score_fn=failing, temperature=1.0)
    assert calls == [(G * width * expand, T), (G * width * expand, 2 * T)]
    assert model.get_num_used_shared_caches() == before == len(model.shared_bitmaps)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_fork_refusals_leave_levels_and_bitmaps_alone():
    model = make_model(torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(41)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    prefix, B, n = rnd(1, 20), 6, 8
    ov = rnd(B, n)
    with pytest.raises(RuntimeError, match="setup_caches"):
        model.fork([0], [1], ov[:1, :1], old_batch=B)
    model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=16, max_shared_batch_sizes=[1, 3], max_shared_seq_lengths=[20, 6])
    model.generate(input_ids=prefix, num_return_sequences=B, max_new_tokens=n, temperature=0.0, token_overrides=ov, shared_cache_op="extend")
    kv = model.model.layers[0].self_attn.kv_cache
    level = kv.shared_caches[1]
    snap = lambda: (model.get_num_used_shared_caches(), len(model.shared_bitmaps), level.k_cache.clone(), level.seq_lens.clone())

    def unchanged(s):
        now = snap()
        assert now[:2] == s[:2] and torch.equal(now[2], s[2]) and torch.equal(now[3], s[3])

    s0 = snap()
    assert s0[:2] == (1, 1)
    for rows, lens, frag in (([0, 1, 2, 3], [1, 1, 1, 1], "Batch size 4 exceeds max batch size 3"),
                             ([5, 0, 3], [6, 7, 6], "Sequence length 7 exceeds max sequence length 6"),
                             ([5, 0, 3], [6, 0, 6], "at least 1"),
                             ([5, 5, 3], [1, 1, 1], "repeats"),
                             ([5, 0, 6], [1, 1, 1], "outside the previous batch")):
        with pytest.raises(ValueError, match=frag):
            model.fork(rows, lens, ov[rows if max(rows) < B else [0, 0, 0], : max(lens)], old_batch=B)
        unchanged(s0)
    with pytest.raises(ValueError, match="token_ids"):
        model.fork([5, 0, 3], [6, 4, 6], ov[[5, 0, 3], :5], old_batch=B)
    unchanged(s0)
    assert model.fork([5, 0, 3], [6, 4, 6], ov[[5, 0, 3], :6], old_batch=B) == 2
    s1 = snap()
    assert s1[:2] == (2, 2)
    with pytest.raises(ValueError, match="No more available shared caches"):
        model.fork([0, 1, 2], [1, 1, 1], ov[:3, :1], old_batch=3)
    unchanged(s1)
