"""-m gpu: calibrated fp8 K/V scales on the device -- hyd_kv_absmax and hyd_kv_scales_from_absmax against their definitions in
torch (bit for bit), the fp8 suffix operator with calibrated against unit scales, and the model shell's kv_scales="calibrate":
power-of-two equivariance of a whole model, the freeze / reset rule, and the untouched default."""
import pytest
import torch

from hydragen_amd import _lib, placement
from hydragen_amd import kv_quant as Q
from tests import kv_scale_cases as cases
from tests.test_fp8_kv import FP8_REL_L2_BOUND
from tests.test_model_gpu import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = Q.FP8_DTYPE
NAN, INF = float("nan"), float("inf")


def rows_per_workgroup(Hkv, d):
    """include/hydragen_hip.h: the consecutive rows of one outer index a workgroup of hyd_kv_absmax covers."""
    return _lib.KV_ABSMAX_PASSES * max(1, 256 // (Hkv * d // 8))


def _rand(shape, dtype, gen, spread=True):
    x = torch.randn(shape, device=DEV, generator=gen)
    if spread:  # magnitudes over many binades, so that a wrong element shows in the maximum
        x = x * torch.exp2(torch.randint(-12, 6, shape, device=DEV, generator=gen).float())
    return x.to(dtype)


def _poison(t, gen):
    """NaN / +inf / -inf, mixed."""
    pick = torch.randint(0, 3, t.shape, device=DEV, generator=gen)
    t.copy_(torch.where(pick == 0, torch.full_like(t, NAN), torch.where(pick == 1, torch.full_like(t, INF), torch.full_like(t, -INF))))


def make_views(kind, n_outer, n_rows, Hkv, d, dtype, gen):
    """-> (k, v) views of the given kind at its native strides, everything outside the views poisoned."""
    if kind == "gemm_split":  # the k / v splits of a fused q|k|v GEMM output
        Hq = 2 * Hkv
        buf = _rand((n_outer, n_rows, (Hq + 2 * Hkv) * d), dtype, gen)
        q, k, v = buf.split([Hq * d, Hkv * d, Hkv * d], dim=-1)
        _poison(q, gen)
        return k.view(n_outer, n_rows, Hkv, d), v.view(n_outer, n_rows, Hkv, d)
    if kind == "shared_slice":  # [:sb, :P, :, :d] of a cache [sb_max, P_max, Hkv, D], D > d
        D = next((w for w in (64, 128, 256) if w > d), d + 8)
        out = []
        for _ in range(2):
            cache = torch.empty((n_outer + 1, n_rows + 3, Hkv, D), dtype=dtype, device=DEV)
            _poison(cache, gen)
            view = cache[:n_outer, :n_rows, :, :d]
            view.copy_(_rand(view.shape, dtype, gen))
            out.append(view)
        return tuple(out)
    if kind == "packed_level":  # [sum P, Hkv, D] packed level: three dimensions
        return tuple(_rand((n_outer * n_rows, Hkv, d), dtype, gen) for _ in range(2))
    assert kind == "arena_halves"  # the two halves of a placement.kv_arena: [batch, K | V, rows, heads, dim] in memory
    arena = placement.kv_arena((n_outer, n_rows, Hkv, d), dtype, DEV, zero=True)
    arena.copy_(_rand(arena.shape, dtype, gen))
    assert arena[0].stride(0) == 2 * n_rows * Hkv * d
    return arena[0], arena[1]


KINDS = ("gemm_split", "shared_slice", "packed_level", "arena_halves")
GEOMS = sorted({(8, d) for d in (8, 64, 80, 96, 128, 192, 256)} | {(h, d) for h in (1, 2, 3, 8, 32) for d in (128, 96)})


def _observe(k, v, row_lens=None, amax=None):
    Hkv = (k if k is not None else v).shape[-2]
    amax = torch.zeros((2, Hkv), device=DEV) if amax is None else amax
    Q.observe_absmax(k, v, amax, row_lens)
    return amax


# ---- 1. kernel == definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv, d", GEOMS)
def test_absmax_kernel_equals_definition(Hkv, d):
    gen = torch.Generator(device=DEV).manual_seed(Hkv * 1000 + d)
    n = 0
    for dtype in (torch.bfloat16, torch.float16):
        for kind in KINDS:
            for n_rows in (1, 7, 64, 65, 1000):
                n_outer = (1, 3)[n % 2] if n_rows < 1000 or Hkv * d <= 1024 else 1
                n += 1
                k, v = make_views(kind, n_outer, n_rows, Hkv, d, dtype, gen)
                got = _observe(k, v)
                want = Q.absmax_reference(k, v)
                assert torch.equal(got, want), (dtype, kind, n_outer, n_rows, got, want)
                assert bool((got > 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_absmax_matches_the_cpu_definition_on_the_largest_case(dtype):
    gen = torch.Generator(device=DEV).manual_seed(3)
    k, v = make_views("gemm_split", 1, 1000, 32, 256, dtype, gen)  # 16 MB each
    assert torch.equal(_observe(k, v).cpu(), Q.absmax_reference(k.cpu(), v.cpu()))


# ---- 2. where the maximum sits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv, d, dtype", [(8, 128, torch.bfloat16), (3, 96, torch.float16), (32, 128, torch.float16),
                                           (1, 8, torch.bfloat16), (2, 64, torch.bfloat16)])
def test_absmax_finds_the_largest_element_wherever_it_is(Hkv, d, dtype):
    gen = torch.Generator(device=DEV).manual_seed(Hkv + d)
    R = rows_per_workgroup(Hkv, d)
    n_outer, n_rows = 2, 2 * R + 5  # three workgroups along the rows of each outer index
    base_k = (_rand((n_outer, n_rows, Hkv, d), dtype, gen, spread=False).float().clamp(-3, 3) / 4).to(dtype)  # |x| < 1
    base_v = base_k.flip(1).contiguous()
    spots = [(0, 0, 0, 0), (0, 0, Hkv - 1, d - 1), (n_outer - 1, n_rows - 1, 0, 0), (n_outer - 1, n_rows - 1, Hkv - 1, d - 1),
             (0, R - 1, Hkv // 2, 3), (0, R, Hkv // 2, 3), (1, 2 * R - 1, 0, d - 1), (1, 2 * R, Hkv - 1, 0)]
    spots += [(1, 5, h, d - 8 + h % 8) for h in range(Hkv)]  # every head in turn, in the last 8-element piece of its row
    for i, (o, r, h, c) in enumerate(spots):
        for which in (0, 1):
            k, v = base_k.clone(), base_v.clone()
            big = (-1) ** i * (7.0 + i)  # every other placement negative
            (k, v)[which][o, r, h, c] = big
            want = Q.absmax_reference(k, v)
            assert want[which, h] == abs(big)
            assert torch.equal(_observe(k, v), want), (o, r, h, c, which)
    # a lone subnormal in a tensor of zeros (and of negative zeros)
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    k, v = torch.zeros_like(base_k), -torch.zeros_like(base_k)
    k.view(torch.int16)[1, n_rows - 2, Hkv - 1, 5] = -32767  # bits 0x8001: minus the smallest subnormal
    got = _observe(k, v).cpu()
    assert got[0, Hkv - 1].item() == tiny and int((got != 0).sum()) == 1
    assert torch.equal(got, Q.absmax_reference(k.cpu(), v.cpu()))


# ---- 3. what must not be read, what must not count ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv, d, dtype", [(8, 128, torch.bfloat16), (3, 96, torch.float16), (8, 64, torch.float16), (2, 80, torch.bfloat16)])
def test_absmax_ignores_poison_outside_the_lengths_and_nonfinite_inside(Hkv, d, dtype):
    gen = torch.Generator(device=DEV).manual_seed(17 * Hkv + d)
    R = rows_per_workgroup(Hkv, d)
    n_outer, n_rows = 4, 2 * R + 9
    lens = torch.tensor([n_rows, 0, R + 1, 5], dtype=torch.int32, device=DEV)
    inside = (torch.arange(n_rows, device=DEV)[None, :] < lens[:, None])[:, :, None, None]
    D = next((w for w in (64, 128, 256) if w > d), d + 8)
    views, clean = [], []
    for _ in range(2):
        cache = torch.empty((n_outer, n_rows, Hkv, D), dtype=dtype, device=DEV)
        _poison(cache, gen)  # columns >= d and rows >= lens stay poisoned
        data = _rand((n_outer, n_rows, Hkv, d), dtype, gen)
        view = cache[..., :d]
        view.copy_(torch.where(inside, data, view))
        views.append(view)
        clean.append(torch.where(inside, data, torch.zeros_like(data)))
    want = Q.absmax_reference(clean[0], clean[1])
    assert bool(torch.isfinite(want).all()) and bool((want > 0).all())
    assert torch.equal(_observe(views[0], views[1], lens), want)
    assert torch.equal(Q.absmax_reference(views[0], views[1], lens), want)  # (the definition agrees with itself)
    assert torch.equal(_observe(views[0], views[1], lens.long()), want)     # int64 lengths are converted
    # NaN / inf INSIDE the range never raise the maximum
    k, v = clean[0].clone(), clean[1].clone()
    hit = torch.rand(k.shape, device=DEV, generator=gen) < 0.05
    for t in (k, v):
        bad = torch.empty_like(t)
        _poison(bad, gen)
        t.copy_(torch.where(hit, bad, t))
    got = _observe(k, v)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, Q.absmax_reference(k, v))
    all_bad = torch.empty_like(k)
    _poison(all_bad, gen)
    assert torch.equal(_observe(all_bad, all_bad), torch.zeros((2, Hkv), device=DEV))


def test_absmax_keeps_a_running_maximum():
    gen = torch.Generator(device=DEV).manual_seed(5)
    Hkv, d = 8, 128
    k1, v1 = make_views("gemm_split", 2, 70, Hkv, d, torch.bfloat16, gen)
    k2, v2 = make_views("packed_level", 1, 33, Hkv, d, torch.bfloat16, gen)
    a1, a2 = Q.absmax_reference(k1, v1), Q.absmax_reference(k2, v2)
    assert not torch.equal(torch.maximum(a1, a2), a1) and not torch.equal(torch.maximum(a1, a2), a2)
    amax = _observe(k1, v1)
    _observe(k2, v2, amax=amax)
    assert torch.equal(amax, torch.maximum(a1, a2))
    # a larger value that is already there survives
    pre = torch.maximum(a1, a2).clone()
    pre[0, 3], pre[1, 0] = 1e30, 65536.0
    amax = pre.clone()
    _observe(k1, v1, amax=amax)
    assert torch.equal(amax, pre)
    # K alone / V alone leave the other row as it is
    amax = torch.full((2, Hkv), 2.0 ** -140, device=DEV)
    _observe(k1, None, amax=amax)
    assert torch.equal(amax[0], a1[0]) and bool((amax[1] == 2.0 ** -140).all())
    _observe(None, v2, amax=amax)
    assert torch.equal(amax[0], a1[0]) and torch.equal(amax[1], a2[1])
    # nothing to read: nothing changes
    _observe(k1[:, :0], v1[:, :0], amax=amax)
    assert torch.equal(amax[0], a1[0]) and torch.equal(amax[1], a2[1])


# ---- 4. the scale rule ------------------------------------------------------------------------------------------------------------------
def test_scales_kernel_equals_definition_bit_for_bit():
    f32 = lambda xs: torch.tensor(xs, dtype=torch.float64).to(torch.float32)  # noqa: E731
    p2 = [2.0 ** k for k in range(-126, 128, 9)]
    edge = f32(p2 + [224 * x for x in p2[2:-2]] + [225 * x for x in p2[2:-2]]
               + [0.0, 65504.0, float(torch.finfo(torch.bfloat16).max), 2.0 ** -24, 2.0 ** -133, 2.0 ** -149, 1e-38, 2.0 ** -93, 448.0, 449.0])
    edge = torch.cat([edge, torch.nextafter(f32(p2), f32([INF] * len(p2))), torch.nextafter(f32(p2), f32([0.0] * len(p2)))])
    gen = torch.Generator().manual_seed(1)
    edge = torch.cat([edge, torch.rand(64, generator=gen) * torch.exp2(torch.randint(-40, 40, (64,), generator=gen).float())])
    amax = torch.stack([edge, edge.flip(0)]).contiguous()
    Hkv = edge.numel()
    for margin in (2.0, 1.0, 448.0, 3.7, 1e6):
        for pow2 in (True, False):
            want = Q.scales_from_absmax_reference(amax, margin, pow2)
            ks, vs = torch.full((Hkv,), -1.0, device=DEV), torch.full((Hkv,), -1.0, device=DEV)
            Q.scales_from_absmax(amax.to(DEV), ks, vs, margin, pow2)
            got = torch.stack([ks, vs]).cpu()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (margin, pow2, got[got != want], want[got != want])


def test_observe_and_scales_replay_in_a_captured_graph():
    gen = torch.Generator(device=DEV).manual_seed(9)
    Hkv, d = 4, 128
    buf = _rand((2, 40, 4 * Hkv * d), torch.bfloat16, gen)
    k, v = (t.view(2, 40, Hkv, d) for t in buf.split([2 * Hkv * d, Hkv * d, Hkv * d], dim=-1)[1:])
    lens = torch.tensor([40, 13], dtype=torch.int32, device=DEV)
    amax = torch.zeros((2, Hkv), device=DEV)
    ks, vs = torch.ones(Hkv, device=DEV), torch.ones(Hkv, device=DEV)

    def step():
        amax.zero_()
        Q.observe_absmax(k, v, amax, lens)
        Q.scales_from_absmax(amax, ks, vs)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    seen = set()
    for scale in (1.0, 300.0, 2.0 ** -9):
        buf.copy_(_rand(buf.shape, torch.bfloat16, gen) * scale)  # new data behind the captured pointers
        g.replay()
        want = Q.scales_from_absmax_reference(Q.absmax_reference(k, v, lens).cpu())
        assert torch.equal(ks.cpu(), want[0]) and torch.equal(vs.cpu(), want[1])
        seen.add(float(ks[0]))
    assert len(seen) == 3


# ---- 5. the operator ------------------------------------------------------------------------------------------------------------------
def test_fp8_suffix_operator_holds_the_budget_with_calibrated_scales_only():
    from hydragen_amd.flash import flash_attention_seqlen

    q, k, v = (t.to(DEV) for t in cases.make_inputs("mixed_heads"))
    want = cases.attention64(q, k, v)
    amax = _observe(k, v)
    ks, vs = torch.ones(cases.H, device=DEV), torch.ones(cases.H, device=DEV)
    Q.scales_from_absmax(amax, ks, vs)
    assert torch.equal(torch.stack([ks, vs]).cpu(), Q.scales_from_absmax_reference(Q.absmax_reference(k.cpu(), v.cpu())))
    out, _ = flash_attention_seqlen(q, Q.quantize_kv(k, ks), Q.quantize_kv(v, vs), k_scale=ks, v_scale=vs)
    cal = cases.rel_l2(out.double().cpu().numpy(), want)
    one = torch.ones(cases.H, device=DEV)
    out1, _ = flash_attention_seqlen(q, Q.quantize_kv(k, one), Q.quantize_kv(v, one), k_scale=one, v_scale=one)
    unit = cases.rel_l2(out1.double().cpu().numpy(), want)
    print(f"fp8 suffix operator, mixed heads: calibrated whole {cal[0]:.3e} worst head {cal[1]:.3e}; unit {unit[0]:.3e} / {unit[1]:.3e}")
    assert cal[0] <= FP8_REL_L2_BOUND and cal[1] <= FP8_REL_L2_BOUND, cal
    assert unit[0] > FP8_REL_L2_BOUND, unit


# ---- 6. the model shell ------------------------------------------------------------------------------------------------------------------
def _caches(model):
    return [layer.self_attn.kv_cache for layer in model.model.layers]


def _setup(model, B, **kw):
    model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=32, max_shared_batch_sizes=[1, B], max_shared_seq_lengths=[50, 16], **kw)


def _two_magnitudes(model):
    """Make K / V of prompts over token ids < 256 about 64 times smaller than those of ids >= 256, at every layer's input: the
    attention norms pass the odd channels only, and the low ids' embeddings carry 1 / 64 of their size there.  (Scaling whole
    embedding rows would not do it: the RMSNorm in front of the projections undoes that.)"""
    with torch.no_grad():
        model.model.embed_tokens.weight[:256, 1::2] *= 1.0 / 64
        for layer in model.model.layers:
            layer.input_layernorm.weight[::2] = 0.0


def _rescaled_twin(kv_heads):
    """Model A and A' = A with v_proj x 2^-10, o_proj x 2^10, k_proj x 2^-6, q_proj x 2^6, in place: the same network in bf16."""
    a, b = (make_model(torch.bfloat16, head_dim=128, kv_heads=kv_heads, heads=4, seed=3) for _ in range(2))
    with torch.no_grad():
        for layer in b.model.layers:
            at = layer.self_attn
            at.v_proj.weight.mul_(2.0 ** -10)
            at.o_proj.weight.mul_(2.0 ** 10)
            at.k_proj.weight.mul_(2.0 ** -6)
            at.q_proj.weight.mul_(2.0 ** 6)
    return a, b


def _flows(model, prefix, uniq, ov):
    """Two generate() calls with forced tokens: shared prompt + unique prompts, then shared prompt + fan-out.  -> per flow
    (step logits [steps, B, V], scales per layer, unique-cache bytes per layer)."""
    out = []
    B = uniq.shape[0]
    for kw in (dict(input_ids=[prefix, uniq], num_return_sequences=1), dict(input_ids=prefix, num_return_sequences=B)):
        _, logits = model.generate(max_new_tokens=ov.shape[1], temperature=0.0, return_logits=True, token_overrides=ov,
                                   shared_cache_op="wipe", **kw)
        kvs = _caches(model)
        out.append((torch.stack(logits), [(c.k_scale.clone(), c.v_scale.clone()) if c.fp8 else None for c in kvs],
                    [(c.per_completion_k_cache.view(torch.uint8).clone(), c.per_completion_v_cache.view(torch.uint8).clone())
                     if c.fp8 else None for c in kvs]))
        model.empty_shared_cache()
    return out


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_model_power_of_two_equivariance_and_unit_scales_are_worse(kv_heads):
    a, b = _rescaled_twin(kv_heads)
    g = torch.Generator(device=DEV).manual_seed(13)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)  # noqa: E731
    B = 6
    prefix, uniq, ov = rnd(1, 50), rnd(B, 9), rnd(B, 6)
    for m in (a, b):
        _setup(m, B, kv_cache_dtype=FP8, kv_scales="calibrate")
    fa, fb = _flows(a, prefix, uniq, ov), _flows(b, prefix, uniq, ov)
    for (la, sa, ba), (lb, sb, bb) in zip(fa, fb):
        for (ksa, vsa), (ksb, vsb) in zip(sa, sb):
            assert not bool((ksa == 1).all()) or not bool((vsa == 1).all())  # calibrated at all
            assert torch.equal(ksb, ksa * 2.0 ** -6) and torch.equal(vsb, vsa * 2.0 ** -10)
        for (ka, va), (kb, vb) in zip(ba, bb):
            assert torch.equal(ka, kb) and torch.equal(va, vb)  # the same fp8 bytes
        assert torch.equal(la, lb)                               # the same logits, step by step
    # against the 16-bit caches of the same model: calibrated A' is as good as A, unit-scale A' is not (its V flushes to zero)
    _setup(b, B)
    ref_b = _flows(b, prefix, uniq, ov)
    _setup(b, B, kv_cache_dtype=FP8, kv_scales="unit")
    unit_b = _flows(b, prefix, uniq, ov)
    for i, flow in enumerate(("unique prompts", "fan-out")):
        want = ref_b[i][0][1:].double()  # (step 0 is the prefill's logits: no fp8 byte read yet)
        e_cal = float((fb[i][0][1:].double() - want).norm() / want.norm())
        e_unit = float((unit_b[i][0][1:].double() - want).norm() / want.norm())
        print(f"kv_scale model equivariance, {kv_heads} kv heads, {flow}: logits relative L2 against bf16 caches, calibrated "
              f"{e_cal:.3e}, unit {e_unit:.3e}, ratio {e_unit / e_cal:.1f}")
        assert e_unit >= 5 * e_cal
        assert all(bool((k == 1).all()) and bool((v == 1).all()) for k, v in unit_b[i][1])


def _prefill_scales(model, levels_k, levels_v, margin=2.0):
    """The definition on given K / V lists per layer -> [(k_scale, v_scale)] per layer."""
    out = []
    for ks, vs in zip(levels_k, levels_v):
        amax = torch.zeros((2, ks[0].shape[-2]), device=DEV)
        for k, v in zip(ks, vs):
            amax = torch.maximum(amax, Q.absmax_reference(k, v))
        s = Q.scales_from_absmax_reference(amax.cpu(), margin).to(DEV)  # (the definition is its evaluation on the CPU)
        out.append((s[0], s[1]))
    return out


def test_freeze_reset_and_graph_replay():
    eager, graphed = (make_model(torch.bfloat16, head_dim=128, kv_heads=4, heads=4, seed=5) for _ in range(2))
    graphed.graph(True)
    g = torch.Generator(device=DEV).manual_seed(23)
    rnd = lambda *s: torch.randint(1, 256, s, device=DEV, generator=g)  # noqa: E731
    B, n = 6, 8
    p1, p2, ov = rnd(1, 40), torch.randint(256, 512, (1, 40), device=DEV, generator=g), rnd(B, n)  # (one length: one graph key)
    for m in (eager, graphed):
        _two_magnitudes(m)
        _setup(m, B, kv_cache_dtype=FP8, kv_scales="calibrate")
    captured, per_call = None, []
    for prompt in (p2, p1):  # the LARGER prompt first: a maximum that survived the first call would show in the second
        outs = []
        for m in (eager, graphed):
            _, logits = m.generate(input_ids=prompt, num_return_sequences=B, max_new_tokens=n, temperature=0.0, return_logits=True,
                                   token_overrides=ov, shared_cache_op="wipe")
            outs.append(torch.stack(logits))
        assert torch.equal(outs[0], outs[1])  # the graphed decode equals the un-graphed one
        cd = graphed.graphed_model.capture_data
        captured = cd if captured is None else captured
        assert cd is captured, "the second call re-captured the decode graph"
        # this call's scales are the definition on this call's prefill K / V alone: the level "wipe" leaves in the shared cache
        for m in (eager, graphed):
            kvs = _caches(m)
            P = prompt.shape[1]
            want = _prefill_scales(m, [[c.shared_caches[0].k_cache[:P]] for c in kvs], [[c.shared_caches[0].v_cache[:P]] for c in kvs])
            for c, (ks, vs) in zip(kvs, want):
                assert torch.equal(c.k_scale, ks) and torch.equal(c.v_scale, vs)
        per_call.append([(c.k_scale.clone(), c.v_scale.clone()) for c in _caches(eager)])
    for (k_big, v_big), (k_small, v_small) in zip(*per_call):  # the prompts differ in magnitude, and so do their scales
        assert bool((k_small <= k_big).all()) and bool((v_small <= v_big).all())
    assert bool((per_call[1][0][1] < per_call[0][0][1]).all())  # layer 0, V: no attention in between

    # frozen: an append_shared after a generate() observes but does not rescale, and the fork reads the rows with their scales
    model = eager
    model.generate(input_ids=p1, num_return_sequences=B, max_new_tokens=n, temperature=0.0, token_overrides=ov, shared_cache_op="wipe")
    before = [(c.k_scale.clone(), c.v_scale.clone(), c.kv_amax.clone()) for c in _caches(model)]
    levels = model.get_num_used_shared_caches()
    model.append_shared(torch.randint(256, 512, (B, 7), device=DEV, generator=g))
    for c, (ks, vs, am) in zip(_caches(model), before):
        assert torch.equal(c.k_scale, ks) and torch.equal(c.v_scale, vs)
        assert bool((c.kv_amax >= am).all()) and not torch.equal(c.kv_amax, am)  # observed
    model.truncate_shared_caches(levels)
    rows, lens = [5, 0, 3], [n - 1, n - 3, n - 2]
    r = torch.tensor(rows, device=DEV)
    levels_kv = []
    for use_kernel in (True, False):
        assert model.fork(rows, lens, ov[r, : max(lens)], old_batch=B, use_kernel=use_kernel) == levels + 1
        levels_kv.append([(c.shared_caches[levels].k_cache.clone(), c.shared_caches[levels].v_cache.clone()) for c in _caches(model)])
        model.truncate_shared_caches(levels)
    for (ka, va), (kb, vb) in zip(*levels_kv):
        assert torch.equal(ka.view(torch.int16), kb.view(torch.int16)) and torch.equal(va.view(torch.int16), vb.view(torch.int16))
        assert bool((ka != 0).any())

    # reset: the running maxima are zeroed with the last level, reset_kv_scales() restores ones
    model.empty_shared_cache()
    assert all(bool((c.kv_amax == 0).all()) for c in _caches(model))
    assert any(not bool((c.v_scale == 1).all()) for c in _caches(model))
    ptrs = [(c.k_scale.data_ptr(), c.v_scale.data_ptr(), c.kv_amax.data_ptr()) for c in _caches(model)]
    model.reset_kv_scales()
    for c, p in zip(_caches(model), ptrs):
        assert bool((c.k_scale == 1).all()) and bool((c.v_scale == 1).all()) and bool((c.kv_amax == 0).all())
        assert (c.k_scale.data_ptr(), c.v_scale.data_ptr(), c.kv_amax.data_ptr()) == p
    # a "preserve" call that starts from no levels leaves zeroed maxima behind, and calibrated scales
    model.generate(input_ids=[p1, rnd(B, 5)], num_return_sequences=1, max_new_tokens=3, temperature=0.0)
    assert all(bool((c.kv_amax == 0).all()) for c in _caches(model))
    assert any(not bool((c.v_scale == 1).all()) for c in _caches(model))


def test_unique_prefill_and_no_sharing_windows():
    """The window closes at the first write to the unique cache: with unique prompts after the unique prefill observed its own K / V,
    in the no-sharing mode at the copy of the shared prefix (the unique prompts come too late)."""
    model = make_model(torch.bfloat16, head_dim=128, kv_heads=4, heads=4, seed=7)
    g = torch.Generator(device=DEV).manual_seed(29)
    B = 4
    prefix = torch.randint(1, 256, (1, 20), device=DEV, generator=g)
    uniq = torch.randint(256, 512, (B, 6), device=DEV, generator=g)
    _two_magnitudes(model)  # the shared prompt's K / V are small, the unique prompts' large
    model.setup_caches(max_unique_batch_size=B, max_unique_seq_length=48, max_shared_batch_sizes=[1], max_shared_seq_lengths=[20],
                       kv_cache_dtype=FP8, kv_scales="calibrate")
    seen, final = {}, {}

    def record(name):
        def hook(k, v, amax, row_lens=None):
            seen.setdefault(name, []).append((k.clone(), v.clone()))
            return real(k, v, amax, row_lens)
        return hook

    real = Q.observe_absmax
    for name, kw in (("hydragen", {}), ("no_sharing", dict(disable_hydragen=True))):
        Q.observe_absmax = record(name)
        try:
            model.generate(input_ids=[prefix, uniq], num_return_sequences=1, max_new_tokens=3, temperature=0.0, shared_cache_op="wipe", **kw)
        finally:
            Q.observe_absmax = real
        L = len(model.model.layers)
        calls = seen[name]
        assert len(calls) == 2 * L  # one launch per layer and prefill: shared, then unique -- none from the decode steps
        for i, c in enumerate(_caches(model)):
            used = [calls[i], calls[L + i]] if name == "hydragen" else [calls[i]]
            amax = torch.zeros((2, 4), device=DEV)
            for k, v in used:
                amax = torch.maximum(amax, Q.absmax_reference(k, v))
            want = Q.scales_from_absmax_reference(amax.cpu()).to(DEV)
            assert torch.equal(c.k_scale, want[0]) and torch.equal(c.v_scale, want[1]), (name, i)
        final[name] = _caches(model)[0].v_scale.clone()
        model.empty_shared_cache()
    assert bool((final["no_sharing"] < final["hydragen"]).all())  # the unique prompts came too late for the no-sharing scales


def test_default_is_untouched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("kv_scales='unit' must not observe or rescale")

    monkeypatch.setattr(Q, "observe_absmax", boom)
    monkeypatch.setattr(Q, "scales_from_absmax", boom)
    model = make_model(torch.bfloat16, head_dim=128, kv_heads=4, heads=4)
    g = torch.Generator(device=DEV).manual_seed(31)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)  # noqa: E731
    B, n = 6, 5
    prefix, uniq, ov = rnd(1, 30), rnd(B, 7), rnd(B, n)
    for kw in (dict(kv_cache_dtype=FP8), dict(kv_cache_dtype=FP8, kv_scales="unit")):
        _setup(model, B, **kw)
        assert all(c.kv_amax is None for c in _caches(model))
        model.generate(input_ids=prefix, num_return_sequences=B, max_new_tokens=n, temperature=0.0, token_overrides=ov, shared_cache_op="wipe")
        rows = [4, 1, 2]
        model.fork(rows, [n - 1] * 3, ov[torch.tensor(rows, device=DEV), : n - 1], old_batch=B)
        model.empty_shared_cache()
        model.generate(input_ids=[prefix, uniq], num_return_sequences=1, max_new_tokens=n, temperature=0.0)
        model.score([prefix, uniq], [3] * B)
        model.reset_kv_scales()
        assert all(bool((c.k_scale == 1).all()) and bool((c.v_scale == 1).all()) for c in _caches(model))
    with pytest.raises(ValueError, match="kv_scales"):
        _setup(model, B, kv_scales="calibrate")
    with pytest.raises(ValueError, match="kv_scales"):
        _setup(model, B, kv_cache_dtype=FP8, kv_scales="per-token")
    _setup(model, B)  # a 16-bit cache with the default: as ever
    model.generate(input_ids=prefix, num_return_sequences=B, max_new_tokens=2, temperature=0.0)
