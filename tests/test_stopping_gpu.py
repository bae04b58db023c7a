"""-m gpu: stop conditions decided on the device.  hyd_stop_update against the two definitions of hydragen_amd/stopping.py, the
contract of the RoPE + append kernel that retiring a finished row relies on, and generate() with EOS lists / stop sequences against
the same generation without them, cut by stopping.truncate_reference."""
import pytest
import torch

from hydragen_amd import layer_ops, stopping
from tests import stop_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the kernel against the definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 1024])
@pytest.mark.parametrize("retire", [True, False])
@pytest.mark.parametrize("shared", [True, False])
def test_kernel_equals_the_definition_step_by_step(rows, retire, shared):
    for name in sorted(stop_cases.CASES):
        for include_stop, pad in ((False, stop_cases.SAFE), (True, 1), (False, 1)):
            spec = stop_cases.spec(name, include_stop, pad)
            tok = stop_cases.tokens(name, rows, seed=rows)
            steps = tok.shape[1]
            w_out, w_len, w_reason, w_index = stopping.truncate_reference(tok, spec)
            step, _, _ = stopping.finish_steps(tok, spec)
            running = torch.arange(steps)[None, :] < step[:, None]
            start = torch.arange(rows) * 3 + 100
            shared_len = (torch.arange(rows) % 7 + 50) if shared else None
            gone = ((shared_len if shared else torch.zeros(rows, dtype=torch.long)) - 1)[:, None].expand(rows, steps)
            adv = start[:, None] + torch.arange(steps)[None, :]
            w_feed = torch.where(running, tok, torch.full_like(tok, pad))
            w_pos = torch.where(running | (not retire), adv, gone)

            state = stopping.new_state(rows, steps, spec, DEV)
            d_tok, d_start = tok.to(DEV), start.to(DEV)
            d_shared = shared_len.to(DEV) if shared else None
            table = spec.stop_table(DEV)[0]
            feeds, poss = [], []
            for t in range(steps):
                f, p = layer_ops.stop_update(d_tok[:, t : t + 1], t, spec, *state, d_start, d_shared, retire, table)
                feeds.append(f)
                poss.append(p)
            out, length, reason, index, live = (x.cpu() for x in state)
            what = (name, include_stop, pad)
            assert torch.equal(out, w_out), what
            assert torch.equal(length, w_len) and torch.equal(reason, w_reason) and torch.equal(index, w_index), what
            assert torch.equal(live, stopping.live_reference(tok, spec)), what
            assert torch.equal(torch.stack(feeds, 1).cpu(), w_feed), what
            assert torch.equal(torch.stack(poss, 1).cpu(), w_pos), what


def test_kernel_on_a_strided_output_matrix_and_without_conditions():
    """out is addressed through out_stride (a column slice of a wider matrix); with no EOS id and no stop nothing finishes."""
    rows, steps = 70, 9
    tok = stop_cases.tokens("overlapping", rows, steps=steps).to(DEV)
    start = torch.zeros(rows, dtype=torch.int64, device=DEV)
    for spec in (stop_cases.spec("overlapping", False), stopping.check_stop(None, None, 3)):
        wide = torch.full((rows, steps + 5), -7, dtype=torch.int64, device=DEV)
        _, length, reason, index, live = stopping.new_state(rows, steps, spec, DEV)
        for t in range(steps):
            layer_ops.stop_update(tok[:, t], t, spec, wide[:, :steps], length, reason, index, live, start)
        want = stopping.truncate_reference(tok.cpu(), spec)
        assert torch.equal(wide[:, :steps].cpu(), want[0]) and bool((wide[:, steps:] == -7).all())
        assert torch.equal(length.cpu(), want[1]) and torch.equal(reason.cpu(), want[2])


# ---- the contract retirement relies on ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_rope_append_skips_a_row_fed_the_position_below_its_cache(fp8):
    """A row fed position shared_len - 1 (cache index -1) leaves its cache bytes untouched and gets seq_lens == 0, while its
    neighbours append normally (documented at hyd_rope_append_decode; hyd_stop_update's retired rows depend on it)."""
    from hydragen_amd.fused_decode import rope_append_decode
    from hydragen_amd.kv_quant import FP8_DTYPE
    from hydragen_amd.llama import RotaryTable

    B, S, H, D = 12, 24, 4, 128
    g = torch.Generator(device=DEV).manual_seed(2)
    q, k, v = (torch.randn(B, 1, H, D, device=DEV, dtype=torch.bfloat16, generator=g) for _ in range(3))
    rot = RotaryTable(D, 256, 10000.0, device=DEV)
    retired = torch.tensor([0, 3, 4, 11], device=DEV)
    for with_shared in (True, False):
        shared = (torch.arange(B, device=DEV) % 5 + 20) if with_shared else None
        base = shared if with_shared else torch.zeros(B, dtype=torch.long, device=DEV)
        idx = torch.arange(B, device=DEV) % 7 + 1
        pos = base + idx
        pos[retired] = base[retired] - 1
        fill = torch.randint(1, 120, (2, B, S, H, D), device=DEV, dtype=torch.uint8, generator=g)  # (finite in either format)
        if fp8:
            kc, vc = fill[0].clone().view(FP8_DTYPE), fill[1].clone().view(FP8_DTYPE)
            sc = dict(k_scale=torch.full((H,), 0.5, device=DEV), v_scale=torch.full((H,), 2.0, device=DEV))
        else:
            kc, vc = fill[0].to(torch.bfloat16), fill[1].to(torch.bfloat16)
            sc = {}
        k0, v0 = kc.clone(), vc.clone()
        _, sl = rope_append_decode(q, k, v, rot.cos_cached, rot.sin_cached, pos[:, None].contiguous(), shared, kc, vc, **sc)
        torch.cuda.synchronize()
        want_sl = (idx + 1).int()
        want_sl[retired] = 0
        assert torch.equal(sl, want_sl)
        b8 = lambda x: x.view(torch.uint8) if fp8 else x.view(torch.int16)  # noqa: E731
        for c, c0 in ((kc, k0), (vc, v0)):
            assert torch.equal(b8(c)[retired], b8(c0)[retired]), "a retired row's cache changed"
            changed = (b8(c) != b8(c0)).flatten(2).any(-1)  # [B, S]
            want = torch.zeros_like(changed)
            live = torch.ones(B, dtype=torch.bool, device=DEV)
            live[retired] = False
            want[torch.arange(B, device=DEV)[live], idx[live]] = True
            assert torch.equal(changed, want), "the neighbours append at their own index and nowhere else"


# ---- generate() -----------------------------------------------------------------------------------------------------------------
NEW = 12


def _model(kv_heads=2, head_dim=128):
    from tests.test_model_gpu import make_model

    return make_model(torch.bfloat16, head_dim=head_dim, kv_heads=kv_heads)


def _prompts(layout):
    g = torch.Generator(device=DEV).manual_seed(11)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)  # noqa: E731
    if layout == "fan-out":
        return dict(input_ids=[rnd(1, 40)], num_return_sequences=16), 16
    ids = [rnd(1, 33), rnd(16, 10)]
    lens = [torch.tensor([33], device=DEV), torch.tensor([10, 7, 3, 10, 9, 1, 5, 10, 2, 10, 6, 4, 8, 10, 10, 3], device=DEV)]
    return dict(input_ids=ids, seq_lens=lens, num_return_sequences=1), 16


def _setup(model, graph, kv=None, room=NEW):
    model.graph(graph)
    model.setup_caches(max_unique_batch_size=16, max_unique_seq_length=16 + room, max_shared_batch_sizes=[1, 16],
                       max_shared_seq_lengths=[40, 10], kv_cache_dtype=kv)


def _gen(model, prompts, seed, temperature, **kw):
    torch.manual_seed(seed)
    return model.generate(max_new_tokens=kw.pop("max_new_tokens", NEW), temperature=temperature, **prompts, **kw)


def _pick(R, strict=True):
    """EOS ids and stop sequences taken out of the free-running tokens R [B, N] (CPU), searched so that every finish reason occurs,
    some row finishes in the first half, some in the second, and one never.  strict False (greedy decoding: the rows of a fan-out
    are all the same, and a random-weight model may loop on one token): the best choice the tokens allow, where at least one
    row finishes."""
    B, N = R.shape
    g = torch.Generator().manual_seed(0)
    ri = lambda n: int(torch.randint(0, n, (1,), generator=g))  # noqa: E731
    best = None
    for _ in range(2000):
        r = [ri(B) for _ in range(4)]
        eos = [int(R[r[0], ri(N // 2)]), int(R[r[1], N // 2 + ri(N - N // 2)])]
        c1, c2 = ri(N // 2 - 1), N // 2 + ri(N - N // 2 - 3)
        stops = [R[r[2], c1 : c1 + 2].tolist(), R[r[3], c2 : c2 + 3].tolist()]
        if len(set(eos)) < 2:
            continue
        spec = stopping.check_stop(eos, stops, 0, False, 512)
        _, length, reason, _ = stopping.truncate_reference(R, spec)
        fin = reason != 0
        score = len(set(reason.tolist())) + bool((length[fin] < N // 2).any()) + bool((length[fin] > N // 2).any())
        if score == 5:
            return eos, stops
        if bool(fin.any()) and (best is None or score > best[0]):
            best = (score, eos, stops)
    assert not strict and best is not None, "no choice of EOS ids / stops exercises every finish reason on these tokens"
    return best[1], best[2]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("layout, temperature", [("fan-out", 0.8), ("fan-out", 0.0), ("shared+unique", 0.0), ("shared+unique", 0.8)])
def test_generate_with_stops_is_the_free_run_cut_by_the_definition(graph, layout, temperature, kv=None, kv_heads=2):
    model = _model(kv_heads)
    _setup(model, graph, kv)
    prompts, B = _prompts(layout)
    R = _gen(model, prompts, 3, temperature)
    assert R.shape == (B, NEW)
    Rc = R.cpu()
    eos, stops = _pick(Rc, strict=temperature > 0)
    # what the choice covers: with sampling every finish reason, an early and a late finish and a row that never finishes
    # (_pick asserts it); greedy rows may be all alike (a fan-out's are), and there at least one row finishes
    covered = stopping.truncate_reference(Rc, stopping.check_stop(eos, stops, 0, False, 512))[2]
    assert (covered != 0).any() and (temperature == 0 or set(covered.tolist()) == {0, 1, 2})
    model.stop_poll_steps = 4
    for include_stop in (False, True):
        spec = stopping.check_stop(eos, stops, 0, include_stop, 512)
        w_out, w_len, w_reason, w_index = stopping.truncate_reference(Rc, spec)
        width = int(w_len.max())
        for retire in (None, False):
            model.stop_retire = retire
            out, fin = _gen(model, prompts, 3, temperature, eos_token_id=eos, stop=stops, pad_token_id=0, include_stop=include_stop,
                            return_finish=True)
            what = (include_stop, retire, eos, stops)
            assert isinstance(fin, stopping.Finish) and fin.lengths.dtype == torch.int32 and fin.lengths.shape == (B,)
            assert torch.equal(out.cpu(), w_out[:, :width]), what
            assert torch.equal(fin.lengths.cpu(), w_len) and torch.equal(fin.reasons.cpu(), w_reason), what
            assert torch.equal(fin.stop_index.cpu(), w_index), what
    # the free run is still what it was: retiring rows left nothing behind in the caches or the graph
    model.stop_retire = None
    assert torch.equal(_gen(model, prompts, 3, temperature), R)


def test_generate_with_stops_on_fp8_unique_caches():
    from hydragen_amd.kv_quant import FP8_DTYPE

    test_generate_with_stops_is_the_free_run_cut_by_the_definition(True, "shared+unique", 0.8, kv=FP8_DTYPE, kv_heads=4)
    test_generate_with_stops_is_the_free_run_cut_by_the_definition(False, "fan-out", 0.8, kv=FP8_DTYPE, kv_heads=4)


def test_generate_with_stops_torch_preamble_and_no_sharing_baseline():
    """retire is off without the fused preamble (the torch scatter would index -1) and forcing it on is refused; the no-sharing
    baseline retires at position -1 (its cache index is the position itself)."""
    model = _model()
    _setup(model, False, room=64)  # (the no-sharing baseline copies the 40-token prompt into every unique cache)
    prompts, B = _prompts("fan-out")
    R = _gen(model, prompts, 5, 0.8).cpu()
    eos, stops = _pick(R)
    spec = stopping.check_stop(eos, stops, 0, False, 512)
    kw = dict(eos_token_id=eos, stop=stops, pad_token_id=0, return_finish=True)
    for layer in model.model.layers:
        layer.self_attn.use_fused_decode = False
    Rt = _gen(model, prompts, 5, 0.8).cpu()
    wt = stopping.truncate_reference(Rt, spec)
    out, fin = _gen(model, prompts, 5, 0.8, **kw)
    assert torch.equal(out.cpu(), wt[0][:, : int(wt[1].max())]) and torch.equal(fin.lengths.cpu(), wt[1])
    model.stop_retire = True
    with pytest.raises(ValueError, match="fused decode preamble"):
        _gen(model, prompts, 5, 0.8, **kw)
    model.stop_retire = None
    for layer in model.model.layers:
        layer.self_attn.use_fused_decode = True
    Rn = _gen(model, prompts, 5, 0.8, disable_hydragen=True).cpu()
    wn = stopping.truncate_reference(Rn, spec)
    out, fin = _gen(model, prompts, 5, 0.8, disable_hydragen=True, **kw)
    assert torch.equal(out.cpu(), wn[0][:, : int(wn[1].max())]) and torch.equal(fin.lengths.cpu(), wn[1])
    assert torch.equal(fin.reasons.cpu(), wn[2])


@pytest.mark.parametrize("graph", [False, True])
def test_logprob_and_top_logprob_masks(graph):
    model = _model()
    _setup(model, graph)
    prompts, B = _prompts("shared+unique")
    R, lp, tid, tlp = _gen(model, prompts, 7, 0.8, return_logprobs=True, top_logprobs=3)
    eos, stops = _pick(R.cpu())
    spec = stopping.check_stop(eos, stops, 0, False, 512)
    _, w_len, _, _ = stopping.truncate_reference(R.cpu(), spec)
    width = int(w_len.max())
    out, lp2, tid2, tlp2, fin = _gen(model, prompts, 7, 0.8, return_logprobs=True, top_logprobs=3, eos_token_id=eos, stop=stops,
                                     pad_token_id=0, return_finish=True)
    assert torch.equal(fin.lengths.cpu(), w_len)
    inside = (torch.arange(width)[None, :] < w_len[:, None]).to(DEV)
    assert bool((~inside).any()) and bool(inside.any())
    assert lp2.shape == (B, width) and tid2.shape == (B, width, 3) and tlp2.shape == (B, width, 3)
    assert torch.equal(lp2[inside], lp[:, :width][inside]) and bool((lp2[~inside] == 0.0).all())
    assert torch.equal(tid2[inside], tid[:, :width][inside]) and bool((tid2[~inside] == -1).all())
    assert torch.equal(tlp2[inside], tlp[:, :width][inside]) and bool((tlp2[~inside] == float("-inf")).all())
    # return_logits: one entry per returned column
    out3, logits = _gen(model, prompts, 7, 0.8, return_logits=True, eos_token_id=eos, stop=stops, pad_token_id=0)
    assert torch.equal(out3, out) and len(logits) == width


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("poll", [8, 3])
def test_early_exit_is_noticed_within_one_polling_period(graph, poll):
    model = _model()
    _setup(model, graph, room=64)
    prompts, B = _prompts("shared+unique")
    big = 64
    R = _gen(model, prompts, 9, 0.8, max_new_tokens=big)
    k = 5
    eos = sorted(set(R[:, k - 1].tolist()))  # every row holds one of these at step k - 1 at the latest
    assert len(eos) <= 16
    forwards = []
    hook = model.register_forward_hook(lambda m, a, o: forwards.append(m.mode))
    model.stop_poll_steps = poll
    try:
        out, fin = _gen(model, prompts, 9, 0.8, max_new_tokens=big, eos_token_id=eos, return_finish=True)
    finally:
        hook.remove()
    decode = sum(m == "decode" for m in forwards)
    assert out.shape[1] <= k and int(fin.lengths.max()) == out.shape[1] and bool((fin.reasons == 1).all())
    assert decode <= k + poll, (decode, k, poll)
    w = stopping.truncate_reference(R.cpu(), stopping.check_stop(eos, None, None, False, 512))
    assert torch.equal(out.cpu(), w[0][:, : out.shape[1]]) and torch.equal(fin.lengths.cpu(), w[1])


def test_penalties_keep_working_with_stops():
    model = _model()
    _setup(model, True)
    prompts, B = _prompts("fan-out")
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1)
    R = _gen(model, prompts, 13, 0.8, **pen).cpu()
    eos, stops = _pick(R)
    spec = stopping.check_stop(eos, stops, 0, False, 512)
    w = stopping.truncate_reference(R, spec)
    out, fin = _gen(model, prompts, 13, 0.8, eos_token_id=eos, stop=stops, pad_token_id=0, return_finish=True, **pen)
    assert torch.equal(out.cpu(), w[0][:, : int(w[1].max())]) and torch.equal(fin.lengths.cpu(), w[1])


def test_single_int_eos_keeps_its_path(monkeypatch):
    """generate(eos_token_id=<int>) alone never reaches hyd_stop_update and returns what it returned before."""
    model = _model()
    _setup(model, True)
    prompts, B = _prompts("shared+unique")
    R = _gen(model, prompts, 17, 0.8)
    eos = int(R[2, 4])
    saved = _gen(model, prompts, 17, 0.8, eos_token_id=eos)
    def boom(*a, **k):
        raise AssertionError("hyd_stop_update reached from the default path")
    monkeypatch.setattr(layer_ops, "stop_update", boom)
    again = _gen(model, prompts, 17, 0.8, eos_token_id=eos)
    assert torch.equal(saved, again) and torch.equal(saved, R[:, : saved.shape[1]])
    with pytest.raises(AssertionError, match="default path"):
        _gen(model, prompts, 17, 0.8, eos_token_id=[eos])
