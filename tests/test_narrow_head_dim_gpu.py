"""-m gpu: narrow unique K/V caches -- head dims 80 / 96 / 192 ... whose per-sequence cache keeps rows of the TRUE width d and is
read as it is by the narrow form of the token-row suffix kernel (csrc/suffix_rows.h, hyd_suffix_params.kv_dim), while q, the
shared levels, the partials and the output run at the kernels' D = 64 / 128 / 256 with zero pad columns.

Every result is held to the float64 oracle (which knows nothing of any padding) with the suite's usual bounds, and -- the kernel's
contract -- to BIT equality with the zero-padding route spelled out by hand (pad_head_dim on q, k and v, the D-wide kernel under
the true head dim's scale, the slice), wherever that route runs the same kernels."""
import numpy as np
import pytest
import torch

from oracle import hydragen_oracle as O
from tests import glue_ref as R
from tests.cases import _round, make_case
from tests.gpu_util import TORCH_DT, assert_close, case_to_device, dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = [0, 1, 7, 8, 9, 16, 17, 39, 40]


def _rand(rng, shape, dt):
    return _round(rng.standard_normal(shape, dtype=np.float32), dt)


def _padded_route(q, k, v, sl, d):
    """What the operators did before (and still do for shapes without a narrow kernel): three pad copies, the D-wide call, a slice."""
    from hydragen_amd import flash as F

    D = F.padded_head_dim(d)
    with F.true_head_dim_scale(d):
        out, lse = F.flash_attention_seqlen(F.pad_head_dim(q, D), F.pad_head_dim(k, D), F.pad_head_dim(v, D), sl)
    return out[..., :d].contiguous(), lse


def _nan_padded_view(t, D):
    """t as the [..., :d] view of a D-wide buffer whose pad columns are NaN: head stride D, and a read past column d poisons the row."""
    wide = torch.full(t.shape[:-1] + (D,), float("nan"), dtype=t.dtype, device=t.device)
    wide[..., : t.shape[-1]] = t
    return wide[..., : t.shape[-1]]


# d = 96: one / two / three waves per sequence and a second blockIdx.y (Hkv = 20); 16 rows: no token split (TS = 1), 40 rows with
# Hkv = 4: two waves share a sequence (TS = 2); d = 48 runs the D = 64 kernel, 160 / 192 the D = 256 one
SHAPES = [(96, 4, 40), (96, 8, 40), (96, 12, 40), (96, 20, 40), (96, 4, 16), (80, 8, 40), (112, 8, 40), (48, 8, 40), (48, 16, 40),
          (160, 2, 40), (160, 6, 40), (192, 2, 40), (192, 6, 40)]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("d,Hkv,rows", SHAPES)
def test_suffix_pass_on_narrow_caches(dt, d, Hkv, rows):
    from hydragen_amd import flash as F

    rng = np.random.default_rng(1000 * d + 10 * Hkv + rows)
    lens = np.minimum(np.asarray(LENS, dtype=np.int32), rows)
    B = len(lens)
    q, k, v = _rand(rng, (B, 1, Hkv, d), dt), _rand(rng, (B, rows, Hkv, d), dt), _rand(rng, (B, rows, Hkv, d), dt)
    want, wlse = O.flash_attention_seqlen(q, k, v, lens)
    tq, tk, tv = dev(q, dt), dev(k, dt), dev(v, dt)
    assert F.narrow_kv_native(tq, tk, tv)
    D = F.padded_head_dim(d)
    live = lens > 0  # (an empty sequence has no defined output; its LSE is -inf in every route)
    reverse = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=DEV)
    for sl in (dev(lens), dev(lens.astype(np.int64))):
        for order in (None, reverse):
            what = f"d={d} Hkv={Hkv} rows={rows} {dt} lens={sl.dtype} order={'reversed' if order is not None else None}"
            with F.seq_order(order):
                out, lse = F.flash_attention_seqlen(tq, tk, tv, sl)
                pout, plse = _padded_route(tq, tk, tv, sl, d)
                vout, vlse = F.flash_attention_seqlen(tq, _nan_padded_view(tk, D), _nan_padded_view(tv, D), sl)
            assert out.shape == (B, 1, Hkv, d) and out.is_contiguous()
            assert_close(out.float().cpu().numpy()[live], want[live], dt, what)                      # (a) the oracle
            assert np.abs(lse.cpu().numpy()[live] - wlse[live]).max() < 2e-3, what
            assert torch.isinf(lse[torch.from_numpy(~live).to(DEV)]).all(), what
            assert torch.equal(out, pout) and torch.equal(lse, plse), "padded route: " + what       # (b) bit for bit
            assert torch.equal(out, vout) and torch.equal(lse, vlse), "NaN-padded views: " + what   # (c) nothing read past d


def test_suffix_pass_four_waves_share_a_sequence():
    """More than 2048 sequences with one wave's worth of heads: the token split by 4 (TS = 4) through LDS."""
    from hydragen_amd import flash as F

    dt, B, Hkv, d, rows = "bf16", 2052, 4, 96, 32
    rng = np.random.default_rng(4)
    lens = rng.integers(0, rows + 1, B).astype(np.int32)
    lens[:4] = [0, 1, rows, rows - 1]
    q, k, v = _rand(rng, (B, 1, Hkv, d), dt), _rand(rng, (B, rows, Hkv, d), dt), _rand(rng, (B, rows, Hkv, d), dt)
    want, wlse = O.flash_attention_seqlen(q, k, v, lens)
    tq, tk, tv, sl = dev(q, dt), dev(k, dt), dev(v, dt), dev(lens)
    out, lse = F.flash_attention_seqlen(tq, tk, tv, sl)
    pout, plse = _padded_route(tq, tk, tv, sl, d)
    live = lens > 0
    assert_close(out.float().cpu().numpy()[live], want[live], dt, "TS = 4")
    assert np.abs(lse.cpu().numpy()[live] - wlse[live]).max() < 2e-3
    assert torch.equal(out, pout) and torch.equal(lse, plse)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rows", [80, 1040])
def test_suffix_pass_where_the_wide_rule_picks_the_other_kernel(dt, rows):
    """Few units with 64 or more rows, and more than 1024 rows: D-wide calls of these shapes go to the one-unit-per-wave kernel,
    narrow ones stay on the token-row kernel (the only one with a narrow form).  Oracle only."""
    from hydragen_amd import flash as F

    d, Hkv, B = 96, 8, 3
    rng = np.random.default_rng(rows)
    lens = np.asarray([rows, 1, rows - 17], dtype=np.int32)
    q, k, v = _rand(rng, (B, 1, Hkv, d), dt), _rand(rng, (B, rows, Hkv, d), dt), _rand(rng, (B, rows, Hkv, d), dt)
    want, wlse = O.flash_attention_seqlen(q, k, v, lens)
    out, lse = F.flash_attention_seqlen(dev(q, dt), dev(k, dt), dev(v, dt), dev(lens))
    assert_close(out.float().cpu().numpy(), want, dt, f"rows={rows}")
    assert np.abs(lse.cpu().numpy() - wlse).max() < 2e-3


def test_no_copy_of_the_unique_cache():
    """k and v of 201 MB each: the call allocates q-sized tensors only.  (The zero-padding route allocates 268 MB copies of both.)"""
    from hydragen_amd import flash as F

    B, rows, H, d = 64, 512, 32, 96
    g = torch.Generator(device=DEV).manual_seed(0)
    k = torch.randn(B, rows, H, d, device=DEV, dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, rows, H, d, device=DEV, dtype=torch.bfloat16, generator=g)
    q = torch.randn(B, 1, H, d, device=DEV, dtype=torch.bfloat16, generator=g)
    sl = torch.full((B,), rows, dtype=torch.int32, device=DEV)
    assert F.narrow_kv_native(q, k, v)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, lse = F.flash_attention_seqlen(q, k, v, sl)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < k.numel() * k.element_size(), f"{grown} bytes allocated during the call"
    assert out.shape == q.shape and torch.isfinite(out).all() and torch.isfinite(lse).all()


def _oracle(case):
    return O.hydragen_attention(case["q"], case["k"], case["v"], case["shared_ks"], case["shared_vs"], case["shared_cu_seq_lens"],
                                case["shared_max_seq_lens"], case["use_varlens"], case["seq_lens"])


# [[64], [4] * 4]: the smallest; [[200], [6] * 8]: above api_attn.hip's one-launch rule (8 * 8 * 206 keys > 8192); a ragged level; four
# levels (the kernel prefetches two partials, the others are fetched behind the key loop); one group of 4096 keys for 8 sequences:
# split-KV, stacked fp32 slices
OPERATOR_SIZES = [
    [[64], [4, 4, 4, 4]],
    [[200], [6] * 8],
    [[48], [9, 10], [5, 2, 3, 4]],
    [[40], [12, 12], [6] * 4, [5] * 8, [3, 1, 2, 4, 5, 6, 7, 8]],
    [[4096], [8] * 8],
]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("d", [80, 96, 192])
@pytest.mark.parametrize("si", range(len(OPERATOR_SIZES)))
def test_whole_operator_on_narrow_caches(dt, d, si):
    from hydragen_amd import flash as F
    from hydragen_amd.attention import hydragen_attention, hydragen_attention_nopad

    sizes, H = OPERATOR_SIZES[si], 8
    case = make_case(sizes=sizes, qheads=H, kvheads=H, dim=d, dtype=dt, seed=100 * d + si, force_seq_lens=True)
    args = case_to_device(case)
    assert F.narrow_kv_native(args["q"], args["k"], args["v"])
    what = f"d={d} {dt} sizes #{si}"
    out = hydragen_attention(**args)
    assert tuple(out.shape) == case["q"].shape and out.is_contiguous()
    assert_close(out.float().cpu().numpy(), _oracle(case), dt, what)
    D = F.padded_head_dim(d)
    pad = lambda t: F.pad_head_dim(t, D)
    # the hand-padded call, where it runs as the prefix + suffix pair too (one level and few keys: ONE launch, other roundings)
    keys = len(sizes[-1]) * H * (sizes[0][0] + max(sizes[-1]))
    if len(sizes) != 2 or keys > 8192:
        with F.true_head_dim_scale(d):
            pout = hydragen_attention(pad(args["q"]), pad(args["k"]), pad(args["v"]), [pad(x) for x in args["shared_ks"]],
                                      [pad(x) for x in args["shared_vs"]], args["shared_cu_seq_lens"], args["shared_max_seq_lens"],
                                      args["use_varlens"], args["seq_lens"])
        assert torch.equal(out, pout[..., :d]), "padded route: " + what
    # pre-padded form: D-wide q and levels in (zero pad columns), nothing copied, D-wide out with pad columns exactly 0
    wide = dict(args, q=pad(args["q"]), shared_ks=[pad(x) for x in args["shared_ks"]], shared_vs=[pad(x) for x in args["shared_vs"]])
    wout = hydragen_attention(**wide)
    assert wout.shape[-1] == D and torch.equal(wout[..., :d], out), "pre-padded form: " + what
    assert not wout[..., d:].view(torch.int16).any(), "pad columns of the output: " + what
    if not any(case["use_varlens"]):
        nout = hydragen_attention_nopad(args["q"], args["k"], args["v"], args["shared_ks"], args["shared_vs"], args["seq_lens"])
        assert torch.equal(nout, out), "nopad: " + what


def _positions(B, L, max_pos=R.EXACT_MAX_POS):
    """Cache indices that cover 0 and L - 1 at positions spread over the table; the last row sits at shared_len - 1: it retires."""
    idx = (np.arange(B) * 3 + (L - 1)) % L
    idx[-2] = 0
    shared = (np.arange(B) * 5 + 2) % (max_pos - L + 1)
    idx[-1] = -1
    return idx + shared, shared


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d", [80, 96, 192])
@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2)])
@pytest.mark.parametrize("wide_cache", [False, True])
def test_preamble_addresses_narrow_rows_exactly(dtype, d, Hq, Hkv, wide_cache):
    """Exact arithmetic (glue_ref: tables of {0, +-1, +-1/2}, inputs on a 2^-3 grid), sentinel-filled buffers compared WHOLE: q_out
    is D wide with the rotated row in front and exact zeros behind, the caches change at [b, idx, :, :d] and nowhere else -- with
    rows of d elements, and as the [..., :d] view of D-wide buffers (head stride D) --, V arrives bit for bit, and the row at
    shared_len - 1 writes nothing and reports length 0."""
    from hydragen_amd.flash import padded_head_dim
    from hydragen_amd.fused_decode import rope_append_decode

    B, L, D = 7, 11, padded_head_dim(d)
    pos, shared = _positions(B, L)
    c = R.make_exact_rope_case(dtype, d, Hq, Hkv, B, pos, shared, L)
    assert not bool(c["written"][-1]) and int(c["seq_lens"][-1]) == 0 and bool(c["written"][:-1].all())
    w = D if wide_cache else d
    hk, hv = R.sentinel16((B + 1, L, Hkv, w), dtype, 0), R.sentinel16((B + 1, L, Hkv, w), dtype, 1)
    dk, dv = hk.to(DEV), hv.to(DEV)
    qo, sl = rope_append_decode(*(c[n].to(DEV)[:, None] for n in ("q", "k", "v")), c["cos"].to(DEV), c["sin"].to(DEV),
                                c["pos"].to(DEV)[:, None], c["shared"].to(DEV), dk[..., :d], dv[..., :d])
    rows = torch.nonzero(c["written"]).flatten()
    hk[rows, c["idx"][rows], :, :d] = c["want_k"][rows]
    hv[rows, c["idx"][rows], :, :d] = c["v"][rows]
    assert qo.shape == (B, 1, Hq, D) and torch.equal(sl.cpu(), c["seq_lens"])
    assert torch.equal(R.bits(qo[:, 0, :, :d].cpu()), R.bits(c["want_q"])), "rotated q"
    assert not R.bits(qo[..., d:].cpu()).any(), "q_out's pad columns are exact zeros"
    assert torch.equal(R.bits(dk.cpu()), R.bits(hk)), "K cache (whole buffer)"
    assert torch.equal(R.bits(dv.cpu()), R.bits(hv)), "V cache (whole buffer)"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("d", [80, 96, 192])
@pytest.mark.parametrize("Hq,Hkv", [(8, 8), (8, 2)])
def test_preamble_rounds_once(dtype, d, Hq, Hkv):
    """Real tables, positions over the whole table: q_out and the appended K within glue_ref.rope_bound of float64 arithmetic on the
    kernel's own fp32 table values -- the bound tests/test_decode_glue_gpu.py holds the D-wide kernel to --, V bit for bit."""
    from hydragen_amd.fused_decode import rope_append_decode
    from hydragen_amd.llama import RotaryTable

    max_pos, B, L = 4096, 96, 8
    rot = RotaryTable(d, max_pos, 1e4, device=DEV)
    cos, sin = rot.cos_cached.cpu().numpy(), rot.sin_cached.cpu().numpy()
    for i, scale in enumerate((1.0, 2.0 ** -10, 100.0)):
        g = torch.Generator().manual_seed(1000 * d + 10 * Hkv + i)
        q, k, v = ((torch.randn(B, 1, H, d, generator=g) * scale).to(dtype) for H in (Hq, Hkv, Hkv))
        pos = torch.randint(0, max_pos, (B,), generator=g)
        pos[:2] = torch.tensor([0, max_pos - 1])
        idx = torch.minimum(torch.arange(B) % L, pos)
        kc, vc = R.sentinel16((B, L, Hkv, d), dtype).to(DEV), R.sentinel16((B, L, Hkv, d), dtype, 1).to(DEV)
        qo, sl = rope_append_decode(q.to(DEV), k.to(DEV), v.to(DEV), rot.cos_cached, rot.sin_cached, pos[:, None].to(DEV),
                                    (pos - idx).to(DEV), kc, vc)
        assert torch.equal(sl.cpu(), (idx + 1).int())
        bi = torch.arange(B)
        assert torch.equal(R.bits(vc.cpu()[bi, idx]), R.bits(v[:, 0]))
        assert not R.bits(qo[..., d:].cpu()).any()
        for name, got, x in (("q", qo[:, 0, :, :d].cpu(), q[:, 0]), ("k", kc.cpu()[bi, idx], k[:, 0])):
            x64 = x.double().numpy()
            want = R.rope_ref64(x64, cos[pos.numpy()], sin[pos.numpy()])
            ratio = np.abs(got.double().numpy() - want) / R.rope_bound(want, x64, dtype)
            assert ratio.max() <= 1.0, (name, scale, float(ratio.max()))


class _PadRecorder:
    """flash.pad_head_dim wrapped: the shapes it was asked to copy."""

    def __enter__(self):
        from hydragen_amd import flash as F

        self.F, self.real, self.shapes = F, F.pad_head_dim, []

        def recording(t, dp):
            self.shapes.append(tuple(t.shape))
            return self.real(t, dp)

        F.pad_head_dim = recording
        return self

    def __exit__(self, *exc):
        self.F.pad_head_dim = self.real


def _check_model(head_dim, graph, spec):
    from tests.test_model_gpu import check_decode_logits, make_model

    model = make_model(torch.bfloat16, head_dim=head_dim, heads=4, kv_heads=4)
    with _PadRecorder() as rec:
        check_decode_logits(model, torch.bfloat16, graph, spec)
    cache = model.model.layers[0].self_attn.kv_cache
    assert cache.narrow and cache.per_completion_k_cache.shape[-1] == head_dim == cache.per_completion_v_cache.shape[-1]
    assert all(sc.k_cache.shape[-1] == 128 and sc.v_cache.shape[-1] == 128 for sc in cache.shared_caches)
    assert not any(sc.k_cache[..., head_dim:].any() for sc in cache.get_used_shared_caches()), "shared pad columns stay zero"
    # the unique cache is never pad-copied (the prefill pads its own, prompt-sized tensors: existing behaviour)
    rows = cache.per_completion_k_cache.shape[1]
    assert not [s for s in rec.shapes if len(s) == 4 and s[1] == rows], rec.shapes


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("spec", ["three-level", "padded-shared"])
def test_model_with_96_wide_heads(graph, spec):
    """A 4 / 4-head model with head dim 96 (Phi-3-mini's geometry, shrunk): narrow unique arena, 128-wide shared caches, the narrow
    preamble and suffix kernels in every decode step -- tests/test_model_gpu.py's logits check with its own bounds."""
    _check_model(96, graph, spec)


def test_model_with_80_wide_heads_under_the_graph():
    _check_model(80, True, "three-level")
