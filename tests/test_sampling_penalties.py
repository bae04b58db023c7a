"""-m "not gpu": repetition / presence / frequency penalties and logit bias -- the float64 definition (hydragen_amd/sampling.py)
against a per-row Python loop, host validation, the additive C ABI (hyd_sample_tokens_penalized, hyd_token_bitmap_build), the
new kernels' registers, and the tie census of the inputs the GPU tests use (tests/penalty_cases.py)."""
import ctypes as C
import inspect
import math
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, layer_ops, sampling
from hydragen_amd._lib import SamplePenaltyParams, TokenBitmapParams
from tests import penalty_cases as PC

REPO = Path(__file__).resolve().parent.parent
NEW = {"hyd_sample_tokens_penalized", "hyd_token_bitmap_build"}


# ---- the definition ------------------------------------------------------------------------------------------------------
def _loop(logits, r, a, f, bias, levels, gen, gen_len):
    """Dicts and sets, one row at a time.  levels: [(ids per group, lens per group, rows_per_group)] as Python lists."""
    out = []
    for b, row in enumerate(logits):
        ctx = set()
        for ids, lens, rpg in levels:
            grp = b // rpg
            ctx |= set(ids[grp][: lens[grp]])
        cnt = {}
        for t in (gen[b][: gen_len[b]] if gen is not None else []):
            if 0 <= t < len(row):
                cnt[t] = cnt.get(t, 0) + 1
        xs = []
        for v, l in enumerate(row):
            x = l
            if v in ctx or v in cnt:
                x = l / r if l > 0 else l * r
            if v in cnt:
                x -= f * cnt[v] + a
            if v in bias:
                x += bias[v]
            xs.append(x)
        out.append(xs)
    return out


@pytest.mark.parametrize("r, a, f", [(1.3, 0.5, 0.25), (0.7, -0.4, -0.1), (1.0, 0.0, 2.0), (2.5, 0.0, 0.0), (1.0, 1.5, 0.0)])
def test_penalize_logits_equals_a_python_loop(r, a, f):
    g = torch.Generator().manual_seed(int(r * 100))
    rows, n = 12, 97  # two words and a tail of the bitmap
    logits = torch.randn(rows, n, generator=g).double() * 3
    shapes = [(1, 20, 12), (3, 9, 4), (12, 5, 1)]  # (groups, L, rows_per_group): three levels, three group sizes
    levels, context = [], []
    for groups, L, rpg in shapes:
        ids = torch.randint(0, n, (groups, L), generator=g)
        lens = torch.randint(1, L + 1, (groups,), generator=g)
        levels.append((ids.tolist(), lens.tolist(), rpg))
        context.append((sampling.token_bitmap_reference(ids, lens, n), rpg))
    gen = torch.randint(0, 12, (rows, 10), generator=g).to(torch.int32)  # a small range: repeated tokens
    gen[3, 1] = -5
    gen[4, 0] = n + 3
    gen_len = torch.randint(0, 11, (rows,), generator=g).to(torch.int32)
    gen_len[0], gen_len[1] = 0, 10
    bias = {5: -math.inf, 96: 2.5, 0: -1.25, 40: 0.5}
    want = torch.tensor(_loop(logits.tolist(), r, a, f, bias, levels, gen.tolist(), gen_len.tolist()), dtype=torch.float64)
    got = sampling.penalize_logits(logits, r, a, f, bias, context, gen, gen_len)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    # the same list as an (ids, values) pair, and a 16-bit input
    pair = (torch.tensor(list(bias.keys())), torch.tensor(list(bias.values())))
    assert torch.equal(sampling.penalize_logits(logits, r, a, f, pair, context, gen, gen_len), want)
    h = logits.to(torch.bfloat16)
    assert torch.equal(sampling.penalize_logits(h, r, a, f, bias, context, gen, gen_len),
                       sampling.penalize_logits(h.double(), r, a, f, bias, context, gen, gen_len))


def test_hand_computed_examples():
    l = torch.tensor([[2.0, -2.0, 1.0, 4.0, -1.0]])
    ctx = [(sampling.token_bitmap_reference(torch.tensor([[0, 1]]), None, 5), 1)]
    # HF's RepetitionPenaltyLogitsProcessor: a positive logit is divided, a negative one multiplied; prompt tokens count
    x = sampling.penalize_logits(l, repetition_penalty=2.0, context=ctx)
    assert x.tolist() == [[1.0, -4.0, 1.0, 4.0, -1.0]]
    # generated tokens: repetition reaches them too; frequency scales with the count, presence does not
    gen, gl = torch.tensor([[3, 3, 4, 0]], dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    x = sampling.penalize_logits(l, repetition_penalty=2.0, context=ctx, gen=gen, gen_len=gl)
    assert x.tolist() == [[1.0, -4.0, 1.0, 2.0, -2.0]]
    x = sampling.penalize_logits(l, frequency_penalty=0.5, presence_penalty=0.25, context=ctx, gen=gen, gen_len=gl)
    assert x.tolist() == [[2.0, -2.0, 1.0, 4.0 - 1.0 - 0.25, -1.0 - 0.5 - 0.25]]  # the prompt alone costs nothing here
    # order: repetition, then the additive penalties, then the bias
    x = sampling.penalize_logits(l, 2.0, 0.25, 0.5, {3: 10.0, 2: -math.inf}, ctx, gen, gl)
    assert x.tolist() == [[1.0, -4.0, -math.inf, 4.0 / 2 - 1.25 + 10.0, -1.0 * 2 - 0.75]]
    assert not sampling.kept_mask(x)[0, 2]  # a banned token is never kept


def test_penalties_active_and_check_penalties():
    act = sampling.penalties_active
    assert not act() and not act(1.0, 0.0, 0.0, {}) and not act(None, None, None, (torch.tensor([]), torch.tensor([])))
    assert act(1.1) and act(None, -0.5) and act(None, None, 0.1) and act(logit_bias={3: 1.0}) and act(0.9)
    sampling.check_penalties(1.2, -3.0, 0.5, {1: -math.inf, 2: 0.0}, n=10)
    sampling.check_penalties()
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=math.nan),
                dict(repetition_penalty=math.inf), dict(presence_penalty=math.inf), dict(frequency_penalty=math.nan),
                dict(logit_bias={1: math.inf}), dict(logit_bias={1: math.nan}), dict(logit_bias={-1: 0.5}),
                dict(logit_bias={10: 0.5}, n=10), dict(logit_bias=(torch.tensor([1, 1]), torch.tensor([0.5, 0.5]))),
                dict(logit_bias=(torch.tensor([1, 2]), torch.tensor([0.5]))), dict(logit_bias=[1, 2, 3]),
                dict(logit_bias={i: 0.0 for i in range(sampling.BIAS_MAX + 1)})):
        with pytest.raises(ValueError):
            sampling.check_penalties(**bad)
    assert sampling.BIAS_MAX >= 1024 and sampling.BIAS_MAX == _lib.SAMPLE_BIAS_MAX and sampling.GEN_MAX == _lib.SAMPLE_GEN_MAX
    assert sampling.MAX_CONTEXT == _lib.SAMPLE_MAX_CONTEXT == _lib.HYD_MAX_LEVELS + 1


def test_token_bitmap_reference_and_cpu_operator():
    g = torch.Generator().manual_seed(3)
    n = 1000
    ids = torch.randint(-2, n + 2, (5, 70), generator=g)
    lens = torch.tensor([0, 1, 70, 33, 64])
    bits = sampling.token_bitmap_reference(ids, lens, n)
    assert bits.shape == (5, 32) and bits.dtype == torch.int32
    for grp in range(5):
        want = {t for t in ids[grp, : lens[grp]].tolist() if 0 <= t < n}
        got = {32 * w + b for w in range(32) for b in range(32) if (int(bits[grp, w]) >> b) & 1}
        assert got == want
    assert torch.equal(layer_ops.token_bitmap(ids, lens, n), bits)
    mask = sampling.context_mask([(bits, 2)], 10, n)
    assert mask.shape == (10, n) and torch.equal(mask[6], mask[7]) and int(mask[4].sum()) == len(set(ids[2].tolist()) & set(range(n)))


def test_penalties_dataclass_on_cpu_tensors():
    """The operator's CPU route: the definition, then torch; the list of generated tokens follows the draws."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 50, generator=g)
    pen = layer_ops.Penalties(frequency_penalty=100.0, gen=torch.zeros(4, 3, dtype=torch.int32),
                              gen_len=torch.zeros(4, dtype=torch.int32), append=True)
    toks = [layer_ops.sample_tokens(x, 0.0, penalties=pen) for _ in range(4)]  # one more than the list holds
    assert pen.gen_len.tolist() == [4] * 4 and torch.equal(pen.gen[:, :3].long(), torch.cat(toks[:3], 1))
    for b in range(4):  # a frequency penalty of 100 forbids repeats: the four largest logits, in order
        assert [int(t[b]) for t in toks] == torch.topk(x[b], 4).indices.tolist()
    tok, lp = layer_ops.sample_tokens(x, 0.0, penalties=layer_ops.Penalties(logit_bias=sampling.normalize_logit_bias(
        {int(x[0].argmax()): -math.inf})), return_logprobs=True)
    assert int(tok[0]) == int(torch.topk(x[0], 2).indices[1]) and lp.shape == (4, 1)
    # neutral penalties: the existing paths (which refuse CPU tensors), not the definition
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer_ops.sample_tokens(x, 0.0, penalties=layer_ops.Penalties(repetition_penalty=1.0))


def test_generate_takes_the_penalties():
    from hydragen_amd.llama import HydragenLlamaForCausalLM

    prm = inspect.signature(HydragenLlamaForCausalLM.generate).parameters
    for name in ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"):
        assert prm[name].default is None
    assert HydragenLlamaForCausalLM.fused_sampling_penalties is True


def test_model_shell_bookkeeping_on_a_cpu_model():
    """No operator runs on CPU tensors, so every forward of this model raises: what must hold around that."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig, PerLayerKVCache

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=2, vocab_size=64, max_position_embeddings=4096)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.float32, device="cpu")
    for layer in m.model.layers:
        layer.self_attn.kv_cache = PerLayerKVCache(4, 16, [1, 2], [16, 8], 2, 32, "cpu", torch.float32)
    m.kv_cache_allocated = True
    ids = torch.ones((1, 4), dtype=torch.long)
    # a level whose prefill fails leaves no token set behind
    with pytest.raises(Exception):
        m.append_shared(ids)
    assert m.shared_bitmaps == [] and m.get_num_used_shared_caches() == 0
    # the three penalties count at most GEN_MAX generated tokens, refused before anything runs; a bias alone has no such limit
    kw = dict(input_ids=ids, num_return_sequences=2, max_new_tokens=sampling.GEN_MAX + 1)
    for pen in (dict(repetition_penalty=1.2), dict(presence_penalty=0.1), dict(frequency_penalty=0.1)):
        with pytest.raises(ValueError, match=str(sampling.GEN_MAX)):
            m.generate(**pen, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # past the checks: the first forward
        m.generate(logit_bias={3: -math.inf}, **kw)
    with pytest.raises(ValueError, match="logit_bias ids"):
        m.generate(logit_bias={64: 1.0}, **kw)
    assert m.shared_bitmaps == [] and not hasattr(m, "track_context_tokens")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_declared():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.hyd_version() == 500  # additive: the version stays
    assert "#define HYD_SAMPLE_BIAS_MAX 1024" in header and "#define HYD_SAMPLE_GEN_MAX 2048" in header


def test_struct_sizes_gcc_vs_ctypes_and_unchanged():
    names = ["hyd_sample_penalty_params", "hyd_token_bitmap", "hyd_token_bitmap_params", "hyd_prefix_params", "hyd_partial",
             "hyd_suffix_params", "hyd_level", "hyd_decode_params", "hyd_rope_params", "hyd_add_rmsnorm_params", "hyd_swiglu_params",
             "hyd_sample_params", "hyd_sample_filter_params", "hyd_token_logprob_params", "hyd_kv_quant"]
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){'
           + "".join(f'printf("%zu ", sizeof({n}));' for n in names)
           + 'printf("%zu %zu %zu\\n", offsetof(hyd_sample_penalty_params, repetition_penalty), offsetof(hyd_sample_penalty_params, context),'
           ' offsetof(hyd_sample_penalty_params, bias_ids));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        sizes = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert sizes[0] == C.sizeof(SamplePenaltyParams) == 304
    assert sizes[1] == C.sizeof(_lib.TokenBitmap) == 16 and sizes[2] == C.sizeof(TokenBitmapParams) == 48
    assert sizes[15:] == [SamplePenaltyParams.repetition_penalty.offset, SamplePenaltyParams.context.offset,
                          SamplePenaltyParams.bias_ids.offset]
    # every existing struct keeps the size of ABI 0.5.0
    assert sizes[3:12] == [176, 24, 344, 80, 1024, 208, 96, 64, 56]
    assert sizes[12:15] == [C.sizeof(_lib.SampleFilterParams), C.sizeof(_lib.TokenLogprobParams), C.sizeof(_lib.KvQuant)] == [88, 80, 24]


def _pp(**kw):
    p = SamplePenaltyParams()
    p.logits = p.out = 4096  # never dereferenced: validation fails first
    p.rows, p.n, p.dtype, p.row_stride = 4, 1000, _lib.HYD_BF16, 1000
    p.temperature, p.top_p = 1.0, 1.0
    p.repetition_penalty = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_penalized_argument_validation():
    lib = _lib.load()
    err = lambda: lib.hyd_last_error_string().decode()  # noqa: E731
    call = lambda p: lib.hyd_sample_tokens_penalized(C.byref(p), None)  # noqa: E731
    BAD, UNSUP = -1, -2
    assert lib.hyd_sample_tokens_penalized(None, None) == BAD
    for r in (0.0, -1.5, math.nan, math.inf):
        assert call(_pp(repetition_penalty=r)) == BAD and "repetition_penalty" in err()
    for k in ("frequency_penalty", "presence_penalty"):
        for v in (math.inf, -math.inf, math.nan):
            assert call(_pp(**{k: v})) == BAD and k in err()
    assert call(_pp(n_context=_lib.SAMPLE_MAX_CONTEXT + 1)) == BAD and "n_context" in err()
    assert call(_pp(n_context=-1)) == BAD
    p = _pp(n_context=2)
    p.context[0].bits, p.context[0].rows_per_group = 4096, 1
    assert call(p) == BAD and "context[1].bits is null" in err()
    p.context[1].bits, p.context[1].rows_per_group = 4096, 0
    assert call(p) == BAD and "rows_per_group" in err()
    p.context[1].bits, p.context[1].rows_per_group = 4098, 2
    assert call(p) == BAD and "aligned" in err()
    assert call(_pp(gen_len=4096)) == BAD and "gen and gen_len" in err()
    assert call(_pp(gen=4096)) == BAD and "gen and gen_len" in err()
    assert call(_pp(gen=4096, gen_len=4096, gen_stride=-1)) == BAD
    assert call(_pp(gen=4096, gen_len=4096, gen_stride=_lib.SAMPLE_GEN_MAX + 1)) == UNSUP and "gen_stride" in err()
    assert call(_pp(append_out=1)) == BAD and "append_out" in err()
    assert call(_pp(n_bias=_lib.SAMPLE_BIAS_MAX + 1, bias_ids=4096, bias_values=4096)) == BAD and "n_bias" in err()
    assert call(_pp(n_bias=3)) == BAD and "bias_ids" in err()
    assert call(_pp(n_bias=3, bias_ids=4100, bias_values=4096)) == BAD and "aligned" in err()
    assert call(_pp(gen=4098, gen_len=4096)) == BAD and "aligned" in err()
    assert call(_pp(logits=4097)) == BAD and "aligned" in err()
    assert call(_pp(n=_lib.SAMPLE_FILTER_MAX_N + 1, row_stride=_lib.SAMPLE_FILTER_MAX_N + 1)) == UNSUP and "rows of up to" in err()
    assert call(_pp(dtype=7)) == UNSUP and "dtype 7" in err()
    # what hyd_sample_tokens_filtered refuses
    assert call(_pp(top_k=-1)) == BAD and call(_pp(top_p=0.0)) == BAD and call(_pp(min_p=1.5)) == BAD
    assert call(_pp(temperature=-1.0)) == BAD and call(_pp(row_stride=999)) == BAD and call(_pp(out=0)) == BAD
    assert call(_pp(rows=0)) == 0  # nothing to launch


def test_token_bitmap_argument_validation():
    lib = _lib.load()
    call = lambda **kw: lib.hyd_token_bitmap_build(C.byref(TokenBitmapParams(**{**dict(ids=4096, bits=4096, id_stride=8, groups=2, L=8, n=100), **kw})), None)  # noqa: E731
    assert lib.hyd_token_bitmap_build(None, None) == -1
    for bad in (dict(ids=0), dict(bits=0), dict(groups=-1), dict(groups=70000), dict(L=-1), dict(n=0), dict(n=_lib.SAMPLE_FILTER_MAX_N + 1),
                dict(id_stride=7), dict(ids=4100), dict(lens=4100), dict(bits=4098)):
        assert call(**bad) == -1, bad
    assert call(groups=0) == 0 and call(L=0, id_stride=0) == 0


# ---- the new kernels' registers --------------------------------------------------------------------------------------------
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_penalty_kernels_have_no_scratch_and_fit_two_rows_per_cu():
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                          str(REPO / "hydragen_amd" / "csrc" / "sample_penalty.hip"), "-o", "-"], capture_output=True, text=True,
                         check=True).stdout
    seen = {}
    for blk in out.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spill == 0 and scratch == 0, (name, spill, scratch)
        seen[name] = (vgpr, lds)
    pen = {k: v for k, v in seen.items() if "sample_penalty_kernel" in k}
    assert len(pen) == 3 and len(seen) == 4  # f16, bf16, fp32 + the bitmap builder
    for name, (vgpr, lds) in pen.items():
        # 1024 threads = 4 waves per SIMD: two rows per CU need <= 64 VGPRs and <= 80 KB of the CU's 160 KB LDS
        assert vgpr <= 64 and lds <= 80 * 1024, (name, vgpr, lds)
    if "roc-7.2.0 26014" in out:  # what this hipcc gives (its .ident line), pinned: 52 -> 64 would pass the ceiling unseen
        got = {re.search(r"ILi(\d)E", k).group(1): v for k, v in pen.items()}  # template argument: HYD_F16 0, HYD_BF16 1, HYD_F32 2
        assert got == {"0": (52, 72016), "1": (50, 72016), "2": (58, 72016)}, got
        assert next(v for k, v in seen.items() if "token_bitmap_kernel" in k) == (8, 0)
    assert next(v for k, v in seen.items() if "token_bitmap_kernel" in k)[1] == 0


# ---- the tie census --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.CASES))
def test_tie_census(name):
    """From the float64 definition alone, on the inputs of the GPU tests: the share of rows whose best and second-best
    penalised logits differ by less than 4 fp32 ulps (the rows a temperature-0 test may leave out) is at most 0.5 %."""
    case = PC.build(name)
    rows = case["logits"].shape[0]
    inside = 0
    for s in range(0, rows, 64):
        inside += int(PC.margin_rows(PC.penalised(case, slice(s, min(s + 64, rows)))).sum())
    print(f"{name}: {inside} of {rows} rows inside the margin")
    assert inside <= 0.005 * rows
