"""-m "not gpu": speculative decoding -- the two torch definitions of hydragen_amd/speculative.py on hand-written cases, the assembled
multi-token attention against a float64 dense softmax written out here, generate()'s refusals, the additive C ABI (struct
layouts, argument validation without a launch) and the register budget of the causal-tail instantiations."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, speculative
from hydragen_amd.speculative import Segment, accept_reference, prompt_lookup_reference

REPO = Path(__file__).resolve().parent.parent
NEW = {"hyd_suffix_attn_causal_fwd", "hyd_rope_append_multi", "hyd_draft_lookup", "hyd_draft_accept"}


def ids(*rows):
    return torch.tensor(rows, dtype=torch.int64)


# ---- prompt lookup ------------------------------------------------------------------------------------------------------------
def lookup(seq, k=3, ngram=(1, 3)):
    d, n = prompt_lookup_reference([Segment(ids(seq))], 1, k, ngram)
    return d[0].tolist(), int(n[0])


def test_lookup_longest_ngram_wins_over_a_later_shorter_one():
    #      0  1  2  3  4  5  6  7  8  9 10 11
    seq = [1, 2, 3, 9, 8, 7, 3, 5, 6, 1, 2, 3]
    # the 1-gram [3] occurs latest at 6 (followers 5 6 1), the 3-gram [1 2 3] only at 0..2 (followers 9 8 7): the 3-gram wins
    assert lookup(seq) == ([9, 8, 7], 3)
    assert lookup(seq, ngram=(1, 1)) == ([5, 6, 1], 3)


def test_lookup_latest_occurrence_wins():
    seq = [4, 5, 1, 1, 1, 4, 5, 2, 2, 2, 4, 5]
    assert lookup(seq, ngram=(2, 2)) == ([2, 2, 2], 3)


def test_lookup_trivial_match_at_the_end_is_excluded():
    assert lookup([7, 8, 9]) == ([0, 0, 0], 0)            # the only occurrence of [9] is the last position itself
    assert lookup([5, 5], k=2) == ([5, 0], 1)             # ... but an occurrence ending one before it counts
    assert lookup([3], k=2) == ([0, 0], 0) and lookup([], k=2) == ([0, 0], 0)


def test_lookup_fewer_than_k_followers_gives_filler():
    assert lookup([1, 2, 6, 1, 2], k=4, ngram=(2, 3)) == ([6, 1, 2, 0], 3)
    assert lookup([1, 2, 1, 2], k=7, ngram=(2, 2)) == ([1, 2, 0, 0, 0, 0, 0], 2)


def test_lookup_ngram_longer_than_the_sequence_is_skipped():
    assert lookup([2, 2], k=1, ngram=(1, 3)) == ([2], 1)  # n = 3 and n = 2 are skipped / find nothing, n = 1 matches at 0


def test_lookup_crosses_level_prompt_and_generated_boundaries_and_maps_rows():
    B = 4
    level0 = Segment(ids([1, 2, 3, 4]))                                         # one sequence for all rows
    level1 = Segment(ids([5, 6, 0], [7, 8, 9]), torch.tensor([2, 3]))           # rows 0-1 read row 0 (2 tokens), rows 2-3 row 1
    prompt = Segment(ids([4, 5], [3, 4], [9, 1], [2, 3]), torch.tensor([2, 2, 2, 1], dtype=torch.int32))
    gen = Segment(ids([6, 4, 0], [5, 0, 0], [2, 3, 4], [4, 7, 0]), torch.tensor([2, 1, 3, 2]))
    seqs = speculative.logical_sequences([level0, level1, prompt, gen], B)
    assert seqs == [[1, 2, 3, 4, 5, 6, 4, 5, 6, 4], [1, 2, 3, 4, 5, 6, 3, 4, 5], [1, 2, 3, 4, 7, 8, 9, 9, 1, 2, 3, 4], [1, 2, 3, 4, 7, 8, 9, 2, 4, 7]]
    d, n = prompt_lookup_reference([level0, level1, prompt, gen], B, 3)
    # row 0: [5 6 4] (prompt + generated) matched at level1/prompt boundary 4..6 -> followers 5 6 4 span prompt and generated
    # row 1: [3 4 5] spans prompt + generated, matched in level0 + level1 at 2..4 -> followers 6 (level1) 3 4 (prompt)
    # row 2: [2 3 4] in generated, matched in level0 -> followers 7 8 9 of level1 row 1
    # row 3: [4 7] spans nothing earlier as a 3-gram [2 4 7]; the 2-gram [4 7] is at 3..4 (level0 / level1) -> 8 9 2
    assert d.tolist() == [[5, 6, 4], [6, 3, 4], [7, 8, 9], [8, 9, 2]] and n.tolist() == [3, 3, 3, 3]


def test_lookup_argument_checks():
    seg = [Segment(ids([1, 2]))]
    for k in (0, 8, -1, True, 2.0):
        with pytest.raises(ValueError, match="draft_tokens"):
            prompt_lookup_reference(seg, 1, k)
    for ng in ((0, 3), (3, 2), (1, 9)):
        with pytest.raises(ValueError, match="ngram"):
            prompt_lookup_reference(seg, 1, 2, ng)
    with pytest.raises(ValueError, match="dividing the batch"):
        prompt_lookup_reference([Segment(ids([1], [2], [3]))], 4, 2)


# ---- acceptance ---------------------------------------------------------------------------------------------------------------
def run_accept(fed, sampled, length, max_new=16, eos=(), pad=99, reason=None, shared_len=None, retire=True, lp=False):
    rows = len(fed)
    out, ln, rs, si, olp = speculative.new_state(rows, max_new, pad, logprobs=lp)
    ln[:] = torch.tensor(length, dtype=torch.int32)
    if reason is not None:
        rs[:] = torch.tensor(reason, dtype=torch.int32)
    start = torch.arange(rows, dtype=torch.int64) * 10 + 100
    logp = -torch.arange(rows * len(fed[0]), dtype=torch.float32).reshape(rows, -1) - 1 if lp else None
    feed, pos, acc, live = accept_reference(ids(*fed), ids(*sampled), out, ln, rs, si, start, shared_len, eos, pad, max_new, retire, logp, olp)
    return dict(out=out, length=ln.tolist(), reason=rs.tolist(), stop_index=si.tolist(), feed=feed.tolist(), pos=pos.tolist(),
                accepted=acc.tolist(), live=live, olp=olp)


def test_accept_all_right_first_wrong_and_in_between():
    r = run_accept(fed=[[5, 1, 2, 3], [5, 1, 2, 3], [5, 1, 2, 3]],
                   sampled=[[1, 2, 3, 4], [7, 2, 3, 4], [1, 2, 8, 4]], length=[3, 3, 3], lp=True)
    assert r["length"] == [7, 4, 6] and r["accepted"] == [3, 0, 2] and r["live"] == 3
    assert r["out"][0, 3:7].tolist() == [1, 2, 3, 4] and r["out"][1, 3:5].tolist() == [7, 99] and r["out"][2, 3:7].tolist() == [1, 2, 8, 99]
    assert r["feed"] == [4, 7, 8]                                  # the next step's first token is the last emitted one
    assert r["pos"] == [100 + 6, 110 + 3, 120 + 5]                 # ... at start_pos + length - 1
    assert r["olp"][0, 3:7].tolist() == [-1, -2, -3, -4] and r["olp"][1, 3:5].tolist() == [-5, 0] and r["olp"][2, 3:7].tolist() == [-9, -10, -11, 0]
    # the emitted tokens are always a prefix of `sampled`
    for b, smp in enumerate([[1, 2, 3, 4], [7, 2, 3, 4], [1, 2, 8, 4]]):
        n = r["length"][b] - 3
        assert r["out"][b, 3:3 + n].tolist() == smp[:n]


def test_accept_eos_inside_the_accepted_run_cuts_there():
    r = run_accept(fed=[[5, 1, 2, 3]], sampled=[[1, 2, 3, 4]], length=[2], eos=(42, 2), shared_len=torch.tensor([64]))
    assert r["length"] == [4] and r["reason"] == [1] and r["stop_index"] == [1] and r["accepted"] == [1] and r["live"] == 0
    assert r["out"][0, :6].tolist() == [99, 99, 1, 2, 99, 99]       # the EOS token is kept, nothing behind it
    assert r["feed"] == [99] and r["pos"] == [63]                   # a finished row: pad, at shared_len - 1
    # an EOS id behind the first wrong draft is never emitted
    r = run_accept(fed=[[5, 1, 2, 3]], sampled=[[7, 42, 3, 4]], length=[2], eos=(42,))
    assert r["length"] == [3] and r["reason"] == [0] and r["live"] == 1


def test_accept_max_new_tokens_cut_and_finished_rows():
    r = run_accept(fed=[[5, 1, 2, 3], [5, 1, 2, 3], [5, 1, 2, 3]], sampled=[[1, 2, 3, 4]] * 3, length=[6, 8, 3], max_new=8,
                   reason=[0, 0, 1], retire=True)
    assert r["length"] == [8, 8, 3] and r["reason"] == [0, 0, 1] and r["accepted"] == [1, 0, 0] and r["live"] == 0
    assert r["out"][0].tolist() == [99] * 6 + [1, 2] and r["out"][1].tolist() == [99] * 8 and r["out"][2].tolist() == [99] * 8
    assert r["feed"] == [99, 99, 99] and r["pos"] == [-1, -1, -1]  # no shared_len: position -1 retires the row
    r = run_accept(fed=[[5, 1]], sampled=[[1, 2]], length=[8], max_new=8, retire=False)
    assert r["pos"] == [100 + 7] and r["feed"] == [99]


def test_accept_first_token_enters_as_a_step_of_one():
    r = run_accept(fed=[[0], [0]], sampled=[[11], [42]], length=[0, 0], eos=(42,))
    assert r["length"] == [1, 1] and r["reason"] == [0, 1] and r["out"][:, 0].tolist() == [11, 42] and r["feed"] == [11, 99]
    assert r["pos"] == [100, -1] and r["accepted"] == [0, 0] and r["live"] == 1


# ---- the assembled attention definition against a dense float64 softmax ----------------------------------------------------------
def dense_causal_tail(q, k, v, seq_lens, shared):
    """float64, one (row, token, head) at a time: the keys of every shared level on the row's path, then the unique keys below
    seq_len - (T - 1 - i); softmax(q . k / sqrt(D)) . v."""
    B, T, Hq, D = q.shape
    g = Hq // k.shape[2]
    out = torch.zeros_like(q)
    for b in range(B):
        for i in range(T):
            lim = max(0, int(seq_lens[b]) - (T - 1 - i))
            for h in range(Hq):
                ks = [sk[b // (B // sk.shape[0]), :, h // g] for sk, _ in shared] + [k[b, :lim, h // g]]
                vs = [sv[b // (B // sv.shape[0]), :, h // g] for _, sv in shared] + [v[b, :lim, h // g]]
                kk, vv = torch.cat(ks), torch.cat(vs)
                if kk.shape[0]:
                    out[b, i, h] = torch.softmax(kk @ q[b, i, h] / D ** 0.5, 0) @ vv
    return out


def torch_ops():
    def attend(q, k, v, mask):  # q [B, T, Hq, D], k / v [B, S, Hkv, D], mask [B, T, S] bool -> out, lse [B, T, Hq]
        g = q.shape[2] // k.shape[2]
        kk, vv = k.repeat_interleave(g, 2), v.repeat_interleave(g, 2)
        s = torch.einsum("bthd,bshd->bths", q, kk) / q.shape[-1] ** 0.5
        s = s.masked_fill(~mask[:, :, None, :], float("-inf"))
        lse = torch.logsumexp(s, -1)
        p = torch.exp(s - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)[..., None])
        return torch.einsum("bths,bshd->bthd", p, vv), lse

    def seqlen(q, k, v, lens):
        return attend(q, k, v, (torch.arange(k.shape[1])[None, None, :] < lens[:, None, None]).expand(q.shape[0], q.shape[1], -1))

    def causal(q, k, v):
        T = q.shape[1]
        o, l = attend(q, k, v, torch.tril(torch.ones(T, T, dtype=torch.bool))[None].expand(q.shape[0], -1, -1))
        return o, l.transpose(1, 2)  # [B, Hq, T], as flash_attention returns it

    def level(q, sk, sv, scu, smax, uv):
        assert not uv
        per = q.shape[0] // sk.shape[0]
        return attend(q, sk.repeat_interleave(per, 0), sv.repeat_interleave(per, 0), torch.ones(q.shape[0], q.shape[1], sk.shape[1], dtype=torch.bool))

    def combine(outs, lses):
        L = torch.stack(lses)
        m = L.max(0).values
        w = torch.exp(L - torch.where(torch.isinf(m), torch.zeros_like(m), m))
        return (torch.stack(outs) * w[..., None]).sum(0) / w.sum(0)[..., None]

    return dict(seqlen=seqlen, causal=causal, level=level, combine=combine)


@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("Hq, Hkv", [(4, 4), (6, 2)])
def test_assembled_definition_is_the_dense_causal_tail(T, Hq, Hkv):
    torch.manual_seed(10 * T + Hq)
    B, D, S = 2, 64, 12
    q = torch.randn(B, T, Hq, D, dtype=torch.float64)
    k, v = torch.randn(B, S, Hkv, D, dtype=torch.float64), torch.randn(B, S, Hkv, D, dtype=torch.float64)
    shared = [(torch.randn(1, 7, Hkv, D, dtype=torch.float64), torch.randn(1, 7, Hkv, D, dtype=torch.float64))]
    seq_lens = torch.tensor([T, 11])
    for levels in ([], shared):
        got = speculative.assembled_causal_tail_attention(q, k, v, seq_lens, [a for a, _ in levels], [b for _, b in levels], ops=torch_ops())
        want = dense_causal_tail(q, k, v, seq_lens, levels)
        assert torch.allclose(got, want, rtol=0, atol=1e-12), float((got - want).abs().max())
    # a retired row (length 0) sees the shared keys only
    got = speculative.assembled_causal_tail_attention(q, k, v, torch.tensor([0, 9]), [shared[0][0]], [shared[0][1]], ops=torch_ops())
    assert torch.allclose(got, dense_causal_tail(q, k, v, torch.tensor([0, 9]), shared), rtol=0, atol=1e-12)
    # ... and the non-causal form (every query sees every new key) is a different function
    full = torch_ops()["seqlen"](q, k, v, seq_lens)[0]
    assert float((full - dense_causal_tail(q, k, v, seq_lens, [])).abs().max()) > 1e-3


# ---- generate(): refusals before any launch ------------------------------------------------------------------------------------
def cpu_model(**cache_kw):
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig, PerLayerKVCache

    cfg = LlamaConfig(hidden_size=128, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=2, vocab_size=64, max_position_embeddings=64)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.float32, device="cpu")
    for layer in m.model.layers:
        layer.self_attn.kv_cache = PerLayerKVCache(4, 16, [1, 2], [16, 8], 2, 64, "cpu", torch.float32, **cache_kw)
    m.kv_cache_allocated = True
    return m


@pytest.fixture(scope="module")
def model():
    return cpu_model()


PROMPT = torch.ones((1, 4), dtype=torch.long)


@pytest.mark.parametrize("kw, words", [
    (dict(repetition_penalty=1.2), "penalties"), (dict(presence_penalty=0.5), "penalties"), (dict(frequency_penalty=0.5), "penalties"),
    (dict(logit_bias={3: -1.0}), "logit_bias"), (dict(stop=[[1, 2]]), "stop"), (dict(token_overrides=torch.ones((2, 4), dtype=torch.long)), "token_overrides"),
    (dict(return_logprobs=True, top_logprobs=2), "top_logprobs"), (dict(return_logits=True), "return_logits"),
    (dict(disable_hydragen=True), "disable_hydragen"), (dict(disable_attention=True), "disable_attention"),
    (dict(disable_hierarchy=True), "disable_hierarchy"),
])
def test_generate_refuses_what_a_speculative_step_does_not_carry(model, kw, words):
    with pytest.raises(NotImplementedError, match=words):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, **kw)


def test_generate_refuses_constraint_and_bad_draft_arguments(model):
    from hydragen_amd.constraint import TokenDFA

    with pytest.raises(NotImplementedError, match="constraint"):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, constraint=TokenDFA.from_choices([[1, 2]], 64, on_accept="free"))
    for k in (8, -1, 2.5, True):
        with pytest.raises(ValueError, match="draft_tokens"):
            model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=k)
    with pytest.raises(ValueError, match="ngram"):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, ngram=(2, 1))
    with pytest.raises(ValueError, match="draft"):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, draft="model")
    with pytest.raises(ValueError, match="max_new_tokens = 4"):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, draft=torch.zeros((2, 5), dtype=torch.long))
    with pytest.raises(ValueError, match="return_draft_stats"):
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, return_draft_stats=True)
    with pytest.raises(ValueError, match="GPU"):  # a model on the CPU
        model.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2)


def test_generate_refuses_fp8_unique_caches():
    m = cpu_model(kv_cache_dtype=torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2)


@pytest.mark.parametrize("heads, head_dim, narrow", [(4, 96, True), (2, 80, False)])
def test_generate_refuses_narrow_head_dims(heads, head_dim, narrow):
    """Head dims other than 64 / 128 / 256 -- with the unique cache kept at its true width (narrow) or not -- before any launch."""
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig, PerLayerKVCache

    cfg = LlamaConfig(hidden_size=heads * head_dim, intermediate_size=128, num_hidden_layers=1, num_attention_heads=heads,
                      num_key_value_heads=heads, vocab_size=64, max_position_embeddings=64)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device="cpu")
    for layer in m.model.layers:
        layer.self_attn.kv_cache = PerLayerKVCache(4, 16, [1, 2], [16, 8], heads, head_dim, "cpu", torch.bfloat16)
    m.kv_cache_allocated = True
    assert m.model.layers[0].self_attn.kv_cache.narrow == narrow
    with pytest.raises(NotImplementedError, match="head dim"):
        m.generate(PROMPT, num_return_sequences=2, max_new_tokens=4, draft_tokens=2)


def test_generate_refuses_more_levels_than_the_lookup_has_segments(model):
    """Given levels + the generated tail must fit hyd_draft_lookup's segment table: refused before any launch, not in mid-decode."""
    levels = [PROMPT] * 10
    with pytest.raises(ValueError, match="segments"):
        model.generate(levels, num_return_sequences=2, max_new_tokens=4, draft_tokens=2)
    with pytest.raises(ValueError, match="GPU"):  # (given drafts search nothing: the count does not matter, the next check speaks)
        model.generate(levels, num_return_sequences=2, max_new_tokens=4, draft_tokens=2, draft=torch.zeros((2, 4), dtype=torch.long))


def test_room_check_demands_k_extra_rows(model):
    start = torch.tensor([[4], [4]])
    model._check_room(start, 13)  # last cache index 4 + 13 - 2 = 15 < 16
    with pytest.raises(ValueError, match="unique cache holds 16"):
        model._check_room(start, 13, extra=1)
    model._check_room(start, 10, extra=3)


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (8, 2)])
def test_end_to_end_seeds_keep_every_greedy_decision_clear_of_the_gap(heads, kv_heads):
    """The condition of the GPU end-to-end test, checked with the float64 model alone: on the chosen seed every top-2 gap of the
    greedy decode is above GAP (twice the measured logit error of plain decoding), so no row has to be cut short."""
    from tests import test_speculative_gpu as tg

    seed = tg.SEEDS[(heads, kv_heads)]
    model, seq = tg.cpu_model(heads, kv_heads, seed), tg.cpu_prompts(seed)
    gaps = []
    for _ in range(tg.NEW):
        top = tg.ref_logits64(model, seq)[:, -1].topk(2, -1)
        gaps.append(float((top.values[:, 0] - top.values[:, 1]).min()))
        seq = torch.cat([seq, top.indices[:, :1]], 1)
    assert min(gaps) >= 2 * tg.GAP, (min(gaps), tg.GAP)  # (twice: plain decoding's own error may move a gap by up to GAP)


@pytest.mark.parametrize("heads, kv_heads", [(4, 4), (4, 2)])
def test_ragged_seeds_keep_five_rows_in_six_clear_of_the_gap(heads, kv_heads):
    """The same for the ragged inputs of tests/test_speculative_paths_gpu.py, whose condition allows one cut row in six: per row the
    smallest top-2 gap of the float64 greedy decode; every row is above GAP and all but one above 2 GAP."""
    from tests import test_speculative_gpu as tg
    from tests import test_speculative_paths_gpu as tp

    seed = tp.RAGGED_SEEDS[(heads, kv_heads)]
    model = tg.cpu_model(heads, kv_heads, seed)
    shared, uniq = tp.ragged_inputs(seed)
    rows = []
    for b, n in enumerate(tp.RAGGED_LENS):
        seq, gaps = torch.cat([shared[b // 3], uniq[b, :n]])[None], []
        for _ in range(tp.RAGGED_NEW):
            top = tg.ref_logits64(model, seq)[:, -1].topk(2, -1)
            gaps.append(float(top.values[0, 0] - top.values[0, 1]))
            seq = torch.cat([seq, top.indices[:, :1]], 1)
        rows.append(min(gaps))
    assert min(rows) > tg.GAP and sorted(rows)[1] >= 2 * tg.GAP, rows
    assert [round(x, 4) for x in sorted(rows)[:2]] == list(tp.RAGGED_GAPS[(heads, kv_heads)]) and (heads, kv_heads) in tp.RAGGED_GEOMETRIES
    assert min(tp.RAGGED_LENS) < 16 < max(tp.RAGGED_LENS) and 32 < max(tp.RAGGED_LENS) and len(set(tp.RAGGED_LENS)) == 6


# ---- the C ABI: additive, validated without a launch ----------------------------------------------------------------------------
def test_symbols_declared_exported_and_version_stays():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS) and all(hasattr(lib, n) for n in NEW)
    assert lib.hyd_version() == 500 == _lib.ABI_VERSION
    assert re.search(r"#define HYD_DRAFT_MAX_SEGMENTS \(HYD_MAX_LEVELS \+ 2\)", header) and re.search(r"#define HYD_DRAFT_MAX_NGRAM 8\b", header)
    assert (_lib.DRAFT_MAX_SEGMENTS, _lib.DRAFT_MAX_NGRAM) == (10, 8)


def test_struct_layouts_gcc_vs_ctypes():
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(hyd_decode_params), offsetof(hyd_decode_params, causal_tail), sizeof(hyd_rope_multi_params), offsetof(hyd_rope_multi_params, T), '
           'sizeof(hyd_draft_segment), sizeof(hyd_draft_lookup_params), offsetof(hyd_draft_lookup_params, K), sizeof(hyd_draft_accept_params), '
           'offsetof(hyd_draft_accept_params, eos), offsetof(hyd_draft_accept_params, retire));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    L = _lib
    assert got == [C.sizeof(L.DecodeParams), L.DecodeParams.causal_tail.offset, C.sizeof(L.RopeMultiParams), L.RopeMultiParams.T.offset,
                   C.sizeof(L.DraftSegment), C.sizeof(L.DraftLookupParams), L.DraftLookupParams.K.offset, C.sizeof(L.DraftAcceptParams),
                   L.DraftAcceptParams.eos.offset, L.DraftAcceptParams.retire.offset]


PTR = 0x10000  # never dereferenced: validation fails first


def err(rc):
    return rc, _lib.load().hyd_last_error_string().decode()


def suffix_params(**kw):
    s = _lib.SuffixParams()
    s.dtype, s.B, s.nq, s.Hq, s.Hkv, s.D, s.kv_len = 1, 4, 3, 8, 2, 128, 16
    s.q = s.k = s.v = s.out = PTR
    s.k_tok_stride = s.v_tok_stride = 256
    s.k_head_stride = s.v_head_stride = 128
    s.k_batch_stride = s.v_batch_stride = 16 * 256
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("kw, code, frag", [
    (dict(nq=1), -1, "2 to 8"), (dict(nq=9), -1, "2 to 8"), (dict(q=None), -1, "null"), (dict(out=PTR + 8), -1, "aligned"),
    (dict(k=PTR + 2), -1, "aligned"), (dict(kv_dim=64), -2, "kv_dim"), (dict(D=96), -2, "head_dim"), (dict(n_partials=9), -1, "n_partials"),
])
def test_causal_suffix_entry_point_rejects_bad_arguments(kw, code, frag):
    lib = _lib.load()
    rc, msg = err(lib.hyd_suffix_attn_causal_fwd(C.byref(suffix_params(**kw)), None))
    assert rc == code and frag in msg, (rc, msg)


def test_decode_causal_tail_field_is_validated_and_refused_for_fp8_and_narrow_rows():
    lib = _lib.load()
    d = _lib.DecodeParams()
    d.suffix = suffix_params()
    d.n_levels = 1
    d.levels[0].sb, d.levels[0].kv_len = 1, 64
    d.levels[0].k = d.levels[0].v = PTR
    d.causal_tail = 2
    rc, msg = err(lib.hyd_decode_attn_fused(C.byref(d), None))
    assert rc == -1 and "causal_tail" in msg
    d.causal_tail = 1
    d.suffix.nq = 1
    rc, msg = err(lib.hyd_decode_attn_fused(C.byref(d), None))
    assert rc == -1 and "2 to 8" in msg
    d.suffix.nq = 3
    kq = _lib.KvQuant()
    kq.kv_dtype, kq.flags = _lib.HYD_FP8_E4M3, _lib.HYD_KVQ_GQA
    rc, msg = err(lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(kq), None))
    assert rc == -2 and "fp8" in msg
    d.suffix.kv_dim = 64
    rc, msg = err(lib.hyd_decode_attn_fused(C.byref(d), None))
    assert rc == -2 and "kv_dim" in msg


def rope_multi_params(**kw):
    p = _lib.RopeMultiParams()
    for f in ("q", "k", "v", "q_out", "k_cache", "v_cache", "cos", "sin", "position_ids", "shared_len", "seq_lens"):
        setattr(p, f, PTR)
    p.dtype, p.B, p.T, p.Hq, p.Hkv, p.D, p.cache_len, p.max_pos = 1, 4, 3, 8, 2, 128, 32, 64
    p.q_tok_stride, p.k_tok_stride, p.v_tok_stride = 1024, 256, 256
    p.q_batch_stride, p.k_batch_stride, p.v_batch_stride = 3072, 768, 768
    p.cs_stride, p.pos_stride = 128, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code, frag", [
    (dict(T=1), -1, "2 to 8"), (dict(T=9), -1, "2 to 8"), (dict(q=None), -1, "q is null"), (dict(k_cache=PTR + 4), -1, "aligned"),
    (dict(position_ids=None), -1, "null"), (dict(seq_lens=None), -1, "null"), (dict(position_ids=PTR + 4), -1, "aligned"),
    (dict(q_tok_stride=1020), -1, "q_tok_stride"), (dict(D=96), -2, "head_dim"), (dict(dtype=2), -2, "dtype"), (dict(cache_len=0), -1, "cache_len"),
    (dict(max_pos=0), -1, "max_pos"), (dict(cs_stride=126), -1, "cos/sin"), (dict(B=0), -1, "non-positive"),
])
def test_rope_append_multi_rejects_bad_arguments(kw, code, frag):
    rc, msg = err(_lib.load().hyd_rope_append_multi(C.byref(rope_multi_params(**kw)), None))
    assert rc == code and frag in msg, (rc, msg)
    assert _lib.load().hyd_rope_append_multi(None, None) == -1


def lookup_params(**kw):
    p = _lib.DraftLookupParams()
    p.drafts = p.n_proposed = PTR
    p.n_segments, p.B, p.K, p.ngram_min, p.ngram_max, p.drafts_stride = 2, 4, 3, 1, 3, 3
    for i in range(2):
        p.segments[i].ids, p.segments[i].len, p.segments[i].div, p.segments[i].row_stride = PTR, 8, 1 + i, 8
    for k, v in kw.items():
        if k.startswith("seg_"):
            setattr(p.segments[1], k[4:], v)
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, frag", [
    (dict(K=0), "1 to 7"), (dict(K=8), "1 to 7"), (dict(ngram_min=0), "ngram"), (dict(ngram_max=9), "ngram"), (dict(ngram_min=3, ngram_max=2), "ngram"),
    (dict(n_segments=0), "n_segments"), (dict(n_segments=11), "n_segments"), (dict(drafts=None), "null"), (dict(n_proposed=None), "null"),
    (dict(drafts=PTR + 4), "aligned"), (dict(n_proposed=PTR + 2), "aligned"), (dict(drafts_stride=2), "drafts_stride"), (dict(B=-1), "B -1"),
    (dict(seg_div=0), "segment 1"), (dict(seg_ids=None), "segment 1"), (dict(seg_ids=PTR + 4), "segment 1"), (dict(seg_lens_i32=PTR + 2), "segment 1"),
])
def test_draft_lookup_rejects_bad_arguments(kw, frag):
    rc, msg = err(_lib.load().hyd_draft_lookup(C.byref(lookup_params(**kw)), None))
    assert rc == -1 and frag in msg, (rc, msg)


def accept_params(**kw):
    p = _lib.DraftAcceptParams()
    for f in ("fed", "sampled", "out", "length", "reason", "stop_index", "accepted", "live", "start_pos", "shared_len", "feed", "next_pos"):
        setattr(p, f, PTR)
    p.rows, p.T, p.n_eos, p.max_new_tokens, p.out_stride = 4, 4, 1, 24, 24
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, frag", [
    (dict(T=0), "1 to 8"), (dict(T=9), "1 to 8"), (dict(rows=-1), "rows"), (dict(n_eos=17), "n_eos"), (dict(n_eos=-1), "n_eos"),
    (dict(max_new_tokens=0), "max_new_tokens"), (dict(max_new_tokens=25), "max_new_tokens"),
    (dict(fed=None), "null"), (dict(sampled=None), "null"), (dict(out=None), "null"), (dict(length=None), "null"), (dict(reason=None), "null"),
    (dict(stop_index=None), "null"), (dict(accepted=None), "null"), (dict(live=None), "null"), (dict(start_pos=None), "null"),
    (dict(feed=None), "null"), (dict(next_pos=None), "null"),
    (dict(fed=PTR + 4), "aligned"), (dict(out=PTR + 4), "aligned"), (dict(live=PTR + 2), "aligned"), (dict(logprobs=PTR + 2), "aligned"),
])
def test_draft_accept_rejects_bad_arguments(kw, frag):
    rc, msg = err(_lib.load().hyd_draft_accept(C.byref(accept_params(**kw)), None))
    assert rc == -1 and frag in msg, (rc, msg)
    assert _lib.load().hyd_draft_accept(C.byref(accept_params(rows=0)), None) == 0  # nothing to do: no launch


# ---- register budget of the new kernels ----------------------------------------------------------------------------------------
@pytest.mark.skipif(not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")
def test_causal_instantiations_keep_the_register_budget():
    """The causal-tail instantiations live in their own source: the matrix-core kernel within 256 VGPRs (two waves per SIMD; head dim
    256: one wave, unified file) and the one-unit-per-wave kernel within 512, nothing in scratch -- the plain kernels' pins
    (tests/test_build_quality.py), which keep counting the plain instantiations alone."""
    from tests.test_build_quality import _metadata

    _, kernels = _metadata("suffix_attn_causal.hip")
    gqa = [k for k in kernels if "suffix_attn_gqa_causal_kernel" in k["name"]]
    unit = [k for k in kernels if "suffix_attn_causal_kernel" in k["name"]]
    # {f16, bf16} x ({64, 128} x {4 waves per unit, 1 / 2 / 4 kv heads per workgroup} + 256 x {1, 2 kv heads}); {f16, bf16} x ({64, 128} x R = 2 + 256 x R = 2 / 4 / 8) x {1, 4 waves}
    assert len(gqa) == 20 and len(unit) == 20 and len(kernels) == 40, [k["name"] for k in kernels]
    for k in gqa:
        d256 = "ELi256E" in k["name"]
        assert k["scratch"] == 0 and k["spill"] == 0 and k["vgpr"] <= (512 if d256 else 256), k
    for k in unit:
        assert k["scratch"] == 0 and k["spill"] == 0 and k["vgpr"] <= 512, k
    for src, pat in (("rope_append.hip", "rope_append_multi_kernel"), ("draft_lookup.hip", "draft_lookup_kernel"), ("draft_accept.hip", "draft_accept_kernel")):
        ks = [k for k in _metadata(src)[1] if pat in k["name"]]
        assert ks and all(k["scratch"] == 0 and k["spill"] == 0 and k["vgpr"] <= 128 for k in ks), ks
