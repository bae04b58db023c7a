"""-m "not gpu": scoring given tokens -- the additive C ABI (hyd_token_logprob_params, hyd_token_logprobs) and its argument
checks, the float64 definition (hydragen_amd/scoring.py) on hand-made rows, the register budget of the new kernel, the
unchanged assembly of the neighbouring kernels, and score()'s host-side argument checks."""
import ctypes as C
import hashlib
import math
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, scoring
from hydragen_amd._lib import TokenLogprobParams

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "hydragen_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
BAD, UNSUP = -1, -2  # HYD_ERR_BAD_ARG, HYD_ERR_UNSUPPORTED
NAN, NINF = float("nan"), -math.inf


def test_symbol_exported_declared_and_version_unchanged():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert "hyd_token_logprobs" in declared and "hyd_token_logprobs" in _lib.EXPORTS
    assert hasattr(lib, "hyd_token_logprobs")
    assert lib.hyd_version() == 500
    assert "#define HYD_TOP_LOGPROBS_MAX 20" in header and _lib.TOP_LOGPROBS_MAX == scoring.TOP_LOGPROBS_MAX == 20


def test_struct_size_gcc_vs_ctypes():
    fields = ["dtype", "n", "rows", "row_stride", "targets", "logprobs", "greedy", "top_n", "top_ids", "top_logprobs"]
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu'
           + " %zu" * len(fields) + '\\n", sizeof(hyd_token_logprob_params)'
           + "".join(f", offsetof(hyd_token_logprob_params, {f})" for f in fields) + ");return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got[0] == C.sizeof(TokenLogprobParams) == 80
    assert got[1:] == [getattr(TokenLogprobParams, f).offset for f in fields]


_BUF = (C.c_uint64 * 8)()  # host memory: every call below must fail before it touches a device


def _params(**kw):
    p = TokenLogprobParams()
    base = C.addressof(_BUF)
    p.logits, p.targets, p.logprobs, p.greedy = base, base, base, base
    p.dtype, p.n, p.rows, p.row_stride, p.top_n = _lib.HYD_BF16, 8, 1, 8, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code, words", [
    (dict(logits=None), BAD, "null"),
    (dict(targets=None), BAD, "null"),
    (dict(logprobs=None), BAD, "null"),
    (dict(greedy=None), BAD, "null"),
    (dict(dtype=7), UNSUP, "dtype"),
    (dict(dtype=-1), UNSUP, "dtype"),
    (dict(n=(1 << 22) + 1, row_stride=(1 << 22) + 1), UNSUP, "n"),
    (dict(n=0), BAD, "n"),
    (dict(rows=-1), BAD, "rows"),
    (dict(rows=(1 << 31) + 1), BAD, "rows"),
    (dict(top_n=21), BAD, "top_n"),
    (dict(top_n=-1), BAD, "top_n"),
    (dict(top_n=5), BAD, "top_ids"),
    (dict(top_n=5, top_ids=C.addressof(_BUF)), BAD, "top_ids"),
    (dict(top_n=5, top_logprobs=C.addressof(_BUF)), BAD, "top_ids"),
    (dict(row_stride=4), BAD, "row_stride"),
    (dict(logits=C.addressof(_BUF) + 1), BAD, "aligned"),
    (dict(targets=C.addressof(_BUF) + 4), BAD, "aligned"),
    (dict(logprobs=C.addressof(_BUF) + 2), BAD, "aligned"),
    (dict(dtype=2, logits=C.addressof(_BUF) + 2), BAD, "aligned"),
])
def test_c_entry_point_rejects_bad_arguments(kw, code, words):
    lib = _lib.load()
    assert lib.hyd_token_logprobs(C.byref(_params(**kw)), None) == code
    assert words in lib.hyd_last_error_string().decode()


def test_c_entry_point_null_params():
    assert _lib.load().hyd_token_logprobs(None, None) == BAD


def test_python_checks():
    from hydragen_amd import layer_ops

    x, t = torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64)
    for bad in (-1, 21):
        with pytest.raises(ValueError):
            layer_ops.token_logprobs(x, t, bad)
    with pytest.raises(ValueError):
        layer_ops.token_logprobs(x, t.int())
    with pytest.raises(ValueError):
        layer_ops.token_logprobs(x, t[:1])
    with pytest.raises(ValueError):
        layer_ops.token_logprobs(x.t(), t)  # not a unit last stride
    with pytest.raises(ValueError):
        layer_ops.token_logprobs(x.double(), t)
    # CPU tensors: the float64 definition
    lp, g, ids, tlp = layer_ops.token_logprobs(torch.tensor([[0.0, 1.0]]), torch.tensor([1]), 1)
    assert g.tolist() == [True] and ids.tolist() == [[1]] and abs(lp.item() - (1 - math.log(1 + math.e))) < 1e-6


def _ref(rows, targets, n=0):
    return scoring.token_logprobs_reference(torch.tensor(rows, dtype=torch.float32), torch.tensor(targets), n)


def test_reference_matches_log_softmax():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(16, 100, generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, 100, (16,), generator=g)
    lp, greedy, ids, tlp = scoring.token_logprobs_reference(x, t, 5)
    ls = torch.log_softmax(x, -1)
    assert torch.allclose(lp.double(), ls.gather(1, t[:, None])[:, 0], atol=1e-6)
    assert torch.equal(greedy, t == x.argmax(-1))
    assert torch.equal(ids, torch.topk(x, 5).indices)
    assert torch.allclose(tlp.double(), torch.topk(ls, 5).values, atol=1e-6)


def test_ties_at_the_max_go_to_the_lowest_index():
    rows = [[1.0, 3.0, 3.0, 0.0, 3.0]] * 3
    lp, greedy, ids, _ = _ref(rows, [1, 2, 4], 3)
    assert greedy.tolist() == [True, False, False]
    assert ids.tolist() == [[1, 2, 4]] * 3
    assert lp[0] == lp[1] == lp[2]


def test_ties_at_the_nth_value_prefer_the_lower_index():
    lp, _, ids, tlp = _ref([[0.0, 2.0, 1.0, 1.0, 5.0, 1.0]], [0], 3)
    assert ids.tolist() == [[4, 1, 2]]
    assert tlp[0, 0] > tlp[0, 1] > tlp[0, 2]
    _, _, ids, _ = _ref([[0.0, 2.0, 1.0, 1.0, 5.0, 1.0]], [0], 5)
    assert ids.tolist() == [[4, 1, 2, 3, 5]]


def test_nan_and_minus_inf_logits():
    rows = [[NAN, 1.0, NINF, 0.0]] * 4
    lp, greedy, ids, tlp = _ref(rows, [0, 1, 2, 3], 3)
    want1 = 1.0 - math.log(math.e + 1.0)
    assert math.isnan(lp[0]) and abs(lp[1] - want1) < 1e-6 and lp[2] == NINF and abs(lp[3] - (want1 - 1.0)) < 1e-6
    assert greedy.tolist() == [False, True, False, False]
    assert ids.tolist() == [[1, 3, -1]] * 4  # two valid logits: padded
    assert tlp[0, 2] == NINF
    # +inf is valid and is the max
    lp, greedy, _, _ = _ref([[math.inf, 1.0]], [0], 0)
    assert lp.tolist() == [0.0] and greedy.tolist() == [True]


def test_targets_out_of_range_and_rows_without_valid_logits():
    lp, greedy, ids, tlp = _ref([[1.0, 2.0], [1.0, 2.0], [NAN, NINF]], [-1, 2, 0], 2)
    assert all(math.isnan(v) for v in lp.tolist()) and not greedy.any()
    assert ids[:2].tolist() == [[1, 0], [1, 0]] and ids[2].tolist() == [-1, -1]
    assert tlp[2].tolist() == [NINF, NINF]


def test_rows_with_fewer_than_n_logits():
    _, _, ids, tlp = _ref([[0.5, 0.25, 0.75]], [0], 20)
    assert ids.shape == (1, 20) and ids[0, :3].tolist() == [2, 0, 1] and (ids[0, 3:] == -1).all()
    assert (tlp[0, 3:] == NINF).all() and torch.isfinite(tlp[0, :3]).all()


def _asm(src: str) -> str:
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                           "-Wno-unused-command-line-argument", str(CSRC / src), "-o", "-"],
                          capture_output=True, text=True, check=True).stdout


def _kernel_meta(asm: str):
    ks = []
    for blk in asm.split("  - .agpr_count:")[1:]:
        ks.append(dict(name=re.search(r"\.name:\s+(\S+)", blk).group(1),
                       vgpr=int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                       spill=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                       sspill=int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                       scratch=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
    return ks


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_token_logprob_kernel_has_no_scratch_and_keeps_its_vgpr_ceiling():
    """1024 threads per row: at most 128 VGPRs; built at 48-62 (the ceiling 64 keeps two workgroups per CU)."""
    ks = _kernel_meta(_asm("token_logprob.hip"))
    assert len(ks) == 6, ks  # f16, bf16, fp32 x (N = 0, N > 0)
    for k in ks:
        assert "token_logprob_kernel" in k["name"]
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] <= 64, k


# sha256 of the gfx950 device assembly (hipcc -S, the per-compile __hip_cuid_ symbol lines dropped) of the neighbouring
# kernels as they were before token_logprob.hip was added: the shared header changes must not move a single instruction
ASM_BEFORE = {
    "sample_filter.hip": "73438862108f935e69542f126a5684d456e090ae5cbef38734d79bec3cadd8cd",
    "layer_ops.hip": "f7040df7d15bb5ce9b6babad83128cdddc26daf758d658e8d8e332c4e128fd4c",
}
ASM_COMPILER = "roc-7.2.0 26014"  # the hipcc the hashes were taken with (its .ident line)


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(ASM_BEFORE))
def test_neighbouring_kernels_compile_to_the_same_assembly(src):
    asm = _asm(src)
    if ASM_COMPILER not in asm:
        pytest.skip(f"the recorded hashes belong to hipcc {ASM_COMPILER}")
    body = "\n".join(line for line in asm.splitlines() if "__hip_cuid_" not in line) + "\n"
    assert hashlib.sha256(body.encode()).hexdigest() == ASM_BEFORE[src]


# ---- score(): host-side argument checks, on a CPU model (they raise before any launch) -----------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig, PerLayerKVCache

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=2, vocab_size=64, max_position_embeddings=64)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.float32, device="cpu")
    for layer in m.model.layers:
        layer.self_attn.kv_cache = PerLayerKVCache(4, 16, [1, 2], [16, 8], 2, 32, "cpu", torch.float32)
    m.kv_cache_allocated = True
    return m


def _ids(b, n):
    return torch.ones((b, n), dtype=torch.long)


@pytest.mark.parametrize("kw, words", [
    (dict(input_ids=_ids(2, 5), target_lens=[0, 1]), "target_lens"),
    (dict(input_ids=_ids(2, 5), target_lens=[1, 6]), "target_lens"),
    (dict(input_ids=_ids(2, 5), target_lens=[2, 3], seq_lens=torch.tensor([5, 2])), "target_lens"),
    (dict(input_ids=_ids(2, 5), target_lens=[1]), "entries"),
    (dict(input_ids=_ids(2, 5), target_lens=[5, 1]), "no context"),
    (dict(input_ids=[_ids(1, 4), _ids(2, 5)], target_lens=[1, 1], top_logprobs=21), "top_logprobs"),
    (dict(input_ids=[_ids(1, 4), _ids(8, 5)], target_lens=[1] * 8), "batch 8"),
    (dict(input_ids=[_ids(1, 4), _ids(2, 17)], target_lens=[1, 1]), "unique cache"),
    (dict(input_ids=[_ids(1, 17), _ids(2, 5)], target_lens=[1, 1]), "shared level"),
    (dict(input_ids=[_ids(1, 16), _ids(2, 16)], target_lens=[1, 1], disable_hydragen=True), "unique cache"),
    (dict(input_ids=[_ids(1, 4), _ids(2, 4), _ids(2, 4)], target_lens=[1, 1], disable_hydragen=True), "disable_hydragen"),
    (dict(input_ids=[_ids(1, 4), _ids(2, 4), _ids(2, 4), _ids(2, 4)], target_lens=[1, 1]), "shared levels"),
])
def test_score_rejects_bad_arguments_before_any_launch(cpu_model, kw, words):
    with pytest.raises(ValueError, match=words):
        cpu_model.score(**kw)
    assert cpu_model.get_num_used_shared_caches() == 0


def test_score_rejects_positions_past_the_rotary_table(cpu_model):
    from hydragen_amd.llama import LlamaConfig

    old = cpu_model.config
    cpu_model.config = LlamaConfig(**{**old.__dict__, "max_position_embeddings": 10})
    try:
        with pytest.raises(ValueError, match="max_position_embeddings"):
            cpu_model.score([_ids(1, 8), _ids(2, 4)], [1, 1])
    finally:
        cpu_model.config = old


def test_score_first_target_needs_the_shared_level_in_this_call(cpu_model):
    from hydragen_amd.llama import SharedCacheOp

    for layer in cpu_model.model.layers:  # a level left by an earlier call (EXTEND): its logits are gone
        layer.self_attn.kv_cache.num_used_shared_caches = 1
    try:
        with pytest.raises(ValueError, match="this call"):
            cpu_model.score(_ids(2, 4), [4, 1], shared_cache_op=SharedCacheOp.EXTEND)
    finally:
        cpu_model.truncate_shared_caches(0)


def test_generate_top_logprobs_needs_return_logprobs(cpu_model):
    with pytest.raises(ValueError, match="return_logprobs"):
        cpu_model.generate(input_ids=_ids(2, 4), top_logprobs=3)
