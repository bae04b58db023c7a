"""-m "not gpu": top-k / top-p / min-p sampling -- the additive C ABI (hyd_sample_filter_params, hyd_sample_tokens_filtered)
and its argument checks, the torch definition of the cuts (hydragen_amd/sampling.py) against the reference's apply_top_p,
HF's top-k tie rule and hand-worked rows, and the register budget of the new kernel."""
import ctypes as C
import math
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, sampling
from hydragen_amd._lib import SampleFilterParams

REPO = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"
BAD, UNSUP = -1, -2  # HYD_ERR_BAD_ARG, HYD_ERR_UNSUPPORTED


def test_symbol_exported_declared_and_version_unchanged():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert "hyd_sample_tokens_filtered" in declared and "hyd_sample_tokens_filtered" in _lib.EXPORTS
    assert hasattr(lib, "hyd_sample_tokens_filtered")
    assert lib.hyd_version() == 500
    assert "#define HYD_SAMPLE_FILTER_MAX_N (1 << 22)" in header and _lib.SAMPLE_FILTER_MAX_N == 1 << 22


def test_struct_size_gcc_vs_ctypes():
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n",'
           'sizeof(hyd_sample_filter_params), offsetof(hyd_sample_filter_params, top_k), offsetof(hyd_sample_filter_params, min_p),'
           'sizeof(hyd_sample_params));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        size, off_k, off_minp, old = map(int, subprocess.check_output([str(Path(d) / "s")]).split())
    assert size == C.sizeof(SampleFilterParams) == 88
    assert off_k == SampleFilterParams.top_k.offset and off_minp == SampleFilterParams.min_p.offset
    assert old == 56  # hyd_sample_params is untouched


_BUF = (C.c_uint64 * 8)()  # host memory: every call below must fail before it touches a device


def _params(**kw):
    p = SampleFilterParams()
    base = C.addressof(_BUF)
    p.logits, p.out, p.logprobs, p.kept = base, base, None, None
    p.row_stride, p.rows, p.n, p.dtype = 8, 1, 8, _lib.HYD_BF16
    p.temperature, p.top_k, p.top_p, p.min_p = 1.0, 0, 1.0, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code, words", [
    (dict(logits=None), BAD, "null"),
    (dict(out=None), BAD, "null"),
    (dict(dtype=7), UNSUP, "dtype"),
    (dict(top_k=-1), BAD, "top_k"),
    (dict(top_p=0.0), BAD, "top_p"),
    (dict(top_p=1.5), BAD, "top_p"),
    (dict(top_p=float("nan")), BAD, "top_p"),
    (dict(min_p=-0.1), BAD, "min_p"),
    (dict(min_p=2.0), BAD, "min_p"),
    (dict(min_p=float("nan")), BAD, "min_p"),
    (dict(temperature=-1.0), BAD, "temperature"),
    (dict(n=(1 << 22) + 1, row_stride=(1 << 22) + 1), UNSUP, "n"),
    (dict(n=0), BAD, "n"),
    (dict(row_stride=4), BAD, "row_stride"),
    (dict(logits=C.addressof(_BUF) + 1), BAD, "aligned"),
    (dict(out=C.addressof(_BUF) + 4), BAD, "aligned"),
    (dict(logprobs=C.addressof(_BUF) + 2), BAD, "aligned"),
    (dict(kept=C.addressof(_BUF) + 1), BAD, "aligned"),
    (dict(dtype=2, logits=C.addressof(_BUF) + 2), BAD, "aligned"),
])
def test_c_entry_point_rejects_bad_arguments(kw, code, words):
    lib = _lib.load()
    assert lib.hyd_sample_tokens_filtered(C.byref(_params(**kw)), None) == code
    assert words in lib.hyd_last_error_string().decode()


def test_c_entry_point_null_params():
    lib = _lib.load()
    assert lib.hyd_sample_tokens_filtered(None, None) == BAD


def test_python_checks():
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=2.0)):
        with pytest.raises(ValueError):
            sampling.kept_mask(torch.zeros(1, 4), **kw)
    assert not sampling.filters_active(None, None, None)
    assert not sampling.filters_active(0, 1.0, 0.0)
    assert sampling.filters_active(5, None, None) and sampling.filters_active(None, 0.9, None)
    assert sampling.filters_active(None, None, 0.1)


def reference_apply_top_p(logits, top_p, min_tokens_to_keep=1):
    """The reference's apply_top_p (hydragen llama.py, modified from HF TopPLogitsWarper), restated: the removal mask."""
    sorted_logits, sorted_indices = torch.sort(logits, descending=False)
    cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    remove = cumulative_probs <= (1 - top_p)
    remove[..., -min_tokens_to_keep:] = 0
    return remove.scatter(1, sorted_indices, remove)


@pytest.mark.parametrize("top_p", [0.1, 0.5, 0.9, 0.95, 0.999])
def test_top_p_matches_the_reference_on_distinct_logits(top_p):
    g = torch.Generator().manual_seed(int(top_p * 1000))
    x = torch.randn(64, 1000, generator=g, dtype=torch.float64) * 3
    keep = sampling.kept_mask(x, top_p=top_p)
    ref = ~reference_apply_top_p(x, top_p)
    # rows whose boundary sits within 1e-9 of the threshold could go either way in float64 sums: none at these seeds
    assert torch.equal(keep, ref)
    assert (keep.sum(-1) >= 1).all()


def test_top_p_keeps_every_tie_at_the_boundary():
    # masses 0.4 | 0.2 0.2 0.2 (tied) : top_p 0.5 is crossed inside the tie group -> the whole group stays
    x = torch.log(torch.tensor([[0.2, 0.4, 0.2, 0.2]], dtype=torch.float64))
    assert sampling.kept_mask(x, top_p=0.5).tolist() == [[True, True, True, True]]
    assert sampling.kept_mask(x, top_p=0.4).tolist() == [[False, True, False, False]]
    # the reference keeps only the tied tokens that torch.sort happens to place last
    assert int((~reference_apply_top_p(x, 0.5)).sum()) < 4


def test_top_k_keeps_ties_like_hf():
    x = torch.tensor([[1.0, 3.0, 2.0, 2.0, 0.0, 2.0]])
    # HF TopKLogitsWarper: remove logits < the k-th largest value
    for k in range(1, 7):
        kth = torch.topk(x, k).values[..., -1:]
        assert torch.equal(sampling.kept_mask(x, top_k=k), x >= kth)
    assert sampling.kept_mask(x, top_k=2).tolist() == [[False, True, True, True, False, True]]
    assert sampling.kept_mask(x, top_k=100).all()


def test_min_p_against_the_probability_ratio():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(32, 500, generator=g, dtype=torch.float64) * 2
    p = torch.softmax(x, -1)
    for mp in (0.01, 0.1, 0.5, 1.0):
        want = p >= mp * p.amax(-1, keepdim=True) * (1 - 1e-12)
        assert torch.equal(sampling.kept_mask(x, min_p=mp), want)


def test_top_k_then_top_p_renormalises_hand_worked():
    # probabilities 0.5, 0.2, 0.15, 0.1, 0.05; top-k 3 keeps 0.5 0.2 0.15 (mass 0.85): renormalised 0.588 0.235 0.176
    x = torch.log(torch.tensor([[0.1, 0.5, 0.05, 0.2, 0.15]], dtype=torch.float64))
    assert sampling.kept_mask(x, top_k=3).tolist() == [[False, True, False, True, True]]
    # top-p 0.8 of the survivors: 0.588 < 0.8 <= 0.823 -> two tokens (over the whole row 0.5 + 0.2 = 0.7 < 0.8: three)
    assert sampling.kept_mask(x, top_k=3, top_p=0.8).tolist() == [[False, True, False, True, False]]
    assert sampling.kept_mask(x, top_p=0.8).tolist() == [[False, True, False, True, True]]
    # min-p 0.35: p >= 0.175 -> 0.5 and 0.2, whatever the other cuts
    assert sampling.kept_mask(x, min_p=0.35).tolist() == [[False, True, False, True, False]]
    assert sampling.kept_mask(x, top_k=3, top_p=0.99, min_p=0.35).tolist() == [[False, True, False, True, False]]


def test_non_finite_logits_are_never_kept():
    x = torch.tensor([[float("nan"), 1.0, -math.inf, 0.5], [-math.inf] * 4])
    assert sampling.kept_mask(x).tolist() == [[False, True, False, True], [False] * 4]
    assert sampling.kept_mask(x, top_k=3, top_p=0.99).tolist() == [[False, True, False, True], [False] * 4]
    f = sampling.filter_logits(x, top_k=1)
    assert f.dtype == x.dtype and f[0].tolist() == [-math.inf, 1.0, -math.inf, -math.inf]


def _kernel_meta():
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                          str(REPO / "hydragen_amd" / "csrc" / "sample_filter.hip"), "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    ks = []
    for blk in out.split("  - .agpr_count:")[1:]:
        ks.append(dict(name=re.search(r"\.name:\s+(\S+)", blk).group(1),
                       vgpr=int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                       spill=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                       sspill=int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                       scratch=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
    return ks


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_sample_filter_kernel_has_no_scratch_and_keeps_its_vgpr_ceiling():
    """1024 threads per row = 4 waves per SIMD: at most 128 VGPRs; the kernel was built at 46 (ceiling 64 keeps two
    workgroups per CU)."""
    ks = _kernel_meta()
    assert len(ks) == 3, ks  # f16, bf16, fp32
    for k in ks:
        assert "sample_filter_kernel" in k["name"]
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] <= 64, k
