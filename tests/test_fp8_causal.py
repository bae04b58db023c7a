"""-m "not gpu": speculative decoding on fp8 unique caches -- the host side of the two new entry points
(hyd_suffix_attn_causal_fwd_kvq, hyd_rope_append_multi_kvq) and of HYD_KVQ_CAUSAL, the build pins of the causal form of the fp8
matrix-core kernel (csrc/suffix_attn_gqa_fp8_causal.hip) and of the two new RoPE + append kernels, and the float64 reference model
with the fp8 round trip that tests/test_fp8_causal_gpu.py compares plain fp8 decoding with (tests/fp8_spec_ref.py)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib
from tests import abi_table
from tests.fp8_spec_ref import fp8_roundtrip, ref_logits64_fp8
from tests.test_build_quality import HIPCC, _device_asm, _metadata, valu_sgpr_to_vmem_hazards

REPO = Path(__file__).resolve().parent.parent
CAUSAL_SRC = "suffix_attn_gqa_fp8_causal.hip"
needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="refusals are replayed on machines without a device only")
needs_hipcc = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
GQA, CAUSAL = _lib.HYD_KVQ_GQA, _lib.HYD_KVQ_CAUSAL


def _err():
    return _lib.load().hyd_last_error_string().decode()


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbols():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    new = {"hyd_suffix_attn_causal_fwd_kvq", "hyd_rope_append_multi_kvq"}
    assert new <= declared and new <= set(_lib.EXPORTS) and all(hasattr(lib, n) for n in new)
    assert re.search(r"^#define HYD_KVQ_CAUSAL 2\s*$", header, flags=re.M) and CAUSAL == 2 and GQA == 1
    assert lib.hyd_version() == 500 and _lib.ABI_VERSION == 500
    # the bound signatures: (params, kv_quant, [qk_norm,] stream)
    assert _lib.EXPORTS["hyd_suffix_attn_causal_fwd_kvq"] == (C.c_int, [C.POINTER(_lib.SuffixParams), C.POINTER(_lib.KvQuant), C.c_void_p])
    assert _lib.EXPORTS["hyd_rope_append_multi_kvq"] == (C.c_int, [C.POINTER(_lib.RopeMultiParams), C.POINTER(_lib.KvQuant), C.c_void_p, C.c_void_p])


def test_python_faces_set_the_flag_only_for_causal_calls():
    from hydragen_amd.flash import kv_quant_params

    assert kv_quant_params(None, None).flags == GQA and kv_quant_params(None, None, causal_tail=True).flags == GQA | CAUSAL
    assert kv_quant_params(None, None, causal_tail=True).kv_dtype == _lib.HYD_FP8_E4M3


# ---- the recorded refusals, through the new entry points ------------------------------------------------------------------------
def _replay(entry, call):
    table, lib, seen = abi_table.load_fixture(), _lib.load(), 0
    for cid, e, kw in abi_table.REFUSAL_CASES:
        if e != entry:
            continue
        kw = dict(kw)
        rc = call(lib, kw.pop("null", False), kw)
        assert {"rc": rc, "error": lib.hyd_last_error_string().decode()} == table[cid], cid
        seen += 1
    return seen


@needs_no_device
def test_null_blocks_answer_what_hyd_rope_append_multi_answers():
    """Every recorded refusal of hyd_rope_append_multi through hyd_rope_append_multi_kvq(p, NULL, NULL): the code and the string --
    and with a 16-bit hyd_kv_quant (kv_dtype == the q dtype), which is no quantization, the same."""
    for kq in (None, lambda p: abi_table.kvq(kv_dtype=p.dtype)):
        def call(lib, null, kw):
            p = None if null else abi_table.rope_multi(**kw)
            k = None if kq is None or p is None else C.byref(kq(p))
            return lib.hyd_rope_append_multi_kvq(None if p is None else C.byref(p), k, None, None)
        assert _replay("hyd_rope_append_multi", call) > 30


@needs_no_device
def test_null_block_answers_what_hyd_suffix_attn_causal_fwd_answers():
    def call(lib, null, kw):
        return lib.hyd_suffix_attn_causal_fwd_kvq(None if null else C.byref(abi_table.suffix(**{"nq": 2, **kw})), None, None)
    assert _replay("hyd_suffix_attn_causal_fwd", call) > 40


@needs_no_device
def test_decode_call_without_the_flag_keeps_its_recorded_answer():
    """hyd_decode_attn_fused_kvq with flags = 1 (HYD_KVQ_GQA alone) and causal_tail = 1: the five records of tests/golden/abi_table.json
    (four on shapes the fp8 kernels take, one on 2-row units, which they do not; the table also has such calls under other flags)."""
    table, lib, seen = abi_table.load_fixture(), _lib.load(), 0
    for case in abi_table.REFUSAL_CASES:
        cid, entry, kw = case
        if entry == "hyd_decode_attn_fused_kvq" and kw.get("causal_tail") == 1 and kw["kq"] == dict(flags=1):
            assert abi_table.run_case(case) == table[cid], cid
            seen += 1
    assert seen == 5
    d = abi_table.decode(ptrs=True, nq=2, Hq=32, causal_tail=1)
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(abi_table.kvq(flags=GQA)), None) == -2 and "16-bit caches only" in _err()
    s = abi_table.suffix(nq=2, Hq=32)
    assert lib.hyd_suffix_attn_causal_fwd_kvq(C.byref(s), C.byref(abi_table.kvq(flags=GQA)), None) == -2 and "16-bit caches only" in _err()


# ---- valid and invalid fp8 calls ---------------------------------------------------------------------------------------------------
FLAGS3 = dict(flags=GQA | CAUSAL, k_scale=abi_table.PTR, v_scale=abi_table.PTR)


@needs_no_device
def test_valid_fp8_calls_end_at_the_launch():
    """Without a device a call that passes every check ends at the launch: HYD_ERR_LAUNCH, never a refusal."""
    lib = _lib.load()
    for shape in (dict(nq=3, Hq=8, Hkv=2, D=128), dict(nq=2, Hq=4, Hkv=4, D=64), dict(nq=8, Hq=8, Hkv=1, D=256, dtype=0), dict(nq=5, Hq=6, Hkv=2, D=64, kv_len=132)):
        s = abi_table.suffix(**shape)
        for kq in (abi_table.kvq(**FLAGS3), abi_table.kvq(flags=GQA | CAUSAL), abi_table.kvq(flags=CAUSAL)):  # (null scales = 1)
            assert lib.hyd_suffix_attn_causal_fwd_kvq(C.byref(s), C.byref(kq), None) == abi_table.HYD_ERR_LAUNCH, (shape, _err())
    d = abi_table.decode(ptrs=True, nq=3, Hq=8, Hkv=2, causal_tail=1, phase=_lib.HYD_PHASE_UNIQUE)  # (the unique phase launches the suffix kernel first)
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(abi_table.kvq(**FLAGS3)), None) == abi_table.HYD_ERR_LAUNCH, _err()
    for p in (abi_table.rope_multi(), abi_table.rope_multi(D=64, T=8, dtype=0), abi_table.rope_multi(D=256, T=3)):
        for kq in (abi_table.kvq(k_scale=abi_table.PTR, v_scale=abi_table.PTR), abi_table.kvq(), abi_table.kvq(flags=GQA | CAUSAL)):
            for qn in (None, C.byref(_qn())):
                assert lib.hyd_rope_append_multi_kvq(C.byref(p), C.byref(kq), qn, None) == abi_table.HYD_ERR_LAUNCH, _err()


def _qn():
    from hydragen_amd.fused_decode import QkNorm

    return QkNorm(abi_table.PTR, abi_table.PTR, 1e-6, 0)


@needs_no_device
def test_bad_kv_quant_blocks_are_refused_as_the_one_token_preamble_refuses_them():
    lib = _lib.load()
    cases = [(dict(kv_dtype=7), -2, "kv_dtype 7"), (dict(k_scale=abi_table.PTR + 2), -1, "4-byte aligned"), (dict(v_scale=abi_table.ODD), -1, "4-byte aligned")]
    for kw, code, frag in cases:
        want = (lib.hyd_rope_append_decode_kvq(C.byref(abi_table.rope()), C.byref(abi_table.kvq(**kw)), None), _err())
        assert want[0] == code and frag in want[1]
        assert (lib.hyd_rope_append_multi_kvq(C.byref(abi_table.rope_multi()), C.byref(abi_table.kvq(**kw)), None, None), _err()) == want
        kq = abi_table.kvq(**{"flags": GQA | CAUSAL, **kw})
        assert (lib.hyd_suffix_attn_causal_fwd_kvq(C.byref(abi_table.suffix(nq=3, Hq=8, Hkv=2)), C.byref(kq), None), _err()) == want
    # the multi-token form's own checks come in their order around it: T first, the cache strides (bytes, still multiples of 8) behind
    assert lib.hyd_rope_append_multi_kvq(C.byref(abi_table.rope_multi(T=9)), C.byref(abi_table.kvq(kv_dtype=7)), None, None) == -1 and "T = 9" in _err()
    assert lib.hyd_rope_append_multi_kvq(C.byref(abi_table.rope_multi(kc_tok_stride=4)), C.byref(abi_table.kvq()), None, None) == -1 and "kc_tok_stride" in _err()


@needs_no_device
def test_causal_shapes_no_fp8_kernel_takes_are_unsupported():
    """With the flag, a shape outside the fp8 causal kernel's is HYD_ERR_UNSUPPORTED before any launch -- in every phase of the decode call."""
    lib = _lib.load()
    kq = abi_table.kvq(**FLAGS3)
    few256 = dict(B=1, nq=2, Hq=4, Hkv=4, D=256, kv_len=132)
    assert lib.hyd_suffix_attn_causal_fwd_kvq(C.byref(abi_table.suffix(**few256)), C.byref(kq), None) == -2 and "per-row key limit" in _err()
    assert lib.hyd_suffix_attn_causal_fwd_kvq(C.byref(abi_table.suffix(nq=3, Hq=8, Hkv=2, kv_dim=96)), C.byref(kq), None) == -2 and "kv_dim 96" in _err()
    assert lib.hyd_suffix_attn_causal_fwd_kvq(C.byref(abi_table.suffix(nq=9, Hq=8, Hkv=2)), C.byref(kq), None) == -1 and "2 to 8" in _err()
    for phase in range(5):
        d = abi_table.decode(ptrs=True, causal_tail=1, phase=phase, **few256)
        assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(kq), None) == -2 and "per-row key limit" in _err(), phase
    d = abi_table.decode(ptrs=True, causal_tail=2, nq=3, Hq=8, Hkv=2)
    assert lib.hyd_decode_attn_fused_kvq(C.byref(d), C.byref(kq), None) == -1 and "causal_tail 2" in _err()


def test_decode_support_query_for_causal_calls():
    """Shapes only, so it runs with and without a device: (flags, shape) -> answer."""
    lib = _lib.load()
    shapes = [(dict(nq=3, Hq=8, Hkv=2, D=128), 1),                       # 12-row grouped-query units
              (dict(nq=2, Hq=4, Hkv=4, D=64), 1),                        # 2-row units: the matrix cores take them too (no fp8 one-unit kernel)
              (dict(B=1, nq=2, Hq=4, Hkv=4, D=256, kv_len=132), 0),      # head dim 256 with few units
              (dict(nq=3, Hq=8, Hkv=2, D=128, **{"suffix.kv_dim": 96}), 0)]
    for kw, want in shapes:
        for single in (0, 1):
            d = abi_table.decode(causal_tail=1, single_launch_small=single, **kw)
            assert lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(abi_table.kvq(flags=GQA | CAUSAL))) == want, kw
            assert lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(abi_table.kvq(flags=GQA))) == 0, kw  # the call is refused without the flag
            assert lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(abi_table.kvq(flags=0))) == 0, kw
            assert lib.hyd_decode_kv_quant_supported(C.byref(d), None) == 1
    for nq in (1, 9):
        d = abi_table.decode(causal_tail=1, nq=nq, Hq=8, Hkv=2)
        assert lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(abi_table.kvq(flags=GQA | CAUSAL))) == 0
    # without causal_tail the flag changes no answer
    for kw in (dict(nq=3, Hq=8, Hkv=2), dict(nq=2, Hq=4, Hkv=4, D=64), dict(nq=1, Hq=8, Hkv=8)):
        d = abi_table.decode(**kw)
        assert lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(abi_table.kvq(flags=GQA | CAUSAL))) == \
            lib.hyd_decode_kv_quant_supported(C.byref(d), C.byref(abi_table.kvq(flags=GQA)))


# ---- build pins --------------------------------------------------------------------------------------------------------------------
@needs_hipcc
def test_fp8_causal_kernels_registers():
    _, kernels = _metadata(CAUSAL_SRC)
    # {f16, bf16} x ({64, 128} x ({4 waves per unit} + {1, 2, 4 kv heads per workgroup}) + 256 x {1, 2 kv heads per workgroup})
    assert len(kernels) == 20, [k["name"] for k in kernels]
    geo = set()
    for k in kernels:
        assert "suffix_attn_gqa_fp8_causal_kernel" in k["name"]
        assert k["spill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
        d256 = "ELi256E" in k["name"]
        assert k["vgpr"] <= (512 if d256 else 256), k  # (D = 256: one wave per SIMD, the unified count)
        geo.add(re.search(r"ELi(64|128|256)ELi(\d)ELi(\d)E", k["name"]).groups())
    assert geo == {(d, w, h) for d in ("64", "128") for w, h in (("4", "1"), ("1", "1"), ("1", "2"), ("1", "4"))} | {("256", "1", "1"), ("256", "1", "2")}


@needs_hipcc
def test_fp8_causal_stream_has_only_the_hand_placed_waits():
    """Between the first and the last LDS-DMA hipcc adds no counted vector-memory wait of its own (it cannot see the DMAs): the only
    counted one is the hand-placed wait of the two-set scheme at D <= 128, which leaves the younger step's 2 * D / 32 requests out."""
    seen = 0
    for m in re.finditer(r"^(_ZN3hyd\d+suffix_attn_gqa_fp8_causal_kernel\w+):(.*?)^\.Lfunc_end", _device_asm(CAUSAL_SRC), flags=re.S | re.M):
        seen += 1
        body = m.group(2)
        first_dma = body.find(" lds")
        assert first_dma > 0, m.group(1)
        lines = body[first_dma:].splitlines()
        last_dma = max(i for i, ln in enumerate(lines) if ln.rstrip().endswith(" lds") or " lds " in ln)
        counted = [ln.strip() for ln in lines[:last_dma] if re.search(r"s_waitcnt vmcnt\((?!0\))", ln)]
        d = int(re.search(r"ELi(64|128|256)E", m.group(1)).group(1))
        if d <= 128:
            assert f"s_waitcnt vmcnt({2 * d // 32})" in counted, m.group(1)  # (the hand-placed one is there)
            counted = [ln for ln in counted if ln != f"s_waitcnt vmcnt({2 * d // 32})"]
        assert not counted, (m.group(1), counted[:3])
    assert seen == 20


@needs_hipcc
def test_fp8_causal_dma_keeps_its_distance_from_valu_written_scalars():
    bad = valu_sgpr_to_vmem_hazards(_device_asm(CAUSAL_SRC))
    assert not bad, f"{len(bad)} hazards, first: {bad[:3]}"


@needs_hipcc
def test_plain_fp8_kernel_file_still_holds_its_twenty_kernels_and_no_causal_one():
    names = [k["name"] for k in _metadata("suffix_attn_gqa_fp8.hip")[1]]
    assert len(names) == 20 and all("suffix_attn_gqa_fp8_kernel" in n for n in names)


@needs_hipcc
def test_multi_token_fp8_rope_kernels_registers():
    kernels = {k["name"]: k for k in _metadata("rope_append.hip")[1]}
    for stem in ("rope_append_multi_fp8_kernel", "rope_append_norm_multi_fp8_kernel"):
        mine = [k for n, k in kernels.items() if re.search(rf"\d+{stem}I", n)]
        assert len(mine) == 6, (stem, sorted(kernels))  # {f16, bf16} x {64, 128, 256}
        for k in mine:
            assert k["vgpr"] <= 128 and k["scratch"] == 0 and k["spill"] == 0, k


# ---- the float64 model with the fp8 round trip -----------------------------------------------------------------------------------
def test_roundtrip_is_the_unit_scale_cache():
    x = torch.tensor([0.0, 1.0, -1.0, 0.3, 447.0, 500.0, -1e4, 2.0 ** -9, 2.0 ** -11, 1.0625, 1.1875], dtype=torch.float64)
    want = torch.tensor([0.0, 1.0, -1.0, 0.3125, 448.0, 448.0, -448.0, 2.0 ** -9, 0.0, 1.0, 1.25], dtype=torch.float64)
    assert torch.equal(fp8_roundtrip(x), want)  # (ties to even: 1.0625 -> 1, 1.1875 -> 1.25; the clamp; the flush below 2^-10)


def test_reference_without_the_round_trip_is_the_16_bit_reference():
    from tests.test_speculative_gpu import PROMPT, cpu_model, cpu_prompts, ref_logits64

    model = cpu_model(4, 4, 3)
    ids = torch.cat([cpu_prompts(3), torch.randint(1, 512, (2, 5), generator=torch.Generator().manual_seed(4))], 1)
    want = ref_logits64(model, ids)
    assert torch.equal(ref_logits64_fp8(model, ids, PROMPT, roundtrip=False), want)
    got = ref_logits64_fp8(model, ids, PROMPT)
    # the prompt's own positions read no quantized key; the generated ones do (position PROMPT reads its own key and value)
    assert torch.equal(got[:, :PROMPT], want[:, :PROMPT]) and not torch.equal(got[:, PROMPT:], want[:, PROMPT:])
    assert float((got - want).abs().max()) < 0.1
    assert torch.equal(ref_logits64_fp8(model, ids, ids.shape[1]), want)
