"""-m "not gpu": stop conditions decided on the device -- the additive C ABI (hyd_stop_params, hyd_stop_update), its argument
validation (no launch), the two torch definitions of hydragen_amd/stopping.py held against each other, generate()'s refusals and
the new kernel's register budget."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import pytest
import torch

from hydragen_amd import _lib, stopping
from hydragen_amd._lib import StopParams
from tests import stop_cases

REPO = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"


def test_symbol_declared_exported_and_version_stays():
    lib = _lib.load()
    header = (REPO / "include" / "hydragen_hip.h").read_text()
    declared = set(re.findall(r"\b(hyd_[a-z_0-9]+)\s*\(", header))
    assert "hyd_stop_update" in declared and "hyd_stop_update" in _lib.EXPORTS and hasattr(lib, "hyd_stop_update")
    assert lib.hyd_version() == 500 == _lib.ABI_VERSION
    for name, val in (("HYD_STOP_MAX_EOS", 16), ("HYD_STOP_MAX_SEQS", 32), ("HYD_STOP_MAX_LEN", 16)):
        assert re.search(rf"#define {name} {val}\b", header)
    assert (_lib.STOP_MAX_EOS, _lib.STOP_MAX_SEQS, _lib.STOP_MAX_LEN) == (16, 32, 16) == (stopping.MAX_EOS, stopping.MAX_SEQS, stopping.MAX_LEN)
    # the contract the retirement of finished rows relies on is written down at the RoPE + append entry point
    doc = header[header.index("Decode-step preamble"):header.index("typedef struct hyd_rope_params")]
    assert "writes no K/V" in doc and "seq_lens[b] = 0" in doc and "may rely on it" in doc


def test_struct_size_gcc_vs_ctypes():
    src = ('#include "hydragen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(hyd_stop_params),'
           'offsetof(hyd_stop_params, eos), offsetof(hyd_stop_params, stop_lens), offsetof(hyd_stop_params, retire));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(REPO / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        got = list(map(int, subprocess.check_output([str(Path(d) / "s")]).split()))
    assert got == [C.sizeof(StopParams), StopParams.eos.offset, StopParams.stop_lens.offset, StopParams.retire.offset]
    assert got[0] == 384


PTR = 0x10000  # never dereferenced: validation fails first


def _params(**kw):
    p = StopParams()
    for f in ("tok", "out", "length", "reason", "stop_index", "live", "stop_tokens", "start_pos", "shared_len", "feed", "next_pos"):
        setattr(p, f, PTR)
    p.out_stride, p.rows, p.t, p.n_eos, p.n_stop = 32, 4, 3, 1, 2
    p.stop_lens[0], p.stop_lens[1] = 1, 16
    for k, v in kw.items():
        if k.startswith("stop_lens_"):
            p.stop_lens[int(k[10:])] = v
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, frag", [
    (dict(tok=None), "null"), (dict(out=None), "null"), (dict(length=None), "null"), (dict(reason=None), "null"),
    (dict(stop_index=None), "null"), (dict(live=None), "null"), (dict(start_pos=None), "null"), (dict(feed=None), "null"),
    (dict(next_pos=None), "null"), (dict(stop_tokens=None), "stop_tokens"),
    (dict(rows=-1), "rows"), (dict(n_eos=-1), "n_eos"), (dict(n_eos=17), "n_eos"), (dict(n_stop=-1), "n_stop"), (dict(n_stop=33), "n_stop"),
    (dict(stop_lens_0=0), "stop_lens[0]"), (dict(stop_lens_1=17), "stop_lens[1]"), (dict(stop_lens_1=-3), "stop_lens[1]"),
    (dict(t=-1), "t -1"), (dict(t=32), "t 32"), (dict(out_stride=0), "out_stride"),
    (dict(tok=PTR + 4), "aligned"), (dict(out=PTR + 4), "aligned"), (dict(feed=PTR + 2), "aligned"), (dict(next_pos=PTR + 4), "aligned"),
    (dict(stop_tokens=PTR + 4), "aligned"), (dict(start_pos=PTR + 1), "aligned"), (dict(shared_len=PTR + 4), "aligned"),
    (dict(length=PTR + 2), "aligned"), (dict(reason=PTR + 1), "aligned"), (dict(stop_index=PTR + 2), "aligned"), (dict(live=PTR + 3), "aligned"),
])
def test_bad_arguments_are_refused_without_a_launch(kw, frag):
    lib = _lib.load()
    assert lib.hyd_stop_update(C.byref(_params(**kw)), None) == -1
    assert frag in lib.hyd_last_error_string().decode()
    with pytest.raises(ValueError):
        _lib.check(-1)


def test_null_params_and_empty_batch():
    lib = _lib.load()
    assert lib.hyd_stop_update(None, None) == -1
    # rows == 0: success, nothing launched (the dummy pointers would fault); a stop length past n_stop is not looked at
    assert lib.hyd_stop_update(C.byref(_params(rows=0, stop_lens_5=99)), None) == 0
    assert lib.hyd_stop_update(C.byref(_params(rows=0, shared_len=None, n_stop=0, stop_tokens=None, n_eos=0)), None) == 0
    # ... but every other argument is still checked
    assert lib.hyd_stop_update(C.byref(_params(rows=0, t=40)), None) == -1


def test_check_stop_limits_and_normalisation():
    s = stopping.check_stop(7, [[1, 2], torch.tensor([3]), (4, 5, 6)], None, False, 10)
    assert s == stopping.StopSpec((7,), ((1, 2), (3,), (4, 5, 6)), 7, False)
    assert stopping.check_stop(None, None).pad == 0 and stopping.check_stop([3, 2], None).pad == 3
    assert stopping.check_stop([3], None, 1, True, 5) == stopping.StopSpec((3,), (), 1, True)
    tab, lens = s.stop_table()
    assert tab.shape == (3, 16) and tab.dtype == torch.int64 and lens == [2, 1, 3] and tab[2, :4].tolist() == [4, 5, 6, 0]
    for bad in (dict(eos_token_id=list(range(17))), dict(stop=[[1]] * 33), dict(stop=[[]]), dict(stop=[[1] * 17]), dict(stop="\n\n"),
                dict(stop=[[1.5]]), dict(eos_token_id=[True]), dict(pad_token_id=10, vocab_size=10), dict(pad_token_id=-1),
                dict(eos_token_id=[10], vocab_size=10), dict(stop=[[1, 10]], vocab_size=10), dict(stop=[torch.zeros(2, 2, dtype=torch.long)])):
        with pytest.raises(ValueError):
            stopping.check_stop(**bad)


def _run_steps(tok, spec, retire=True, shared_len=None):
    rows, steps = tok.shape
    state = stopping.new_state(rows, steps, spec)
    start = torch.arange(rows) * 3 + 100
    feeds, poss = [], []
    for t in range(steps):
        f, p = stopping.stop_update_reference(tok[:, t], t, spec, *state, start, shared_len, retire)
        feeds.append(f)
        poss.append(p)
    return state, torch.stack(feeds, 1), torch.stack(poss, 1), start


def _can_finish_a_row(k, eos, stops, steps):
    """Whether stop sequence k can be what finishes a row, from the rules alone: it fits into the generated columns, holds no
    EOS id (rule b comes first, and an earlier EOS finishes the row before k completes), no other stop sequence completes
    inside it before its last token, and no stop sequence with a lower index completes on its last token."""
    s = stops[k]
    if len(s) > steps or any(e in s for e in eos):
        return False
    for j, o in enumerate(stops):
        for end in range(len(o), len(s) + 1):
            if j != k and s[end - len(o) : end] == o and (end < len(s) or j < k):
                return False
    return True


@pytest.mark.parametrize("include_stop", [False, True])
@pytest.mark.parametrize("pad", [stop_cases.SAFE, 1])
@pytest.mark.parametrize("name", sorted(stop_cases.CASES))
def test_step_definition_equals_scan_definition(name, include_stop, pad):
    spec = stop_cases.spec(name, include_stop, pad)
    tok = stop_cases.tokens(name, 200)
    (out, length, reason, index, live), feed, pos, start = _run_steps(tok, spec)
    w_out, w_len, w_reason, w_index = stopping.truncate_reference(tok, spec)
    assert torch.equal(out, w_out) and torch.equal(length, w_len) and torch.equal(reason, w_reason) and torch.equal(index, w_index)
    assert torch.equal(live, stopping.live_reference(tok, spec))
    # the inputs really exercise the rules: every reason code, a row that never finishes, every EOS id and every stop sequence that
    # can finish a row at all (the 16-token stop cannot fit; a stop that holds an EOS id or a complete other stop never gets its turn)
    assert set(reason.tolist()) == {0, 1, 2}
    assert length[reason == 0].eq(tok.shape[1]).all()
    eos, stops, _ = stop_cases.CASES[name]
    assert set(index[reason == 1].tolist()) == set(range(len(eos)))
    assert set(index[reason == 2].tolist()) == {k for k in range(len(stops)) if _can_finish_a_row(k, eos, stops, tok.shape[1])}
    # the feed follows the rules: the token while running, pad afterwards; positions advance or retire
    step, _, _ = stopping.finish_steps(tok, spec)
    running = torch.arange(tok.shape[1])[None, :] < step[:, None]
    assert torch.equal(feed, torch.where(running, tok, torch.full_like(tok, pad)))
    assert torch.equal(pos, torch.where(running, start[:, None] + torch.arange(tok.shape[1])[None, :], torch.full_like(tok, -1)))


def test_planted_rows_finish_as_the_rules_say():
    def run(name, include_stop=False):
        spec = stop_cases.spec(name, include_stop)
        tok = stop_cases.tokens(name, 16)
        n = len(stop_cases.CASES[name][2])
        _, length, reason, index = stopping.truncate_reference(tok, spec)
        rows = [15 - i for i in range(n + 1)]  # the planted rows, then the all-SAFE row
        return [(int(length[r]), int(reason[r]), int(index[r])) for r in rows]

    T = stop_cases.T
    # 5 1 2 1 2 5: 1 2 1 completes at step 3; 5 2 1 2 1 5: 2 1 2 completes at step 3; 1 2 5 1 2 1: step 5
    assert run("overlapping") == [(1, 2, 0), (1, 2, 1), (3, 2, 0), (T, 0, -1)]
    assert run("overlapping", True) == [(4, 2, 0), (4, 2, 1), (6, 2, 0), (T, 0, -1)]
    # 1 2 completes before 1 2 3 can, whatever the list order
    assert run("prefix-long-first") == [(1, 2, 1), (0, 2, 1), (T, 0, -1)]
    assert run("prefix-short-first") == [(1, 2, 0), (0, 2, 0), (T, 0, -1)]
    # 1 2 3 at the very start is not the tail of 0 1 2 3; sixteen 3s cannot fit in 14 steps
    assert run("longer-than-generated") == [(5, 2, 0), (T, 0, -1), (T, 0, -1), (T, 0, -1)]
    # 2 3 ends in the EOS id 3: EOS, kept; 4 is EOS id 1 and stop 1: EOS; 1 1: a stop
    assert run("eos-and-stop-together") == [(3, 1, 0), (2, 1, 1), (1, 2, 2), (T, 0, -1)]
    assert run("eos-and-stop-together", True) == [(3, 1, 0), (2, 1, 1), (3, 2, 2), (T, 0, -1)]
    # 5 0 2 1: stops 0, 1, 2 complete together -> 0 (cutting 2 tokens); 0 2 1 at the start: the same; 5 5 1: only stop 1
    assert run("lowest-k") == [(2, 2, 0), (1, 2, 0), (2, 2, 1), (T, 0, -1)]
    assert run("many-eos") == [(3, 1, 1), (1, 1, 0), (1, 2, 0), (T, 0, -1)]


def test_no_condition_never_finishes_and_retire_off_keeps_positions():
    tok = stop_cases.tokens("lowest-k", 40)
    spec = stopping.check_stop(None, None, 2)
    out, length, reason, index = stopping.truncate_reference(tok, spec)
    assert torch.equal(out, tok) and length.eq(tok.shape[1]).all() and reason.eq(0).all() and index.eq(-1).all()
    (o2, *_), feed, pos, start = _run_steps(tok, spec)
    assert torch.equal(o2, tok) and torch.equal(feed, tok)
    # EOS ids only, more of them than there are stop sequences (the EOS index is no index into the stop list)
    spec = stopping.check_stop([0, 1, 2, 3, 4], None, 5)
    (o3, l3, r3, i3, _), _, _, _ = _run_steps(tok, spec)
    w3 = stopping.truncate_reference(tok, spec)
    assert torch.equal(o3, w3[0]) and torch.equal(l3, w3[1]) and torch.equal(r3, w3[2]) and torch.equal(i3, w3[3])
    assert set(i3.tolist()) >= {0, 1, 2, 3, 4} and set(r3.tolist()) == {0, 1}
    # retire off: every row keeps advancing; retire on with shared lengths: finished rows sit at shared_len - 1
    spec = stop_cases.spec("lowest-k", False)
    shared = torch.arange(40) + 7
    _, _, pos_off, start = _run_steps(tok, spec, retire=False, shared_len=shared)
    assert torch.equal(pos_off, start[:, None] + torch.arange(tok.shape[1])[None, :])
    _, _, pos_on, _ = _run_steps(tok, spec, retire=True, shared_len=shared)
    step, _, _ = stopping.finish_steps(tok, spec)
    done = torch.arange(tok.shape[1])[None, :] >= step[:, None]
    assert done.any() and torch.equal(pos_on[done], (shared[:, None] - 1).expand_as(pos_on)[done]) and torch.equal(pos_on[~done], pos_off[~done])


def test_generate_refuses_what_the_kernel_cannot_do():
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
                      vocab_size=32, max_position_embeddings=64)
    model = HydragenLlamaForCausalLM(cfg)
    model.kv_cache_allocated = True  # (the refusals come before any cache is touched)
    ids = torch.zeros((1, 4), dtype=torch.long)
    for kw in (dict(stop=[[1]]), dict(pad_token_id=0), dict(eos_token_id=[1]), dict(return_finish=True)):
        with pytest.raises(ValueError, match="token_overrides"):
            model.generate(input_ids=ids, token_overrides=torch.zeros((1, 5), dtype=torch.long), **kw)
        with pytest.raises(ValueError, match="GPU"):
            model.generate(input_ids=ids, **kw)
    with pytest.raises(ValueError, match="vocabulary"):
        model.generate(input_ids=ids, stop=[[32]])
    with pytest.raises(ValueError, match="vocabulary"):
        model.generate(input_ids=ids, pad_token_id=32)
    with pytest.raises(ValueError, match="1 to 16"):
        model.generate(input_ids=ids, stop=[[1] * 17])


def test_cpu_tensors_take_the_definition():
    from hydragen_amd import layer_ops

    spec = stop_cases.spec("overlapping", False)
    tok = stop_cases.tokens("overlapping", 9)
    state = stopping.new_state(9, tok.shape[1], spec)
    start = torch.zeros(9, dtype=torch.int64)
    for t in range(tok.shape[1]):
        layer_ops.stop_update(tok[:, t : t + 1], t, spec, *state, start)
    want = stopping.truncate_reference(tok, spec)
    assert all(torch.equal(a, b) for a, b in zip(state[:4], want))
    with pytest.raises(ValueError, match="outside"):
        layer_ops.stop_update(tok[:, 0], tok.shape[1], spec, *state, start)


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_stop_kernel_has_no_scratch_no_spill_no_lds():
    asm = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                          str(REPO / "hydragen_amd" / "csrc" / "stop_update.hip"), "-o", "-"], capture_output=True, text=True, check=True).stdout
    blocks = asm.split("  - .agpr_count:")[1:]
    assert len(blocks) == 1 and "stop_update_kernel" in blocks[0]
    meta = {k: int(re.search(rf"\.{k}:\s+(\d+)", blocks[0]).group(1)) for k in
            ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert meta["vgpr_spill_count"] == meta["sgpr_spill_count"] == meta["private_segment_fixed_size"] == 0, meta
    assert meta["group_segment_fixed_size"] == 0 and meta["vgpr_count"] <= 64, meta
    # the running-row count goes out through a vector atomic, one per wave
    assert asm.count("global_atomic_add") == 1
