"""-m gpu: the full ordered list of C entry points -- every hyd_* name, the per-layer ones included -- that generate() goes through
in each of its three decode loops (hydragen_amd/generation.py), against tests/golden/generate_entry_points.json.  The golden file
was recorded with `python -m tests.test_generate_trace_gpu FILE` on the commit before the loops moved out of llama.py (twice: the
two recordings were equal).  Every case runs a number of steps that no drawn token can change: either the call has no exit
before max_new_tokens, or a one-choice automaton fixes every token.  (The recorder does not see torch's own launches.)"""
import json
import pathlib

import pytest
import torch

from hydragen_amd import _lib
from tests.gpu_util import Recorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = pathlib.Path(__file__).parent / "golden" / "generate_entry_points.json"
EOS = 511
FIVE, NINE = [20, 21, 22, 23, 24], [30, 31, 32, 33, 34, 35, 36, 37, 38]


def _prompt(seed, shape):
    return torch.randint(1, 500, shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _forced(choice):
    """Every token is fixed: the one choice, then EOS."""
    from hydragen_amd.constraint import TokenDFA

    return TokenDFA.from_choices([choice], 512, eos=[EOS]).to(DEV)


# name -> (unique prompts?, generate()'s arguments, attributes set on the model).  "No poll": max_new_tokens < stop_poll_steps
CASES = {
    "plain, fan": (False, lambda: dict(max_new_tokens=6), {}),
    "plain, ragged own prompts": (True, lambda: dict(max_new_tokens=6), {}),
    "plain, int eos, forced": (False, lambda: dict(eos_token_id=EOS, constraint=_forced(FIVE), max_new_tokens=12), {}),
    "plain, frequency + overrides": (False, lambda: dict(frequency_penalty=0.5, token_overrides=_prompt(3, (4, 6)), max_new_tokens=6), {}),
    "stop, forced": (False, lambda: dict(eos_token_id=[EOS], constraint=_forced(FIVE), max_new_tokens=16), dict(stop_poll_steps=2)),
    "stop sequence, logprobs, finish": (False, lambda: dict(
        eos_token_id=[EOS], constraint=_forced(FIVE), max_new_tokens=16, stop=[FIVE[2:4]], return_logprobs=True, top_logprobs=2,
        return_finish=True), dict(stop_poll_steps=2)),
    "draft constraint": (False, lambda: dict(
        eos_token_id=[EOS], constraint=_forced(NINE), max_new_tokens=16, draft_tokens=3, draft="constraint", return_draft_stats=True),
        dict(stop_poll_steps=1)),
    "draft tensor, forced": (False, lambda: dict(
        eos_token_id=[EOS], constraint=_forced(NINE), max_new_tokens=16, draft_tokens=2, draft=_prompt(4, (4, 16)), return_draft_stats=True),
        dict(stop_poll_steps=1)),
    "draft prompt_lookup, forced": (False, lambda: dict(
        eos_token_id=[EOS], constraint=_forced(NINE), max_new_tokens=16, draft_tokens=3, draft="prompt_lookup", return_draft_stats=True),
        dict(stop_poll_steps=1)),
    "draft tensor, no constraint": (False, lambda: dict(
        max_new_tokens=6, draft_tokens=2, draft=_prompt(5, (4, 6)), temperature=0.7, return_logprobs=True), {}),
}


def inputs(unique):
    """One shared [1, 8] prompt fanned out to 4 samples, or the shared prompt and 4 own prompts of ragged lengths."""
    if not unique:
        return dict(input_ids=_prompt(1, (1, 8)), num_return_sequences=4)
    return dict(input_ids=[_prompt(1, (1, 8)), _prompt(2, (4, 5))], seq_lens=[torch.tensor([8], device=DEV), torch.tensor([3, 5, 2, 4], device=DEV)])


def make_model():
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0, std=0.05)
    m.setup_caches(max_unique_batch_size=4, max_unique_seq_length=32, max_shared_batch_sizes=[1], max_shared_seq_lengths=[8])
    m.graph(False)
    for unique in (False, True):  # (what a first call sets up is no part of a trace)
        m.generate(max_new_tokens=3, temperature=0.7, **inputs(unique))
    return m


@pytest.fixture(scope="module")
def model():
    return make_model()


def run_case(model, name, monkeypatch):
    """(generate()'s return value, the entry points it went through, in order) for one case."""
    unique, kw, attrs = CASES[name]
    kw = {"temperature": 0.7, **inputs(unique), **kw()}
    with monkeypatch.context() as m:
        for attr, value in attrs.items():
            m.setattr(model, attr, value)
        rec = Recorder(_lib.load())
        m.setattr(_lib, "_lib", rec)
        torch.manual_seed(1234)
        out = model.generate(**kw)
    return out, rec.calls


def run_length(calls):
    out = []
    for name in calls:
        if out and out[-1][0] == name:
            out[-1][1] += 1
        else:
            out.append([name, 1])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_entry_points_equal_the_recorded_ones(model, monkeypatch, name):
    want = json.loads(GOLDEN.read_text())[name]
    got = run_length(run_case(model, name, monkeypatch)[1])
    assert len(got) > 4 and got == want


if __name__ == "__main__":
    import sys

    with pytest.MonkeyPatch.context() as mp:
        model_ = make_model()
        traces = {name: run_length(run_case(model_, name, mp)[1]) for name in CASES}
    pathlib.Path(sys.argv[1]).write_text(json.dumps(traces, separators=(",", ":")) + "\n")
