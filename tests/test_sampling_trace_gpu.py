"""-m gpu: which C entry points generate() calls, and how often, for every sampling route (sampling.sample_route's table) -- the
launches a decode call is made of, and the promise that neutral penalty arguments and constraint=None add none."""
import pytest
import torch

from hydragen_amd import _lib
from tests.gpu_util import Recorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN, FILTERED, PENALIZED, CONSTRAINED = (
    "hyd_sample_tokens", "hyd_sample_tokens_filtered", "hyd_sample_tokens_penalized", "hyd_sample_tokens_constrained")
LOGPROBS, STOP, BITMAP = "hyd_token_logprobs", "hyd_stop_update", "hyd_token_bitmap_build"
COUNTED = (PLAIN, FILTERED, PENALIZED, CONSTRAINED, LOGPROBS, STOP, BITMAP)
EOS = 511


@pytest.fixture(scope="module")
def model():
    from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=DEV, seed=0, std=0.05)
    m.setup_caches(max_unique_batch_size=4, max_unique_seq_length=16, max_shared_batch_sizes=[1], max_shared_seq_lengths=[8])
    m.graph(False)
    for ids, fan in ((_prompt(1, (1, 8)), 4), ([_prompt(1, (1, 8)), _prompt(2, (4, 3))], 1)):  # (what a first call sets up is no part of a trace)
        m.generate(input_ids=ids, num_return_sequences=fan, max_new_tokens=3, temperature=0.7)
    return m


def _prompt(seed, shape):
    return torch.randint(1, 500, shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _dfa():
    from hydragen_amd.constraint import TokenDFA

    return TokenDFA.from_choices([[5, 6, 7, 8], [5, 9, 10, 11], [300, 301, 302, 303]], 512, eos=[EOS]).to(DEV)


def _trace(model, monkeypatch, unique=False, switches=(), **kw):
    """The entry points one generate() call goes through, in order.  The fan variant: one shared [1, 8] prompt and 4 samples (the
    first draw fans out: torch); the unique variant: the shared prompt plus 4 own prompts of 3 tokens, one sample each."""
    if kw.get("constraint") == "dfa":
        kw["constraint"] = _dfa()
    ids = [_prompt(1, (1, 8)), _prompt(2, (4, 3))] if unique else _prompt(1, (1, 8))
    with monkeypatch.context() as m:
        for name in switches:
            m.setattr(model, name, False)
        rec = Recorder(_lib.load())
        m.setattr(_lib, "_lib", rec)
        torch.manual_seed(1234)
        model.generate(input_ids=ids, num_return_sequences=1 if unique else 4, max_new_tokens=3, temperature=0.7, **kw)
    return rec.calls


def _counts(calls):
    return {name: calls.count(name) for name in COUNTED if name in calls}


FAN = {
    "defaults": (dict(), (), {PLAIN: 2}),
    "top_p": (dict(top_p=0.9), (), {FILTERED: 2}),
    "top_p, torch cuts": (dict(top_p=0.9), ("fused_sampling_filters",), {PLAIN: 2}),
    "logprobs": (dict(return_logprobs=True), (), {FILTERED: 2}),
    "frequency": (dict(frequency_penalty=0.5), (), {PENALIZED: 2}),
    "frequency, torch penalties": (dict(frequency_penalty=0.5), ("fused_sampling_penalties",), {PLAIN: 2}),
    "bias alone": (dict(logit_bias={3: -2.0, 17: 1.5}), (), {PENALIZED: 2}),
    # the fanned first draw: the filtered kernel on the masked rows
    "constraint": (dict(constraint="dfa"), (), {FILTERED: 1, CONSTRAINED: 2}),
    "constraint + frequency, torch penalties": (dict(constraint="dfa", frequency_penalty=0.5), ("fused_sampling_penalties",), {FILTERED: 3}),
    "eos list": (dict(eos_token_id=[EOS]), (), {STOP: 3, PLAIN: 2}),
    "top_logprobs": (dict(return_logprobs=True, top_logprobs=2), (), {LOGPROBS: 3, FILTERED: 2}),
}
UNIQUE = {
    "defaults": (dict(), (), {PLAIN: 3}),
    "frequency": (dict(frequency_penalty=0.5), (), {PENALIZED: 3, BITMAP: 2}),  # the own prompts' token set
    "constraint": (dict(constraint="dfa"), (), {CONSTRAINED: 3}),
}


@pytest.mark.parametrize("variant, case", [("fan", c) for c in FAN] + [("unique", c) for c in UNIQUE])
def test_entry_points_of_a_generate_call(model, monkeypatch, variant, case):
    kw, switches, want = (FAN if variant == "fan" else UNIQUE)[case]
    want = {BITMAP: 1, **want}  # append_shared records the shared level's token set, whatever is asked for
    assert _counts(_trace(model, monkeypatch, variant == "unique", switches, **kw)) == want


@pytest.mark.parametrize("unique", [False, True])
def test_neutral_arguments_add_no_call(model, monkeypatch, unique):
    for base in (dict(), dict(top_p=0.9, return_logprobs=True), dict(eos_token_id=[EOS])):
        want = _trace(model, monkeypatch, unique, **base)
        assert want and _trace(model, monkeypatch, unique, constraint=None, **base) == want
        neutral = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias={})
        assert _trace(model, monkeypatch, unique, **neutral, **base) == want
