"""The tiny Qwen3 model behind tests/golden/qwen3_tiny.npz, and the recorder of that file.

    python tests/qwen3_golden.py --write      (needs transformers; the tests that READ the file do not)

A 2-layer Qwen3 (hidden 64, 4 query / 2 kv heads, head_dim 64 -- not hidden // heads = 16 --, vocab 64) whose weights come from
numpy.random.default_rng(seed), not from transformers' initialisation, so that a test rebuilds them without transformers.  Every
weight sits on a grid that bf16 and fp16 both hold exactly (multiples of 2^-8 below 1, gains multiples of 2^-6 below 4): the
16-bit models under test and the fp32 model that recorded the logits have the same weights, bit for bit.  The norm gains are
1 + 0.3 normal, and the q and k gains differ.

The file holds the seed, two right-padded shared prompts (9 and 5 tokens), the forced continuations of their completions, and
transformers' fp32 logits at every position of every completion's full sequence.  It is data: the tests compare against it and
recompute it only to check that the installed transformers still agrees with the record."""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

FIXTURE = REPO / "tests" / "golden" / "qwen3_tiny.npz"
SEED = 20260
CFG = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=64,
           rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=64, head_dim=64)
PROMPT_LENS = (9, 5)   # two shared prompts, right-padded to 9
NRET, NEW = 2, 5       # completions per prompt, forced tokens per completion


def _grid(x, step):
    k = np.clip(np.rint(x / step), -255, 255)  # at most 8 significant bits: exact in bf16 and in fp16
    return (k * step).astype(np.float32)


def tiny_weights(seed=SEED):
    """{state-dict name: float32 array} in transformers' names, which are this project's names too."""
    rng = np.random.default_rng(seed)
    c = CFG
    H, Hkv, D, hid, inter, V = c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"], c["hidden_size"], c["intermediate_size"], c["vocab_size"]
    w = {"model.embed_tokens.weight": _grid(rng.standard_normal((V, hid)) * 0.5, 2.0 ** -8)}
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        for name, shape in (("self_attn.q_proj", (H * D, hid)), ("self_attn.k_proj", (Hkv * D, hid)), ("self_attn.v_proj", (Hkv * D, hid)),
                            ("self_attn.o_proj", (hid, H * D)), ("mlp.gate_proj", (inter, hid)), ("mlp.up_proj", (inter, hid)),
                            ("mlp.down_proj", (hid, inter))):
            w[p + name + ".weight"] = _grid(rng.standard_normal(shape) * 0.12, 2.0 ** -8)
        for name, n in (("self_attn.q_norm", D), ("self_attn.k_norm", D), ("input_layernorm", hid), ("post_attention_layernorm", hid)):
            w[p + name + ".weight"] = _grid(1 + 0.3 * rng.standard_normal(n), 2.0 ** -6)
    w["model.norm.weight"] = _grid(1 + 0.3 * rng.standard_normal(hid), 2.0 ** -6)
    w["lm_head.weight"] = _grid(rng.standard_normal((V, hid)) * 0.12, 2.0 ** -8)
    return w


def tokens(seed=SEED):
    """(prompts int64 [2, 9] right-padded with 0, forced int64 [2 * NRET, NEW]): token ids in [1, vocab)."""
    rng = np.random.default_rng(seed + 1)
    prompts = rng.integers(1, CFG["vocab_size"], (len(PROMPT_LENS), max(PROMPT_LENS)))
    for i, n in enumerate(PROMPT_LENS):
        prompts[i, n:] = 0
    return prompts.astype(np.int64), rng.integers(1, CFG["vocab_size"], (len(PROMPT_LENS) * NRET, NEW)).astype(np.int64)


def full_sequences(prompts, forced):
    """Completion j's whole token sequence: its prompt's true tokens, then its forced tokens but the last (whose logits nobody asks for)."""
    return [np.concatenate([prompts[j // NRET, : PROMPT_LENS[j // NRET]], forced[j, : NEW - 1]]) for j in range(forced.shape[0])]


def hf_logits(seed=SEED):
    """transformers' fp32 logits [completions, longest sequence, vocab] (zero behind a sequence's end)."""
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM

    hf = Qwen3ForCausalLM(Qwen3Config(**CFG, tie_word_embeddings=False, attention_bias=False))
    report = hf.load_state_dict({k: torch.from_numpy(v) for k, v in tiny_weights(seed).items()}, strict=False)
    assert not report.unexpected_keys and all("inv_freq" in k for k in report.missing_keys), report
    hf.eval()
    seqs = full_sequences(*tokens(seed))
    out = np.zeros((len(seqs), max(map(len, seqs)), CFG["vocab_size"]), dtype=np.float32)
    with torch.no_grad():
        for j, s in enumerate(seqs):
            out[j, : len(s)] = hf(torch.from_numpy(s)[None]).logits[0].float().numpy()
    return out


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def write():
    prompts, forced = tokens()
    np.savez_compressed(FIXTURE, seed=np.int64(SEED), prompts=prompts, prompt_lens=np.array(PROMPT_LENS, dtype=np.int64), forced=forced,
                        logits=hf_logits())
    print(f"{FIXTURE}: {FIXTURE.stat().st_size} bytes")


if __name__ == "__main__":
    if "--write" not in sys.argv:
        raise SystemExit(__doc__)
    write()
