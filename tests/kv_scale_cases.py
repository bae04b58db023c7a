"""Inputs shared by tests/test_kv_scale.py and tests/test_kv_scale_gpu.py: the K / V statistics at which an fp8 cache with unit
scales fails and a calibrated one does not, and the error they are judged by."""
import numpy as np
import torch

from hydragen_amd.kv_quant import dequantize_kv, quantize_kv
from oracle import hydragen_oracle as O

B, S, H, D = 4, 64, 4, 128

# name -> (q factor per head, K std per head, V std per head)
STATS = {
    "mixed_heads": ((20.0, 1.0, 1.0, 1.0), (0.05, 1.0, 1.0, 1.0), (1e-3, 1.0, 30.0, 2000.0)),
    "v_std_2e-3": ((1.0,) * 4, (1.0,) * 4, (2e-3,) * 4),
    "v_std_3000": ((1.0,) * 4, (1.0,) * 4, (3000.0,) * 4),
}


def make_inputs(name, dtype=torch.bfloat16):
    """q [B, 1, H, D], k / v [B, S, H, D] in `dtype` (what a prefill hands the cache), seeded by the case."""
    qf, ks, vs = STATS[name]
    g = torch.Generator().manual_seed(1000 + sorted(STATS).index(name))
    per_head = lambda f: torch.tensor(f, dtype=torch.float32).reshape(1, 1, H, 1)  # noqa: E731
    q = (torch.randn((B, 1, H, D), generator=g) * per_head(qf)).to(dtype)
    k = (torch.randn((B, S, H, D), generator=g) * per_head(ks)).to(dtype)
    v = (torch.randn((B, S, H, D), generator=g) * per_head(vs)).to(dtype)
    return q, k, v


def attention64(q, k, v):
    """float64 attention of the oracle on torch tensors of any float dtype -> numpy [B, 1, H, D]."""
    f = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    return O.flash_attention_seqlen(f(q), f(k), f(v), None)[0]


def rel_l2(got, want):
    """(whole tensor, worst head) relative L2 of [B, 1, H, D] arrays."""
    heads = [np.linalg.norm(got[:, :, h] - want[:, :, h]) / np.linalg.norm(want[:, :, h]) for h in range(want.shape[2])]
    return float(np.linalg.norm(got - want) / np.linalg.norm(want)), float(max(heads))


def fp8_round_trip(x, scale):
    return dequantize_kv(quantize_kv(x, scale), scale, x.dtype)
