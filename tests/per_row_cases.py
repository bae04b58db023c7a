"""What tests/test_per_row_sampling.py and tests/test_per_row_sampling_gpu.py share: the table of 12 parameter combinations the rows
of a per-row call cycle through, and the rows of the seeded mirror test."""
import torch

NAMES = ("temperature", "top_k", "top_p", "min_p", "repetition_penalty", "frequency_penalty", "presence_penalty")


def F32(v):
    """v rounded to fp32, as a Python float: per-row values reach the kernel as fp32, and a scalar launch that is to give the same
    bits is given the same number."""
    return float(torch.tensor(v, dtype=torch.float32))


# T in {0, 0.7, 1.3}; top_k in {0, 1, 40}; top_p in {1, 0.9, 0.5}; min_p in {0, 0.05}; each penalty on and off (a repetition penalty
# below and above 1, a negative frequency penalty)
TABLE = [tuple(v if i == 1 else F32(v) for i, v in enumerate(row)) for row in [
    (0.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0),
    (0.7, 1, 1.0, 0.0, 1.0, 0.0, 0.0),
    (1.3, 40, 1.0, 0.0, 1.3, 0.0, 0.0),
    (0.7, 0, 0.9, 0.0, 1.0, 0.5, 0.0),
    (1.3, 0, 0.5, 0.05, 1.0, 0.0, 0.25),
    (0.0, 40, 0.9, 0.0, 1.2, 0.1, 0.1),
    (0.7, 40, 0.5, 0.05, 1.0, 0.0, 0.0),
    (1.3, 1, 0.9, 0.05, 0.8, 0.0, 0.0),
    (0.7, 0, 1.0, 0.05, 1.0, -0.5, 0.0),
    (0.0, 0, 0.5, 0.0, 1.5, 0.0, 0.5),
    (1.3, 40, 0.9, 0.05, 1.3, 0.25, 0.25),
    (0.7, 0, 1.0, 0.0, 1.0, 0.0, 0.0),
]]
assert len(TABLE) == 12

MIRROR_SEED = 0  # see mirror_case
MIRROR_ROWS, MIRROR_N, MIRROR_OFFSET = 256, 32003, 12


def mirror_case(seed=MIRROR_SEED):
    """(bf16 [256, 32003] rows of randn * 3 on the CPU, a temperature per row from {0.7, 1.0, 1.3}, a distinct 64-bit seed per row,
    the offset).  MIRROR_SEED: the first generator seed for which tests/sampler_mirror.mirror_draw, run alone on the CPU, leaves no
    row with 0 < margin <= EPS."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(MIRROR_ROWS, MIRROR_N, generator=g) * 3.0).to(torch.bfloat16)
    temps = [(0.7, 1.0, 1.3)[r % 3] for r in range(MIRROR_ROWS)]
    seeds = [(0xD1B54A32D192ED03 * (r + 1) + seed) & 0xFFFFFFFFFFFFFFFF for r in range(MIRROR_ROWS)]
    return x, temps, seeds, MIRROR_OFFSET
