#!/usr/bin/env python3
"""What calibrating the fp8 K/V scales costs, and what it buys.

    python tools/kv_scale_bench.py [--model llama2-7b] [--layers 8] [--batch 1024] [--prefix 2048] [--new 33] [--out profiles/kv_scale_calibration.md]

Part 1 -- hyd_kv_absmax (kv_quant.observe_absmax: K and V in one launch) against torch's abs().amax() on the same views, at C2's
shared level ([1, prefix, 32, 128] K and V) and at a unique-prompt shape ([batch, 64, 32, 128]): device time between events around
--iters launches, median over --reps, alternating in one process, and the bytes per second the kernel reads (2 x outer x rows x
Hkv x d x 2 bytes).  The results are compared first.

Part 2 -- the attention error of the fp8 suffix operator on the device (flash_attention_seqlen on quantize_kv bytes) against
float64 attention on the bf16 inputs, with unit and with calibrated scales, on the inputs of tests/kv_scale_cases.py and two more
rows (unit normal, K std 40): relative L2.

Part 3 -- a generate() of the model shell with fp8 unique caches, kv_scales="calibrate" against "unit" (two models with the same
weights, alternating): the prefill (max_new_tokens=1: every prompt launch, no decode step) and the decode step ((generate of --new
tokens - prefill) / (--new - 1), graph replay), host wall time with a synchronisation at both ends, median over --reps.  No decode
launch differs between the two, so the decode step is expected equal.

Part 4 -- a small model whose V is 2^-10 and whose K is 2^-6 of unit size (v_proj x 2^-10, o_proj x 2^10, k_proj x 2^-6, q_proj x
2^6: the same network in bf16 arithmetic, the model of tests/test_kv_scale_gpu.py): relative L2 of the decode steps' logits with
fp8 caches against the same model with bf16 caches, "unit" and "calibrate".

Writes the tables to --out and prints one JSON line per measurement."""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from hydragen_amd import kv_quant as Q
from hydragen_amd.flash import flash_attention_seqlen
from hydragen_amd.llama import HydragenLlamaForCausalLM, LlamaConfig

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama2-7b")
ap.add_argument("--layers", type=int, default=8, help="override the layer count (0 = architecture's own)")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--prefix", type=int, default=2048)
ap.add_argument("--new", type=int, default=33, help="tokens of the timed generate()")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20, help="launches per timed window of part 1")
ap.add_argument("--out", default="profiles/kv_scale_calibration.md")
a = ap.parse_args()

assert torch.cuda.is_available(), "kv_scale_bench.py measures on the GPU: there is no CPU figure"
dev = "cuda:0"
torch.manual_seed(0)
results = []


def emit(**kw):
    results.append(kw)
    print(json.dumps(kw), flush=True)


def device_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return round(statistics.median(xs), 2), [round(min(xs), 2), round(max(xs), 2)]


# ---- part 1: the reduction ----------------------------------------------------------------------------------------------------------
def part1(name, n_outer, n_rows, Hkv=32, d=128):
    # the k / v splits of a fused q|k|v output, as the prefill hands them over
    buf = torch.randn((n_outer, n_rows, 3 * Hkv * d), device=dev, dtype=torch.bfloat16)
    k, v = (t.view(n_outer, n_rows, Hkv, d) for t in buf.split(Hkv * d, dim=-1)[1:])
    amax = torch.zeros((2, Hkv), device=dev)

    def kernel():
        Q.observe_absmax(k, v, amax)

    def torch_amax():
        return torch.stack([k.abs().amax(dim=(0, 1, 3)), v.abs().amax(dim=(0, 1, 3))])

    kernel()
    assert torch.equal(amax, torch_amax().float()) and torch.equal(amax, Q.absmax_reference(k, v))
    us = {"kernel": [], "torch": []}
    for rep in range(a.reps + 1):
        for which, fn in (("kernel", kernel), ("torch", torch_amax)):
            t = device_us(fn, a.iters)
            if rep:
                us[which].append(t)
    nbytes = 2 * n_outer * n_rows * Hkv * d * 2
    (ker, ks), (ref, rs) = med(us["kernel"]), med(us["torch"])
    emit(part="absmax", shape=name, n_outer=n_outer, n_rows=n_rows, kv_heads=Hkv, head_dim=d, bytes_read=nbytes, us_kernel=ker,
         spread_kernel_us=ks, us_torch=ref, spread_torch_us=rs, tb_per_s_kernel=round(nbytes / ker / 1e6, 2), reps=a.reps, iters=a.iters)
    del buf


# ---- part 2: the error on the device ---------------------------------------------------------------------------------------------------
def attention64(q, k, v):
    q, k, v = (t.double() for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / q.shape[-1] ** 0.5
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


def part2():
    B, S, H, D = 4, 64, 4, 128
    rows = {
        "unit normal": ((1.0,) * 4, (1.0,) * 4, (1.0,) * 4),
        "V std 2e-3": ((1.0,) * 4, (1.0,) * 4, (2e-3,) * 4),
        "V std 3000": ((1.0,) * 4, (1.0,) * 4, (3000.0,) * 4),
        "mixed heads (K std 0.05, 1, 1, 1 with q x 20, 1, 1, 1; V std 1e-3, 1, 30, 2000)": ((20.0, 1.0, 1.0, 1.0), (0.05, 1.0, 1.0, 1.0), (1e-3, 1.0, 30.0, 2000.0)),
        "K std 40": ((1.0,) * 4, (40.0,) * 4, (1.0,) * 4),
    }
    g = torch.Generator(device=dev).manual_seed(1)
    ph = lambda f: torch.tensor(f, device=dev).reshape(1, 1, H, 1)  # noqa: E731
    for name, (qf, kstd, vstd) in rows.items():
        q = (torch.randn((B, 1, H, D), device=dev, generator=g) * ph(qf)).bfloat16()
        k = (torch.randn((B, S, H, D), device=dev, generator=g) * ph(kstd)).bfloat16()
        v = (torch.randn((B, S, H, D), device=dev, generator=g) * ph(vstd)).bfloat16()
        want = attention64(q, k, v)
        amax = torch.zeros((2, H), device=dev)
        Q.observe_absmax(k, v, amax)
        ks, vs = torch.ones(H, device=dev), torch.ones(H, device=dev)
        Q.scales_from_absmax(amax, ks, vs)
        err = {}
        for which, (sk, sv) in (("unit", (torch.ones_like(ks), torch.ones_like(vs))), ("calibrated", (ks, vs))):
            out, _ = flash_attention_seqlen(q, Q.quantize_kv(k, sk), Q.quantize_kv(v, sv), k_scale=sk, v_scale=sv)
            diff = out.double() - want
            err[which] = float(diff.norm() / want.norm())
            per_head = lambda t: t.pow(2).sum(dim=(0, 1, 3)).sqrt()  # noqa: E731
            err[which + "_worst_head"] = float((per_head(diff) / per_head(want)).max())
        emit(part="error", stats=name, **{k_: float(f"{v_:.3g}") for k_, v_ in err.items()})


# ---- part 3: the model shell -------------------------------------------------------------------------------------------------------------
def part3():
    cfg = LlamaConfig.llama2_7b() if a.model == "llama2-7b" else LlamaConfig.llama3_70b()
    if a.layers:
        cfg.num_hidden_layers = a.layers
    cfg.max_position_embeddings = max(cfg.max_position_embeddings, a.prefix + a.new + 16)
    models = {}
    for mode in ("unit", "calibrate"):
        m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=dev, seed=0)
        m.graph(True)
        m.setup_caches(max_unique_batch_size=a.batch, max_unique_seq_length=a.new + 16, max_shared_batch_sizes=[1],
                       max_shared_seq_lengths=[a.prefix], kv_cache_dtype=torch.float8_e4m3fn, kv_scales=mode)
        models[mode] = m
    prompt = torch.randint(1, cfg.vocab_size, (1, a.prefix), device=dev)
    ms = {(mode, n): [] for mode in models for n in (1, a.new)}
    with torch.no_grad():
        for rep in range(a.reps + 1):  # (rep 0 warms up and captures the decode graphs)
            for mode, m in models.items():
                for n in (1, a.new):
                    t = wall_ms(lambda: m.generate(input_ids=prompt, num_return_sequences=a.batch, max_new_tokens=n, temperature=1.0))
                    if rep:
                        ms[(mode, n)].append(t)
    rec = dict(part="generate", model=a.model, layers=cfg.num_hidden_layers, batch=a.batch, prefix=a.prefix, new_tokens=a.new, reps=a.reps)
    for mode in models:
        pre = ms[(mode, 1)]
        step = [(full - p) / (a.new - 1) for full, p in zip(ms[(mode, a.new)], pre)]
        rec[f"ms_prefill_{mode}"], rec[f"spread_prefill_{mode}"] = med(pre)
        rec[f"ms_decode_step_{mode}"], rec[f"spread_decode_step_{mode}"] = (round(statistics.median(step), 4),
                                                                            [round(min(step), 4), round(max(step), 4)])
    ks = models["calibrate"].model.layers[0].self_attn.kv_cache.k_scale
    rec["layer0_k_scale_calibrated"] = sorted(set(ks.tolist()))
    emit(**rec)


# ---- part 4: a model with small V and K ---------------------------------------------------------------------------------------------------
def part4():
    cfg = LlamaConfig(hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=512, max_position_embeddings=1024, rms_norm_eps=1e-5)
    m = HydragenLlamaForCausalLM.from_config(cfg, dtype=torch.bfloat16, device=dev, seed=3, std=0.05)
    with torch.no_grad():
        for layer in m.model.layers:
            at = layer.self_attn
            at.v_proj.weight.mul_(2.0 ** -10)
            at.o_proj.weight.mul_(2.0 ** 10)
            at.k_proj.weight.mul_(2.0 ** -6)
            at.q_proj.weight.mul_(2.0 ** 6)
    g = torch.Generator(device=dev).manual_seed(13)
    B, n = 6, 6
    prefix, ov = torch.randint(1, 512, (1, 50), device=dev, generator=g), torch.randint(1, 512, (B, n), device=dev, generator=g)
    logits = {}
    for name, kw in (("bf16", {}), ("unit", dict(kv_cache_dtype=torch.float8_e4m3fn)),
                     ("calibrate", dict(kv_cache_dtype=torch.float8_e4m3fn, kv_scales="calibrate"))):
        m.setup_caches(max_unique_batch_size=B, max_unique_seq_length=32, max_shared_batch_sizes=[1], max_shared_seq_lengths=[50], **kw)
        _, lg = m.generate(input_ids=prefix, num_return_sequences=B, max_new_tokens=n, temperature=0.0, return_logits=True, token_overrides=ov)
        logits[name] = torch.stack(lg[1:]).double()
    err = {k_: float((logits[k_] - logits["bf16"]).norm() / logits["bf16"].norm()) for k_ in ("unit", "calibrate")}
    emit(part="model", rel_l2_unit=float(f"{err['unit']:.3g}"), rel_l2_calibrate=float(f"{err['calibrate']:.3g}"),
         ratio=round(err["unit"] / err["calibrate"], 1))


part1("C2 shared level", 1, a.prefix)
part1("unique prompts", a.batch, 64)
part2()
part3()
part4()

p1 = [r for r in results if r["part"] == "absmax"]
p2 = [r for r in results if r["part"] == "error"]
g = [r for r in results if r["part"] == "generate"][0]
pm = [r for r in results if r["part"] == "model"][0]
lines = [f"""# Calibrated fp8 K/V scales (tools/kv_scale_bench.py)

## The reduction: hyd_kv_absmax against torch's abs().amax()

K and V views [outer, rows, 32, 128] bf16, the k / v splits of a fused q|k|v buffer (row stride 3 x 32 x 128).  Device time
between events around {a.iters} back-to-back launches, median over {a.reps} repetitions (min .. max), the two alternating in one
process.  The kernel is one launch for K and V; torch is abs() + amax() per tensor (four launches, two temporaries).  The rate
counts the bytes the kernel must read; at the shared level's size repeated launches find them in the Infinity Cache.

| shape | bytes read | hyd_kv_absmax | rate | torch abs().amax() |
|---|---|---|---|---|"""]
for r in p1:
    lines.append(f"| {r['shape']} [{r['n_outer']}, {r['n_rows']}, {r['kv_heads']}, {r['head_dim']}] | {r['bytes_read'] / 2**20:.0f} MiB | {r['us_kernel']} us "
                 f"({r['spread_kernel_us'][0]} .. {r['spread_kernel_us'][1]}) | {r['tb_per_s_kernel']} TB/s | {r['us_torch']} us "
                 f"({r['spread_torch_us'][0]} .. {r['spread_torch_us'][1]}) |")
lines.append("""
## The error: fp8 suffix operator on the device against float64 attention on the bf16 inputs

B 4 x S 64 x H 4 x D 128, relative L2, whole tensor (worst head).  Scales from hyd_kv_absmax + hyd_kv_scales_from_absmax, margin 2.

| K / V statistics | scale 1 | calibrated |
|---|---|---|""")
for r in p2:
    lines.append(f"| {r['stats']} | {r['unit']:.2e} ({r['unit_worst_head']:.2e}) | {r['calibrated']:.2e} ({r['calibrated_worst_head']:.2e}) |")
lines.append(f"""
The K std 40 row is not a range problem and calibration does not help it: three mantissa bits, amplified by the score range.

A whole model with small K and V (2 layers, 4 heads x 128, v_proj x 2^-10 and k_proj x 2^-6 with o_proj / q_proj scaled back: the
same network in bf16), one shared prompt of 50 tokens, 6 completions, 5 decode steps: relative L2 of the logits with fp8 caches
against bf16 caches {pm['rel_l2_unit']:.2e} with "unit" (V flushes to zero) and {pm['rel_l2_calibrate']:.2e} with "calibrate": a factor of {pm['ratio']}.

## generate(): kv_scales="calibrate" against "unit"

{a.model} shell ({g['layers']} layers, random weights, bf16, fp8 unique caches), one shared prompt of {g['prefix']} tokens, {g['batch']}
completions, HIP-graph decode.  Host wall time with a synchronisation at both ends, median over {g['reps']} repetitions (min .. max),
two models with the same weights alternating.  Prefill: generate(max_new_tokens=1).  Decode step: (generate of {g['new_tokens']} tokens
- prefill) / {g['new_tokens'] - 1}.

| | "unit" | "calibrate" |
|---|---|---|
| prefill | {g['ms_prefill_unit']} ms ({g['spread_prefill_unit'][0]} .. {g['spread_prefill_unit'][1]}) | {g['ms_prefill_calibrate']} ms ({g['spread_prefill_calibrate'][0]} .. {g['spread_prefill_calibrate'][1]}) |
| decode step | {g['ms_decode_step_unit']} ms ({g['spread_decode_step_unit'][0]} .. {g['spread_decode_step_unit'][1]}) | {g['ms_decode_step_calibrate']} ms ({g['spread_decode_step_calibrate'][0]} .. {g['spread_decode_step_calibrate'][1]}) |

"calibrate" adds, per layer and prefill, one hyd_kv_absmax launch (and the int32 lengths of a shared level), and per call one
hyd_kv_scales_from_absmax launch per layer before the first decode step; no decode launch differs.  Layer 0's calibrated K scales
on these random weights: {g['layer0_k_scale_calibrated']}.
""")
out = Path(a.out)
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines))
print(f"wrote {out}")
