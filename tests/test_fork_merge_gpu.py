"""-m gpu: fork with merged levels on the device -- hyd_kv_gather_paths against its torch definition (exact), bad device data, the
model's fork(merge_from=) through the kernel and through torch (bit-identical), a twice-forked hierarchy with uneven survivors
against the same tokens decoded without a fork (the decomposition bound of tests/test_fork_gpu.py), the penalties' bitmap of the
merged level, graph replay across merged forks, the beam-search driver with select="prompt", and the refusals."""
import ctypes as C

import pytest
import torch

from tests.test_model_gpu import make_model, rdiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
B_ARENA, R_ARENA = 12, 48


# ---- 1. the kernel against gather_paths_reference ---------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8)


def _random_bytes(t, g):
    raw = _bits(t)
    if t.element_size() == 1:
        raw.copy_(torch.randint(0, 256, tuple(raw.shape), device=DEV, generator=g).to(torch.uint8))
    else:
        raw.copy_((torch.randint(0, 65536, tuple(raw.shape), device=DEV, generator=g) - 32768).to(torch.int16))


def _source(dtype, Hkv, d, seed):
    """K and V views of a real arena of batch 12 and 48 rows (the batch stride is the arena's), filled with random BYTES: NaNs of
    every payload for the 16-bit copy, every e4m3fn code for the widening."""
    from hydragen_amd import placement

    arena = placement.kv_arena((B_ARENA, R_ARENA, Hkv, d), dtype, DEV, zero=True)
    g = torch.Generator(device=DEV).manual_seed(seed)
    _random_bytes(arena, g)
    k, v = arena[0], arena[1]
    assert k.stride(0) == 2 * R_ARENA * Hkv * d and v.data_ptr() != k.data_ptr()
    if dtype == FP8:  # NaN (both signs) and +-448 in chosen places of rows that are gathered
        special = torch.tensor([0x7F, 0xFF, 0x7E, 0xFE, 0x00, 0x80, 0x01, 0x81], dtype=torch.uint8, device=DEV)
        for t in (k, v):
            t.view(torch.uint8)[7, 0, :, :8] = special
            t.view(torch.uint8)[2, 14, -1, -8:] = special
    return k, v


def _level(lens_l, Hkv, D, dtype, g, slack=2):
    """A packed chain level of random bytes with the given sequence lengths and `slack` unused tokens behind them."""
    cu = torch.zeros(len(lens_l) + 1, dtype=torch.int32, device=DEV)
    cu[1:] = torch.tensor(lens_l, device=DEV).cumsum(0)
    k = torch.empty((sum(lens_l) + slack, Hkv, D), dtype=dtype, device=DEV)
    v = torch.empty_like(k)
    _random_bytes(k, g)
    _random_bytes(v, g)
    return (k, v, cu, len(lens_l))


ROWS = [7, 6, 8, 2, 11]   # level of 4 (3 rows each): three children of parent 2, none of parent 1; not monotone
CONFIGS = ([(dt, dt, h, d, d) for dt in (torch.bfloat16, torch.float16) for h in (1, 4, 8) for d in (64, 128, 256)]
           + [(torch.bfloat16, torch.bfloat16, 8, 80, 128), (torch.bfloat16, torch.bfloat16, 8, 96, 128),
              (torch.bfloat16, torch.bfloat16, 4, 192, 256)]
           + [(FP8, dt, 8, d, d, sc) for dt in (torch.bfloat16, torch.float16) for d in (64, 128) for sc in (True, False)])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(str(x).replace("torch.", "") for x in c))
def test_gather_kernel_equals_reference_bit_for_bit(cfg):
    """A workgroup's chunk is 1024 destination vectors: 128 tokens with Hkv = 1, d = 64 (every segment boundary of a path inside
    one chunk), 8 tokens with Hkv = 8, d = 128 (a 17-token segment spans three), 4 with Hkv = 8, d = 256.  The draw of all-16
    chain lengths puts the segment boundaries at tokens 16 and 32: exactly on a chunk boundary for every chunk of 4 .. 32 tokens."""
    from hydragen_amd.fork import gather_paths, gather_paths_reference

    src_dtype, dtype, Hkv, d, D = cfg[:5]
    scaled = len(cfg) > 5 and cfg[5]
    k, v = _source(src_dtype, Hkv, d, seed=Hkv * 1000 + d)
    kw = {}
    if scaled:  # non-power-of-two per-head scales
        kw = dict(k_scale=(torch.arange(Hkv, device=DEV).float() * 0.37 + 0.11), v_scale=(torch.arange(Hkv, device=DEV).float() * 0.053 + 1.3))
    rows = torch.tensor(ROWS, device=DEV)
    g = torch.Generator().manual_seed(d + Hkv)
    gd = torch.Generator(device=DEV).manual_seed(d * 7 + Hkv)
    chain_choices, uniq_choices = torch.tensor([1, 15, 16, 17]), torch.tensor([0, 1, 15, 16, 17, 48])
    pick = lambda c, n: c[torch.randint(0, c.numel(), (n,), generator=g)].tolist()
    draws = [(pick(chain_choices, 4), pick(chain_choices, 2), pick(uniq_choices, 5)) for _ in range(2)]
    draws += [([16] * 4, [16] * 2, [16, 48, 0, 1, 15]), ([17] * 4, [17] * 2, [17, 0, 17, 48, 0])]
    for la, lb, lens_l in draws:
        full = [_level(la, Hkv, D, dtype, gd), _level(lb, Hkv, D, dtype, gd)]
        lens = torch.tensor(lens_l, device=DEV)
        for nl in (0, 1, 2):
            levels = full[:nl]
            paths = [sum([la[r // 3], lb[r // 6]][:nl]) + n for r, n in zip(ROWS, lens_l)]
            total, cap = sum(paths), sum(paths) + 9
            outs = []
            for fn, extra in ((gather_paths, dict(max_len=max(max(lens_l), 1), max_path=max(max(paths), 1))), (gather_paths, {}), (gather_paths_reference, {})):
                kd = torch.empty((cap, Hkv, D), dtype=dtype, device=DEV)
                vd = torch.empty_like(kd)
                _bits(kd).fill_(0x5A5A)
                _bits(vd).fill_(0x3C3C)
                cu = fn(levels, k, v, rows, lens, kd, vd, old_batch=B_ARENA, **kw, **extra)
                assert cu.dtype == torch.int32 and cu.is_cuda and cu.tolist() == [0] + torch.tensor(paths).cumsum(0).tolist()
                outs.append((kd, vd))
            (k1, v1), (k2, v2), (kr, vr) = outs
            for got in ((k1, v1), (k2, v2)):
                for a, b, fill in ((got[0], kr, 0x5A5A), (got[1], vr, 0x3C3C)):
                    assert torch.equal(_bits(a), _bits(b)), (cfg, la, lb, lens_l, nl, (_bits(a) != _bits(b)).nonzero()[:4].tolist())
                    assert bool((_bits(a[total:]) == fill).all())        # tokens at or past cu_dst[n] keep the sentinel
            # the pieces themselves: chain segments are the levels' bytes, a 16-bit unique segment the source's, pad columns zero
            at = 0
            for r, n, pl in zip(ROWS, lens_l, paths):
                for (lk, lv, lcu, s) in levels:
                    p = r // (B_ARENA // s)
                    lo, hi = int(lcu[p]), int(lcu[p + 1])
                    assert torch.equal(_bits(k1[at : at + hi - lo]), _bits(lk[lo:hi])) and torch.equal(_bits(v1[at : at + hi - lo]), _bits(lv[lo:hi]))
                    at += hi - lo
                if src_dtype != FP8:
                    assert torch.equal(_bits(k1[at : at + n, :, :d]), _bits(k[r, :n])) and torch.equal(_bits(v1[at : at + n, :, :d]), _bits(v[r, :n]))
                assert not _bits(k1[at : at + n, :, d:]).any() and not _bits(v1[at : at + n, :, d:]).any()
                at += n
            assert at == total


def test_gather_kernel_skips_sequences_with_bad_device_data():
    """A row outside [0, B), a parent whose offsets were corrupted, a unique length over the source's rows, a path past the
    capacity: exactly that sequence is skipped, the others are copied, and every other byte of the pool -- the guard tokens behind
    the destination included -- keeps its value."""
    from hydragen_amd import _lib
    from hydragen_amd.flash import _stream

    Hkv, d = 4, 64
    k, v = _source(torch.bfloat16, Hkv, d, seed=9)
    gd = torch.Generator(device=DEV).manual_seed(3)
    la, lb = [5, 16, 3, 17], [9, 4]
    A, Bl = _level(la, Hkv, d, torch.bfloat16, gd), _level(lb, Hkv, d, torch.bfloat16, gd)
    Bl[2][2] = Bl[0].shape[0] + 5       # corrupted: the second sequence of the level of 2 runs past it (rows 6 .. 11 hang off it)
    A[2][4] = A[2][3] - 1               # corrupted: the last sequence of the level of 4 is negative (rows 9 .. 11)
    cap, guard = 120, 8
    pool = torch.full((2, cap + guard, Hkv, d), 3.0, dtype=torch.bfloat16, device=DEV)
    kd, vd = pool[0, :cap], pool[1, :cap]
    #          good  row>=B  bad cu_B  len>rows  good  bad cu_A  overflow  row<0
    rows_l = [1,    12,     7,        2,        5,    10,       3,        -1]
    lens_l = [5,    4,      4,        49,       7,    2,        40,       3]
    path_ok = lambda r, n: la[r // 3] + lb[r // 6] + n
    cu_l = [0, 19, 30, 50, 60, 88, 95, 100, 110]   # 0: 5 + 9 + 5 = 19 tokens; 4: 16 + 9 + 7 = 32 at 60; 6: 16 + 9 + 40 = 65 at 95 > 120
    assert path_ok(1, 5) == 19 and path_ok(5, 7) == 32 and 95 + path_ok(3, 40) > cap
    rows = torch.tensor(rows_l, dtype=torch.int32, device=DEV)
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    cu = torch.tensor(cu_l, dtype=torch.int32, device=DEV)
    p = _lib.KvGatherParams()
    for j, (lk, lv, lcu, s) in enumerate((A, Bl)):
        p.level_k[j], p.level_v[j], p.level_cu[j] = lk.data_ptr(), lv.data_ptr(), lcu.data_ptr()
        p.level_s[j], p.level_cap[j], p.level_div[j] = s, lk.shape[0], B_ARENA // s
    p.k_src, p.v_src, p.k_dst, p.v_dst = k.data_ptr(), v.data_ptr(), kd.data_ptr(), vd.data_ptr()
    p.rows, p.lens, p.cu_dst = rows.data_ptr(), lens.data_ptr(), cu.data_ptr()
    p.k_batch_stride, p.k_tok_stride, p.k_head_stride = k.stride(0), k.stride(1), k.stride(2)
    p.v_batch_stride, p.v_tok_stride, p.v_head_stride = v.stride(0), v.stride(1), v.stride(2)
    p.src_dtype = p.dst_dtype = _lib.HYD_BF16
    p.n, p.n_levels, p.B, p.src_rows, p.Hkv, p.d_src, p.d_dst = len(rows_l), 2, B_ARENA, R_ARENA, Hkv, d, d
    p.capacity, p.max_len, p.max_path = cap, 0, 0
    _lib.check(_lib.load().hyd_kv_gather_paths(C.byref(p), _stream()))
    torch.cuda.synchronize()
    want = torch.full_like(pool, 3.0)
    for i in (0, 4):
        r, n, at = rows_l[i], lens_l[i], cu_l[i]
        for w, (src, which) in enumerate(((k, 0), (v, 1))):
            a_lo, b_lo = int(A[2][r // 3]), int(Bl[2][r // 6])
            piece = torch.cat([A[which][a_lo : a_lo + la[r // 3]], Bl[which][b_lo : b_lo + lb[r // 6]], src[r, :n]])
            want[w, at : at + piece.shape[0]] = piece
    assert torch.equal(_bits(pool), _bits(want))
    # a path longer than the host's bound is skipped too: max_path 31 keeps sequence 0 (19) and drops sequence 4 (32)
    pool.fill_(3.0)
    p.max_path = 31
    _lib.check(_lib.load().hyd_kv_gather_paths(C.byref(p), _stream()))
    torch.cuda.synchronize()
    want[:, 60:92] = 3.0
    assert torch.equal(_bits(pool), _bits(want))


# ---- 2. the model -----------------------------------------------------------------------------------------------------------
def _set_scales(model):
    for i, layer in enumerate(model.model.layers):
        kv = layer.self_attn.kv_cache
        n = kv.k_scale.numel()
        kv.k_scale.copy_(torch.arange(n, device=DEV).float() * 0.21 + 0.6 + 0.1 * i)
        kv.v_scale.copy_(torch.arange(n, device=DEV).float() * 0.13 + 0.45 + 0.1 * i)


N, M1, M2, B0, EXPAND = 8, 6, 5, 6, 3
ROWS1, LENS1 = [5, 0, 3], [N - 1, N - 3, N - 2]
ROWS2, LENS2 = [0, 2, 1, 7], [M1, M1 - 2, M1 - 1, M1 - 3]    # three children of survivor 0, none of survivor 1, one of survivor 2
ROWS2_REGULAR, LENS2_REGULAR = [1, 5, 6], [M1 - 1, M1, M1 - 2]  # one child of every survivor: the chain fork takes it too


def _tokens(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    return dict(prefix=rnd(1, 50), ovA=rnd(B0, N), ovB=rnd(len(ROWS1) * EXPAND, M1), ovC=rnd(8, M2))


def _setup(model, **kw):
    model.setup_caches(max_unique_batch_size=12, max_unique_seq_length=32, max_shared_batch_sizes=[1, 4, 4],
                       max_shared_seq_lengths=[50, 32, 16], **kw)


def _twice_forked(model, tk, rows2, lens2, second, first_merged=False, use_kernel=True, **gen_kw):
    """Teacher-forced: B0 completions of N tokens, a first fork of ROWS1 (plain, or merge_from == used), EXPAND children of M1
    tokens each with their OWN tokens, then the second fork of rows2 -- second = "merged" (merge_from=1) or "chain" (plain) --
    and two children per survivor decoding M2 tokens (the two of a survivor fed the same tokens).
    -> (tokens, logits [M2, 2 * k, V], paths: the k survivors' token lists since the prefix, first: their first uncached token)."""
    ext = dict(temperature=0.0, shared_cache_op="extend")
    model.generate(input_ids=tk["prefix"], num_return_sequences=B0, max_new_tokens=N, token_overrides=tk["ovA"], temperature=0.0,
                   shared_cache_op="wipe")
    r1, L1 = torch.tensor(ROWS1, device=DEV), torch.tensor(LENS1, device=DEV)
    used = model.fork(ROWS1, LENS1, tk["ovA"][r1, : max(LENS1)], old_batch=B0, use_kernel=use_kernel, merge_from=1 if first_merged else None)
    assert used == 2
    first1 = tk["ovA"][r1, L1].repeat_interleave(EXPAND, 0)
    model.generate(input_ids=first1[:, None], num_return_sequences=1, max_new_tokens=M1, token_overrides=tk["ovB"], **ext)
    fedB = torch.cat([first1[:, None], tk["ovB"]], dim=1)       # [9, M1 + 1]: cached are the first M1
    r2, L2 = torch.tensor(rows2, device=DEV), torch.tensor(lens2, device=DEV)
    used = model.fork(rows2, lens2, fedB[r2, : max(lens2)], old_batch=len(ROWS1) * EXPAND, use_kernel=use_kernel,
                      merge_from=1 if second == "merged" else None)
    assert used == (2 if second == "merged" else 3) == len(model.shared_bitmaps)
    first2 = fedB[r2, L2]
    k = len(rows2)
    out = model.generate(input_ids=first2.repeat_interleave(2, 0)[:, None], num_return_sequences=1, max_new_tokens=M2, return_logits=True,
                         token_overrides=tk["ovC"][:k].repeat_interleave(2, 0), **ext, **gen_kw)
    paths = [tk["ovA"][ROWS1[r // EXPAND], : LENS1[r // EXPAND]].tolist() + fedB[r, :n].tolist() for r, n in zip(rows2, lens2)]
    return out[0], torch.stack(out[1]), paths, first2


def _unforked(model, tk, paths, first2, **gen_kw):
    """The same tokens in one generate(): the prefix level, then every survivor's path and first uncached token as its own prompt."""
    k = len(paths)
    lens = torch.tensor([len(p) + 1 for p in paths], device=DEV)
    uniq = torch.ones((k, int(lens.max())), dtype=torch.long, device=DEV)
    for i, p in enumerate(paths):
        uniq[i, : len(p) + 1] = torch.tensor(p + [int(first2[i])], device=DEV)
    out = model.generate(input_ids=[tk["prefix"], uniq], seq_lens=[torch.tensor([50], device=DEV), lens], num_return_sequences=1,
                         max_new_tokens=M2, temperature=0.0, return_logits=True, token_overrides=tk["ovC"][:k], shared_cache_op="wipe", **gen_kw)
    return out[0], torch.stack(out[1]), uniq, lens


def _level_state(model, idx):
    out = []
    for layer in model.model.layers:
        sc = layer.self_attn.kv_cache.shared_caches[idx]
        total = int(sc.cumsum_lengths[sc.current_batch_size])
        out.append((_bits(sc.k_cache[:total]).clone(), _bits(sc.v_cache[:total]).clone(), sc.seq_lens[: sc.current_batch_size].clone(),
                    sc.cumsum_lengths[: sc.current_batch_size + 1].clone(), sc.use_varlen, sc.sliced_sequence_length, sc.current_batch_size))
    return out


def _same_state(a, b):
    return all(all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(la, lb)) for la, lb in zip(a, b))


@pytest.mark.parametrize("kind", ["fp16", "bf16", "bf16-fp8kv"])
def test_model_merged_fork_kernel_route_equals_torch_route(kind):
    dtype = torch.float16 if kind == "fp16" else torch.bfloat16
    model = make_model(dtype, head_dim=128, kv_heads=4) if kind != "fp16" else make_model(dtype, head_dim=64, kv_heads=2)
    tk = _tokens(11)
    _setup(model, kv_cache_dtype=FP8 if kind.endswith("fp8kv") else None)
    if kind.endswith("fp8kv"):
        _set_scales(model)
    results = []
    for use_kernel in (True, False):
        _, logits, paths, _ = _twice_forked(model, tk, ROWS2, LENS2, "merged", use_kernel=use_kernel)
        sc = model.model.layers[-1].self_attn.kv_cache.shared_caches[1]
        assert sc.use_varlen and sc.current_batch_size == 4 and sc.seq_lens[:4].tolist() == [len(p) for p in paths]
        assert model.get_num_used_shared_caches() == 2
        results.append((logits, _level_state(model, 1)))
    (la, sa), (lb, sb) = results
    assert _same_state(sa, sb)          # the same level buffers ...
    assert torch.equal(la, lb)          # ... into the same launches: the same logits


@pytest.mark.parametrize("kind", ["fp16", "bf16-fp8kv"])
def test_merge_from_the_end_of_the_chain_is_the_plain_fork(kind):
    """merge_from == levels in use: a chain of no levels.  The same level bytes and bookkeeping as fork() and the same logits --
    for the first fork behind the prompt, and for a second one behind the first."""
    dtype = torch.float16 if kind == "fp16" else torch.bfloat16
    model = make_model(dtype, head_dim=64, kv_heads=2) if kind == "fp16" else make_model(dtype, head_dim=128, kv_heads=4)
    tk = _tokens(13)
    _setup(model, kv_cache_dtype=FP8 if kind.endswith("fp8kv") else None)
    if kind.endswith("fp8kv"):
        _set_scales(model)
    results = []
    for first_merged in (False, True):
        _, logits, _, _ = _twice_forked(model, tk, ROWS2_REGULAR, LENS2_REGULAR, "chain", first_merged=first_merged)
        results.append((logits, _level_state(model, 1), _level_state(model, 2), [b.clone() for b in model.shared_bitmaps]))
    (la, a1, a2, ba), (lb, b1, b2, bb) = results
    assert _same_state(a1, b1) and _same_state(a2, b2) and torch.equal(la, lb)
    assert len(ba) == len(bb) == 3 and all(torch.equal(x, y) for x, y in zip(ba, bb))
    # the second fork as merge_from == 2 (a chain of no levels behind two levels in use)
    ext = dict(temperature=0.0, shared_cache_op="extend")
    outs = []
    for merge in (None, 2):
        model.generate(input_ids=tk["prefix"], num_return_sequences=B0, max_new_tokens=N, token_overrides=tk["ovA"], temperature=0.0, shared_cache_op="wipe")
        r1, L1 = torch.tensor(ROWS1, device=DEV), torch.tensor(LENS1, device=DEV)
        model.fork(ROWS1, LENS1, tk["ovA"][r1, : max(LENS1)], old_batch=B0)
        first1 = tk["ovA"][r1, L1].repeat_interleave(EXPAND, 0)
        model.generate(input_ids=first1[:, None], num_return_sequences=1, max_new_tokens=M1, token_overrides=tk["ovB"], **ext)
        fedB = torch.cat([first1[:, None], tk["ovB"]], dim=1)
        r2, L2 = torch.tensor(ROWS2_REGULAR, device=DEV), torch.tensor(LENS2_REGULAR, device=DEV)
        assert model.fork(ROWS2_REGULAR, LENS2_REGULAR, fedB[r2, : max(LENS2_REGULAR)], old_batch=9, merge_from=merge) == 3
        _, lg = model.generate(input_ids=fedB[r2, L2].repeat_interleave(2, 0)[:, None], num_return_sequences=1, max_new_tokens=M2,
                               return_logits=True, token_overrides=tk["ovC"][:3].repeat_interleave(2, 0), **ext)
        outs.append((torch.stack(lg), _level_state(model, 2)))
    assert torch.equal(outs[0][0], outs[1][0]) and _same_state(outs[0][1], outs[1][1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("geom", [(128, 4), (64, 2)])
def test_merged_hierarchy_against_unforked_decode(dtype, geom):
    """The decomposition check of test_forked_hierarchy_against_unforked_decode, with its bound, on a hierarchy forked twice with
    uneven survivors (three children of one path, none of another): prefix level + ONE merged level + the children's own keys
    against the same tokens decoded in one generate() (prefix level + unique keys).  Where the selection is regular, also
    against the chain-fork route (prefix + two promoted levels).  The children of one survivor are bit-identical to each other."""
    bound = 0.02 if dtype == torch.float16 else 0.08
    model = make_model(dtype, head_dim=geom[0], kv_heads=geom[1])
    tk = _tokens(5)
    _setup(model)
    for rows2, lens2 in ((ROWS2, LENS2), (ROWS2_REGULAR, LENS2_REGULAR)):
        _, b, paths, first2 = _twice_forked(model, tk, rows2, lens2, "merged")
        assert model.get_num_used_shared_caches() == 2
        assert torch.equal(b[:, 0::2], b[:, 1::2])     # the two children of one survivor
        _, a, _, _ = _unforked(model, tk, paths, first2)
        err = rdiff(b[:, 0::2], a).mean()
        print(f"merged vs unforked {dtype} {geom} rows {rows2}: mean rdiff {float(err):.5f} (bound {bound})")
        assert err < bound
        if rows2 is ROWS2_REGULAR:
            _, c, paths_c, _ = _twice_forked(model, tk, rows2, lens2, "chain")
            assert paths_c == paths and model.get_num_used_shared_caches() == 3
            err = rdiff(b, c).mean()
            print(f"merged vs chain {dtype} {geom}: mean rdiff {float(err):.5f} (bound {bound})")
            assert err < bound
        else:
            with pytest.raises(ValueError, match="level 1"):   # the chain fork refuses the uneven selection
                _twice_forked(model, tk, rows2, lens2, "chain")
        model.empty_shared_cache()


# ---- 3. penalties -----------------------------------------------------------------------------------------------------------
def test_merged_bitmap_is_the_paths_token_set_and_penalised_draws_agree():
    """After two merged forks shared_bitmaps[1] is token_bitmap of the full paths.  A repetition_penalty draw without noise
    (temperature 0) on the merged hierarchy equals the draw of the unforked hierarchy's penalised route, row for row, wherever
    the penalised top-2 margin exceeds twice the largest logit difference between the two decompositions; and it is the greedy
    token of the definition (sampling.penalize_logits) on the merged hierarchy's own logits with the merged bitmap."""
    from hydragen_amd import layer_ops, sampling

    model = make_model(torch.float16, head_dim=64, kv_heads=2)
    tk = _tokens(17)
    tk = {n: (t % 24 + 1) for n, t in tk.items()}      # a small range: many repeats, the penalty decides
    _setup(model)
    import math

    # only tokens 0 .. 31 can be drawn: most of them sit in some path, so the penalty decides the draw, path by path
    ban = torch.arange(32, 512, device=DEV)
    bias = (ban, torch.full((ban.numel(),), -math.inf, device=DEV))
    pen = dict(repetition_penalty=1.7, logit_bias=bias)
    out_f, lg_f, paths, first2 = _twice_forked(model, tk, ROWS2, LENS2, "merged", first_merged=True, **pen)
    assert len(model.shared_bitmaps) == 2
    k, V = len(paths), model.vocab_size
    ids = torch.zeros((k, max(len(p) for p in paths)), dtype=torch.long, device=DEV)
    for i, p in enumerate(paths):
        ids[i, : len(p)] = torch.tensor(p, device=DEV)
    plen = torch.tensor([len(p) for p in paths], device=DEV)
    merged_bits = model.shared_bitmaps[1].clone()
    assert torch.equal(merged_bits, layer_ops.token_bitmap(ids, plen, V))
    prefix_bits = model.shared_bitmaps[0].clone()
    out_u, lg_u, _, _ = _unforked(model, tk, paths, first2, **pen)
    ov = tk["ovC"][:k]
    gap = float((lg_f[:, 0::2] - lg_u).abs().max())
    skipped = 0
    for j in range(M2):
        gen, gl = ov[:, :j].to(torch.int32), torch.full((k,), j, dtype=torch.int32, device=DEV)
        ctx = [(prefix_bits, k), (merged_bits, 1), (layer_ops.token_bitmap(first2[:, None], None, V), 1)]
        x_f = sampling.penalize_logits(lg_f[j, 0::2], 1.7, logit_bias=bias, context=ctx, gen=gen, gen_len=gl)
        x_u = sampling.penalize_logits(lg_u[j], 1.7, logit_bias=bias, context=ctx, gen=gen, gen_len=gl)
        top_f, top_u = x_f.double().topk(2, dim=-1).values, x_u.double().topk(2, dim=-1).values
        safe = ((top_f[:, 0] - top_f[:, 1]) > 2 * gap + 1e-6) & ((top_u[:, 0] - top_u[:, 1]) > 2 * gap + 1e-6)
        skipped += int((~safe).sum())
        assert torch.equal(out_f[0::2, j][safe], out_u[:, j][safe])
        assert torch.equal(out_f[0::2, j][safe], x_f.argmax(-1)[safe])
        assert torch.equal(out_f[0::2, j], out_f[1::2, j])
    print(f"penalised draws: {k * M2 - skipped} of {k * M2} rows compared (largest logit difference {gap:.4f})")
    assert skipped <= k * M2 // 2
    # the penalty acted: some unpenalised greedy token differs
    plain, _, _, _ = _unforked(model, tk, paths, first2, logit_bias=bias)
    assert not torch.equal(plain, out_u) and bool((out_u < 32).all())


# ---- 4. graph replay --------------------------------------------------------------------------------------------------------
def test_merged_forks_replay_the_captured_graph():
    """Two rounds of (unique prefill, plain fork, unique prefill of the children, MERGED fork of uneven survivors, decode) with the
    same shapes and different ragged lengths on a graphed model: the second round replays the graph the first one captured -- the
    merged level sits in slot 1's own buffers, and the key (batch sizes, varlen flags, sliced lengths) is the same -- and each
    round's logits are bit-identical to the same round on an eager model with the same weights."""
    eager, graphed = make_model(torch.bfloat16, head_dim=128, kv_heads=4), make_model(torch.bfloat16, head_dim=128, kv_heads=4)
    graphed.graph(True)
    g = torch.Generator(device=DEV).manual_seed(21)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    prefix, B, n, m = rnd(1, 50), 6, 10, 5
    uniq, kids, ov = rnd(B, n), rnd(6, n), rnd(8, m + 1)
    for mdl in (eager, graphed):
        mdl.setup_caches(max_unique_batch_size=8, max_unique_seq_length=32, max_shared_batch_sizes=[1, 4, 3], max_shared_seq_lengths=[50, 24, n])
    rows1, rows2 = [4, 1, 2], [0, 1, 4, 5]     # children 0, 1 of survivor 0; none of survivor 1; both of survivor 2
    captured = None
    for lens1, lens2 in (([9, 4, 7], [3, 10, 6, 1]), ([3, 10, 6], [8, 2, 5, 9])):
        out = []
        for mdl in (eager, graphed):
            mdl.generate(input_ids=[prefix, uniq], num_return_sequences=1, max_new_tokens=1, temperature=0.0, shared_cache_op="wipe")
            r1 = torch.tensor(rows1, device=DEV)
            assert mdl.fork(rows1, lens1, uniq[r1, : max(lens1)], old_batch=B) == 2
            mdl.generate(input_ids=kids, num_return_sequences=1, max_new_tokens=1, temperature=0.0, shared_cache_op="extend")
            r2 = torch.tensor(rows2, device=DEV)
            assert mdl.fork(rows2, lens2, kids[r2, : max(lens2)], old_batch=6, merge_from=1) == 2
            _, logits = mdl.generate(input_ids=ov[:, :1], num_return_sequences=1, max_new_tokens=m, temperature=0.0, return_logits=True,
                                     token_overrides=ov[:, 1:], shared_cache_op="extend")
            out.append(torch.stack(logits))
        assert torch.equal(out[0], out[1]), (lens1, lens2)
        cd = graphed.graphed_model.capture_data
        assert cd is not None
        if captured is None:
            captured = cd
        assert cd is captured, "the second merged fork re-captured the decode graph"


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2])
def test_beam_search_over_prompts_is_consistent_with_its_trace(G):
    from hydragen_amd.fork import select_beams, stepwise_beam_search

    width, expand, T, steps = 2, 3, 4, 10
    model = make_model(torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(31 + G)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    levels = rnd(1, 20) if G == 1 else [rnd(1, 20), rnd(2, 7)]
    # the prompt's levels and ONE more: G * width paths of up to (steps - 1) * T tokens
    sb = [1, 2] if G == 1 else [1, 2, 4]
    sl = [20, (steps - 1) * T] if G == 1 else [20, 7, (steps - 1) * T]
    model.setup_caches(max_unique_batch_size=G * width * expand, max_unique_seq_length=16, max_shared_batch_sizes=sb, max_shared_seq_lengths=sl)
    before = model.get_num_used_shared_caches()
    rounds = []

    def one_parent(tok, lp):
        """Every survivor of a round hangs off ONE path of its prompt: the path alternates with the round."""
        rnd_no = tok.shape[1] // T - 1
        rounds.append(rnd_no)
        r = torch.arange(tok.shape[0], device=lp.device)
        bonus = (((r % (width * expand)) // expand) == (rnd_no % width)).float() * 1000.0
        return lp.sum(1) + bonus

    tokens, scores, trace = stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=steps, score_fn=one_parent,
                                                 return_trace=True, select="prompt", temperature=1.0)
    assert model.get_num_used_shared_caches() == before == len(model.shared_bitmaps)
    assert rounds == list(range(steps))
    assert tokens.shape == (G * width, steps * T) and scores.shape == (G * width,) and len(trace) == steps
    paths = lps = None
    for s, t in enumerate(trace):
        assert (t["group_size"], t["width"]) == (width * expand, width) and t["candidate_scores"].shape == (G * width * expand,)
        assert t["rows"].tolist() == select_beams(t["candidate_scores"], 6, 2).tolist()
        assert t["parents"].tolist() == (t["rows"] // (width * expand if s == 0 else expand)).tolist()
        if s > 0:   # both survivors of a prompt are children of the SAME path: what the chain form cannot keep
            par = t["parents"].reshape(G, width)
            assert bool((par[:, 0] == par[:, 1]).all()) and par[:, 0].tolist() == [gi * width + s % width for gi in range(G)]
        assert t["tokens"].shape == (G * width, T) and t["logprobs"].shape == (G * width, T)
        paths = t["tokens"] if s == 0 else torch.cat([paths[t["parents"]], t["tokens"]], dim=1)
        lps = t["logprobs"] if s == 0 else torch.cat([lps[t["parents"]], t["logprobs"]], dim=1)
        # the kept candidates' scores are the scorer's: the sums of their paths' per-round log-probs plus the round's bonus
        assert torch.allclose(t["candidate_scores"][t["rows"]], lps.sum(1) + 1000.0, atol=1e-2, rtol=1e-5)
    assert torch.equal(tokens.cpu(), paths)
    assert torch.allclose(scores.cpu(), lps.sum(1) + 1000.0, atol=1e-2, rtol=1e-5)
    assert bool((lps <= 0).all()) and bool(lps.isfinite().all())

    # the chain form needs a level per round: on these caches it runs out of them, and leaves the count as it was
    with pytest.raises(ValueError, match="No more available shared caches"):
        stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=steps, temperature=1.0)
    assert model.get_num_used_shared_caches() == before == len(model.shared_bitmaps)

    calls = []

    def failing(tok, lp):
        calls.append(tok.shape)
        if len(calls) == 3:
            raise RuntimeError("scorer failed")
        return lp.sum(1)

    with pytest.raises(RuntimeError, match="scorer failed"):
        stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=steps, score_fn=failing, select="prompt", temperature=1.0)
    assert calls == [(G * width * expand, T), (G * width * expand, 2 * T), (G * width * expand, 3 * T)]
    assert model.get_num_used_shared_caches() == before == len(model.shared_bitmaps)
    with pytest.raises(ValueError, match="select"):
        stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=2, select="global")


def test_select_path_is_the_default_and_unchanged():
    """select="path" is the call without the argument: the same tokens, scores and trace on the same seed -- one best child per
    path (group_size = expand, width = 1 from round 1 on), one level per round."""
    from hydragen_amd.fork import stepwise_beam_search

    width, expand, T, steps = 2, 3, 4, 3
    model = make_model(torch.bfloat16)
    levels = torch.randint(1, 512, (1, 20), device=DEV, generator=torch.Generator(device=DEV).manual_seed(32))
    model.setup_caches(max_unique_batch_size=width * expand, max_unique_seq_length=16, max_shared_batch_sizes=[1, 2, 2], max_shared_seq_lengths=[20, T, T])
    res = []
    for kw in ({}, dict(select="path")):
        torch.manual_seed(5)
        res.append(stepwise_beam_search(model, levels, width=width, expand=expand, step_tokens=T, steps=steps, return_trace=True, temperature=1.0, **kw))
    (ta, sa, tra), (tb, sb, trb) = res
    assert torch.equal(ta, tb) and torch.equal(sa, sb)
    for a, b in zip(tra, trb):
        assert a.keys() == b.keys() and all(torch.equal(a[n], b[n]) if isinstance(a[n], torch.Tensor) else a[n] == b[n] for n in a)
    assert [(t["group_size"], t["width"]) for t in tra] == [(6, 2), (3, 1), (3, 1)]
    assert all(t["parents"].tolist() == (t["rows"] // t["group_size"]).tolist() for t in tra)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_merged_fork_refusals_leave_levels_and_bitmaps_alone():
    model = make_model(torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(41)
    rnd = lambda *s: torch.randint(1, 512, s, device=DEV, generator=g)
    p0, p1, n, m = rnd(1, 20), rnd(2, 7), 6, 5
    ovA, ovB = rnd(12, n), rnd(12, m)
    # two prompts, a path level of 4 sequences of at most 9 tokens, one more level
    model.setup_caches(max_unique_batch_size=12, max_unique_seq_length=16, max_shared_batch_sizes=[1, 2, 4, 4], max_shared_seq_lengths=[20, 7, 9, 8])
    model.generate(input_ids=[p0, p1], num_return_sequences=6, max_new_tokens=n, temperature=0.0, token_overrides=ovA, shared_cache_op="extend")
    rows1 = [1, 4, 6, 11]
    r1 = torch.tensor(rows1, device=DEV)
    assert model.fork(rows1, [n - 1] * 4, ovA[r1, : n - 1], old_batch=12) == 3
    first = ovA[r1, n - 1].repeat_interleave(3, 0)
    model.generate(input_ids=first[:, None], num_return_sequences=1, max_new_tokens=m, temperature=0.0, token_overrides=ovB, shared_cache_op="extend")
    fed = torch.cat([first[:, None], ovB], dim=1)
    kvs = [layer.self_attn.kv_cache for layer in model.model.layers]

    def snap():
        return (model.get_num_used_shared_caches(), len(model.shared_bitmaps), [b.clone() for b in model.shared_bitmaps],
                [(c.k_cache.clone(), c.v_cache.clone(), c.seq_lens.clone(), c.cumsum_lengths.clone(), c.current_batch_size, c.use_varlen,
                  c.sliced_sequence_length) for kv in kvs for c in kv.shared_caches])

    def unchanged(s):
        now = snap()
        assert now[:2] == s[:2] and all(torch.equal(a, b) for a, b in zip(now[2], s[2]))
        for a, b in zip(now[3], s[3]):
            assert all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))

    s0 = snap()
    assert s0[:2] == (3, 3)
    ids = lambda rows, L: fed[torch.tensor(rows, device=DEV), :L]
    for rows, lens, merge, frag in (([0, 1, 6, 7], [2] * 4, 4, "merge_from 4"),
                                    ([0, 1, 6, 7], [2] * 4, -1, "merge_from -1"),
                                    ([0, 1, 6, 7], [2] * 4, True, "merge_from True"),
                                    ([0, 1, 6, 7], [2, 2, 2, 5], 2, "Sequence length 10 exceeds max sequence length 9"),   # 5 + 5 tokens
                                    ([0, 1, 2, 6, 7, 8], [2] * 6, 2, "Batch size 6 exceeds max batch size 4"),
                                    ([0, 6, 7, 8], [2] * 4, 2, r"level 1: rows\[1\] = 6"),                               # crosses a prompt group
                                    ([0, 0, 6, 7], [2] * 4, 2, "repeats"),
                                    ([0, 1, 6, 12], [2] * 4, 2, "outside the previous batch"),
                                    ([0, 1, 6, 7], [2, 2, 2, 17], 2, "at most the 16 tokens")):
        with pytest.raises(ValueError, match=frag):
            model.fork(rows, lens, ids([min(r, 11) for r in rows], max(lens)), old_batch=12, merge_from=merge)
        unchanged(s0)
    with pytest.raises(ValueError, match="token_ids"):
        model.fork([0, 1, 6, 7], [2, 3, 2, 2], ids([0, 1, 6, 7], 2), old_batch=12, merge_from=2)
    unchanged(s0)
    # both survivors of each prompt from one path: the plain fork refuses, the merged one takes it
    with pytest.raises(ValueError, match="level 2"):
        model.fork([0, 1, 6, 7], [2, 3, 4, 1], ids([0, 1, 6, 7], 4), old_batch=12)
    unchanged(s0)
    assert model.fork([0, 1, 6, 7], [2, 3, 4, 1], ids([0, 1, 6, 7], 4), old_batch=12, merge_from=2) == 3
    sc = kvs[0].shared_caches[2]
    assert sc.current_batch_size == 4 and sc.seq_lens[:4].tolist() == [7, 8, 9, 6] and len(model.shared_bitmaps) == 3
