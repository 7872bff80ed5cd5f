"""GPU: the prologue, split-layout, row-movement, transpose / cast and mask kernels through the C ABI, bit for bit against the exact
reference of tests/layout_ref.py, every output inside sentinel canaries that must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import layout_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I32 = 0x5A5A5A5A
CANARY_F32 = 0x7FA5A5A5              # a NaN bit pattern no output takes
PAD = 64


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    return o


def lib():
    from msa_amd import _lib
    return _lib.load()


def check(code, what):
    assert code == 0, (what, code)


def i32_buf(n):
    return torch.full((n + PAD,), CANARY_I32, dtype=torch.int32, device=DEV)


def f32_buf(n):
    return torch.full((n + PAD,), CANARY_F32, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    """Host numpy bit patterns of a device tensor (floats as unsigned integers of their width)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def expect_ints(got, want):
    """``got`` an int32 canary buffer, ``want`` its first values; every entry behind them keeps the canary."""
    g = bits(got).astype(np.int64)
    want = np.asarray(want, dtype=np.int64)
    n = len(want)
    assert np.array_equal(g[:n], want), np.nonzero(g[:n] != want)[0][:10]
    assert (g[n:] == CANARY_I32).all(), f"{int((g[n:] != CANARY_I32).sum())} canary entries changed"


# ------------------------------------------------------------------------------------------------ prologue
DTYPES = [torch.float64, torch.int64, torch.float32, torch.int32, torch.bfloat16, torch.uint8, torch.bool, torch.float16]


def _device_mask(arr, dtype, layout):
    """A [B, n] device mask holding ``arr`` in ``dtype`` with a given stride layout: plain, feature 0 of [B, n, D], transposed storage."""
    t = torch.from_numpy(arr)
    t = t.to(dtype) if dtype != torch.bool else t != 0
    B, n = t.shape
    if layout == "feat":
        big = torch.zeros(B, n, 5, dtype=t.dtype)
        big[:, :, 0] = t
        return big.to(DEV)[:, :, 0]
    if layout == "trans":
        return t.t().contiguous().to(DEV).t()
    return t.to(DEV)


def _stored_f32(t):
    """The fp32 value the kernel reads from a device mask: float64 rounds (numpy RNE), every other dtype here converts exactly."""
    if t.dtype == torch.float64:
        return t.cpu().numpy().astype(np.float32)
    return t.cpu().float().numpy()


def _step_masks(name, segs):
    """Device masks of a case: the real step's dtypes and strides for the step-shaped cases, a sweep of dtypes and strides otherwise."""
    out = []
    for j, (arr, p, off) in enumerate(segs):
        if name in ("headline", "bert_large", "b128"):
            dtype = torch.float64 if p < 2 else torch.int64
            layout = "feat" if off > 0 else "plain"
        elif name.startswith("frac"):
            dtype, layout = [torch.float64, torch.float32, torch.float16, torch.bfloat16][j % 4], ["plain", "trans"][j % 2]
        else:
            dtype, layout = DTYPES[j % len(DTYPES)], ["plain", "feat", "trans"][j % 3]
        out.append((_device_mask(arr, dtype, layout), p, off))
    return out


def _run_prologue(ops, name, rowset, use_bufs):
    segs, lens, B, labels, V, _ = L.prologue_case(name)
    dsegs = _step_masks(name, segs)
    ref = L.prologue_ref([(_stored_f32(m), p, o) for m, p, o in dsegs], lens, B, labels, V, rowset)
    lab_d = torch.from_numpy(labels).to(DEV) if labels is not None else None
    nf, ni = ops.prologue_sizes(lens, B, rowset)
    fb, ib = f32_buf(nf), i32_buf(ni)
    pro = ops.prologue(dsegs, lens, B, lab_d, V, DEV, bufs=(fb, ib) if use_bufs else None, rowset=rowset)
    torch.cuda.synchronize()
    tokens = B * sum(lens)
    n = len(ref["idx"])
    if use_bufs:
        kbs = [ref["key_bias"]] + ([ref["key_bias_perm"]] if rowset else [])
        want_f = L.f32_bits(np.concatenate(kbs))
        got_f = bits(fb)
        assert np.array_equal(got_f[:want_f.size], want_f), np.nonzero(got_f[:want_f.size] != want_f)[0][:10]
        assert (got_f[want_f.size:] == CANARY_F32).all()
        idx = np.full(max(tokens, 1), CANARY_I32, dtype=np.int64)
        idx[:n] = ref["idx"]
        want_i = np.concatenate([ref["kv_len"], ref["valid"], ref["seq_cnt"], idx, ref["words"]] + ([ref["rank"]] if rowset else []))
        expect_ints(ib, want_i)
    else:
        key_bias = pro.key_bias
        assert np.array_equal(bits(key_bias), L.f32_bits(ref["key_bias_perm"] if rowset else ref["key_bias"]))
        for k in ("kv_len", "valid", "words"):
            assert np.array_equal(bits(getattr(pro, k)).astype(np.int64), ref[k]), k
        assert np.array_equal(bits(pro.idx[:n]).astype(np.int64), ref["idx"])
        if rowset:
            assert np.array_equal(bits(pro.rank).astype(np.int64), ref["rank"])


@pytest.mark.parametrize("name", list(L.PROLOGUE_CASES))
def test_prologue_equals_the_reference_in_both_modes(ops, name):
    rowset = L.PROLOGUE_CASES[name].get("rowset", False)
    _run_prologue(ops, name, rowset, use_bufs=True)
    _run_prologue(ops, name, not rowset, use_bufs=False)


def test_prologue_key_bias_rounds_like_the_reference(ops):
    """(1 - m) * -10000 in two fp32 roundings: m = 3e-8 is a live key (-9999.999) and m = 1 gives -0 (one fma gave -10000 and +0)."""
    m = torch.tensor([[1.0, 0.3, 0.7, 3e-8, 1e-9, 0.123456, 0.999, 0.0]], dtype=torch.float32)
    pro = ops.prologue([(m.to(DEV), 0, 0)], [8], 1, None, 100, DEV)
    want = L.key_bias(m.numpy()[0])
    assert np.array_equal(bits(pro.key_bias[:8]), L.f32_bits(want))
    assert bits(pro.key_bias[:1])[0] == 0x80000000 and int(pro.kv_len[0]) == 7 and float(pro.key_bias[3]) > -10000.0


# ------------------------------------------------------------------------------------------------ split layout and row maps
@pytest.mark.parametrize("name", list(L.SPLIT_CASES))
def test_split_layout_equals_the_reference(ops, name):
    lens, valid, heads = L.split_case(name)
    rows = lib().mmbert_attn_tile_rows(0)
    nq_max = sum((n + rows - 1) // rows for n in lens)
    nf_max = nq_max + len(lens)
    ns = len(lens)
    out = i32_buf(4 * nf_max + 4 * nq_max + 3 * ns + 4)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    vd = torch.tensor(valid, dtype=torch.int32, device=DEV)
    check(lib().mmbert_split_layout(ops._stream(), ln.data_ptr(), vd.data_ptr(), ns, rows, L.xs_of(heads), nf_max, nq_max, out.data_ptr()),
          "mmbert_split_layout")
    torch.cuda.synchronize()
    expect_ints(out, L.split_layout_ref(lens, valid, heads, rows, nf_max, nq_max))
    # DeviceSplitLayout (mode 0) with and without a rank: its row maps against the reference
    base = ops.SeqLayout(lens, heads, DEV)
    for use_rank in (False, True):
        rank = L.seq_ranks(lens, 9) if use_rank else None
        rk = torch.from_numpy(rank.astype(np.int32)).to(DEV) if use_rank else None
        d = ops.DeviceSplitLayout(base, vd, DEV, rank=rk)
        perm, inv, owned, _ = L.split_rows_ref(lens, valid, 0, rank)
        assert owned.all()
        for got, want in ((d.perm, perm), (d.inv, inv), (d.perm32, perm), (d.inv32, inv)):
            assert np.array_equal(bits(got).astype(np.int64), want)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("use_rank", [False, True])
def test_split_rows_every_mode_equals_the_reference(ops, mode, use_rank):
    lens, valid, heads = L.split_case("three_heads_zero")
    lens, valid = lens + [50] * 48, valid + [int(v) for v in np.random.default_rng(2).integers(0, 60, size=48)]
    rank = L.seq_ranks(lens, 4) if use_rank else None
    perm, inv, owned, st = L.split_rows_ref(lens, valid, mode, rank)
    M, npk = sum(lens), st["n_packed"]
    rs = torch.from_numpy(np.repeat(np.arange(len(lens)), lens)).to(DEV)
    rp = torch.from_numpy(np.concatenate([np.arange(n) for n in lens])).to(DEV)
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)
    sa, sb, v = i32(st["start_a"]), i32(st["start_b"]), i32(st["v"])
    rk = i32(rank) if use_rank else None
    p64, i64 = (torch.full((n + PAD,), CANARY_I32, dtype=torch.int64, device=DEV) for n in (npk, M))
    p32, i32b = i32_buf(npk), i32_buf(M)
    check(lib().mmbert_split_rows(ops._stream(), rs.data_ptr(), rp.data_ptr(), sa.data_ptr(), sb.data_ptr(), v.data_ptr(), mode, M, st["rows_a"],
                                  p64.data_ptr(), i64.data_ptr(), ops._ptr(rk), p32.data_ptr(), i32b.data_ptr()), "mmbert_split_rows")
    torch.cuda.synchronize()
    want_p = np.where(owned, perm, CANARY_I32)
    for buf, want in ((p64, want_p), (i64, inv)):
        g = bits(buf)
        assert np.array_equal(g[:len(want)], want) and (g[len(want):] == CANARY_I32).all()
    expect_ints(p32, want_p)
    expect_ints(i32b, inv)


# ------------------------------------------------------------------------------------------------ row movement
@pytest.mark.parametrize("M", L.ACTIVE_M)
def test_active_rows_equals_the_reference(ops, M):
    lab = L.active_labels(M)
    want = L.active_rows_ref(lab, 30522)
    idx, cnt = i32_buf(max(M, 1)), i32_buf(1)
    labels = torch.from_numpy(lab).to(DEV) if M else torch.zeros(1, dtype=torch.int64, device=DEV)
    check(lib().mmbert_active_rows(ops._stream(), labels.data_ptr(), M, 30522, idx.data_ptr(), cnt.data_ptr()), "mmbert_active_rows")
    torch.cuda.synchronize()
    expect_ints(cnt, [len(want)])
    expect_ints(idx, want)


def test_compact_rows_stamped_inverse_and_scatter_across_the_stamp_wrap(ops):
    """int32 / int64 lists, ``extra`` only, a list pointing past ``nrows``, four matrices of different widths; the stamp set just below
    0xFFFFFFF0 and advanced past the wrap; an entry index >= nlist reads as a zero row."""
    rng = np.random.default_rng(8)
    N = 3000
    mp = rng.permutation(N)
    mp_d = torch.from_numpy(mp).to(DEV)
    rinv = ops.RowInverse(N, DEV)
    rinv.stamp = 0xFFFFFFEE
    table = np.zeros(N, dtype=np.int64)
    widths = [(768, torch.bfloat16), (36, torch.float32), (4, torch.float32), (1024, torch.float32)]
    for n, ne, width in ((400, 6, torch.int32), (3, 2, torch.int64), (0, 5, torch.int32), (250, 0, torch.int64)):
        pick = rng.permutation(N)[:n + ne]
        rows = torch.from_numpy(pick[:n]).to(width).to(DEV)
        extra = torch.from_numpy(pick[n:]).long().to(DEV)
        want = L.compact_ref(pick[:n], pick[n:], mp)
        r64, r32 = ops.compact_rows(rows, extra, mp_d, inverse=rinv)
        assert np.array_equal(bits(r64), want) and np.array_equal(bits(r32).astype(np.int64), want)
        table = L.stamp_table_ref(table, want, rinv.stamp)
        torch.cuda.synchronize()
        assert np.array_equal(bits(rinv.table), table), rinv.stamp
        srcs = [torch.randn(n + ne, w, device=DEV).to(dt) for w, dt in widths]
        nrows = N - 400                                               # (the list points past the rows asked for too)
        for nl in ((n + ne, max(n + ne - 3, 0)) if n + ne > 3 else (n + ne,)):
            rinv.nlist = nl
            outs = ops.scatter_rows_zero([s[:nl] for s in srcs], rinv, nrows)
            take = L.scatter_ref(table, rinv.stamp, nl, nrows)
            for s, o in zip(srcs, outs):
                sb = bits(s[:nl]).view(np.uint8).reshape(nl, -1) if nl else np.zeros((0, o.shape[1] * o.element_size()), np.uint8)
                w = L.copy_rows(sb, take) if nl else np.zeros((nrows, sb.shape[1]), np.uint8)
                assert np.array_equal(bits(o).view(np.uint8).reshape(nrows, -1), w)
    assert rinv.stamp < 0xFFFFFFEE                                    # the wrap happened


def _gather_direct(ops, srcs, idx, dst_extra):
    """mmbert_gather_rows on uint8 [rows, row_bytes] views; destinations with ``dst_extra`` canary bytes behind every row."""
    n, k = idx.numel(), len(srcs)
    dsts = [torch.full((n, s.shape[1] + dst_extra), 0xA5, dtype=torch.uint8, device=DEV) for s in srcs]
    PA, LA, IA = ctypes.c_void_p * k, ctypes.c_longlong * k, ctypes.c_int * k
    check(lib().mmbert_gather_rows(ops._stream(), k, PA(*[s.data_ptr() for s in srcs]), PA(*[d.data_ptr() for d in dsts]), LA(*[s.stride(0) for s in srcs]),
                                   LA(*[d.stride(0) for d in dsts]), IA(*[s.shape[1] for s in srcs]), idx.data_ptr(), n), "mmbert_gather_rows")
    return dsts


def test_gather_rows_every_width_both_paths_twelve_segments(ops):
    rng = np.random.default_rng(12)
    M = 700
    idx_np = rng.integers(0, M, size=66000)
    idx_np[:50] = 3                                                   # repeated rows
    idx = torch.from_numpy(idx_np.astype(np.int32)).to(DEV)
    srcs, hosts = [], []
    for j, (width, off) in enumerate([(4, 0), (12, 4), (16, 0), (16, 4), (1536, 0), (6144, 0), (20, 8), (48, 16), (1536, 4), (8, 0), (64, 32), (4, 12)]):
        pitch = width + 32 + (4 if off else 0)                       # a pitch off 16 bytes or an offset off 16: the 4-byte path
        base = torch.from_numpy(rng.integers(0, 256, size=(M, pitch), dtype=np.uint8)).to(DEV)
        srcs.append(base[:, off:off + width])
        hosts.append(bits(base)[:, off:off + width])
    dsts = _gather_direct(ops, srcs, idx, dst_extra=16)
    torch.cuda.synchronize()
    for h, d in zip(hosts, dsts):
        got = bits(d)
        assert np.array_equal(got[:, :h.shape[1]], L.copy_rows(h, idx_np))
        assert (got[:, h.shape[1]:] == 0xA5).all()


def test_pack_i64_fill_segments_and_counts_past_the_grid(ops):
    segs = L.pack_case()
    want = L.pack_ref(segs)
    k = len(segs)
    dev = [torch.from_numpy(s).to(DEV) if not isinstance(s, tuple) else None for s in segs]
    cnts = [len(s) if not isinstance(s, tuple) else s[0] for s in segs]
    offs = np.concatenate(([0], np.cumsum(cnts)[:-1])).tolist()
    out = torch.full((want.size + PAD,), CANARY_I32, dtype=torch.int64, device=DEV)
    PA, LA = ctypes.c_void_p * k, ctypes.c_longlong * k
    check(lib().mmbert_pack_i64(ops._stream(), k, PA(*[d.data_ptr() if d is not None else None for d in dev]), LA(*offs), LA(*cnts),
                                LA(*[s[1] if isinstance(s, tuple) else 0 for s in segs]), out.data_ptr()), "mmbert_pack_i64")
    torch.cuda.synchronize()
    g = bits(out)
    assert np.array_equal(g[:want.size], want) and (g[want.size:] == CANARY_I32).all()


# ------------------------------------------------------------------------------------------------ casts and transposes
def test_casts_round_to_nearest_even_keep_subnormals_and_quiet_nans(ops):
    x = L.cast_bits(4096)
    xd = torch.from_numpy(x.view(np.int32)).to(DEV)
    y = torch.full((x.size + PAD,), L.SENTINEL_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    check(lib().mmbert_cast_f32_bf16(ops._stream(), xd.data_ptr(), y.data_ptr(), x.size), "cast")
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    bd = torch.from_numpy(allb.view(np.int16)).to(DEV)
    f = f32_buf(65536)
    check(lib().mmbert_cast_bf16_f32(ops._stream(), bd.data_ptr(), f.data_ptr(), 65536), "cast back")
    torch.cuda.synchronize()
    g = bits(y)
    assert np.array_equal(g[:x.size], L.bf16_rne(x)) and (g[x.size:] == L.SENTINEL_BF16).all()
    gf = bits(f)
    assert np.array_equal(gf[:65536], L.bf16_to_f32_bits(allb)) and (gf[65536:] == CANARY_F32).all()


@pytest.mark.parametrize("which", list(L.TRANSPOSE_CASES))
@pytest.mark.parametrize("bf16src", [False, True])
def test_transpose_synthetic_descriptors(ops, which, bf16src):
    descs, ntiles, src, dst0 = L.transpose_case(which, bf16src)
    want = L.transpose_ref(src, dst0, descs, bf16src)
    s = torch.from_numpy(src.view(np.int16 if bf16src else np.int32)).to(DEV).view(torch.bfloat16 if bf16src else torch.float32)
    d = torch.from_numpy(dst0.view(np.int16)).to(DEV).view(torch.bfloat16)
    ops.transpose_cast(s, d, torch.from_numpy(L.tdesc_raw(descs)).to(DEV), len(descs), ntiles)
    torch.cuda.synchronize()
    got = bits(d)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])


def rne_dev(x):
    """The reference's bit rule on the device (torch integer ops): fp32 -> bf16 bits as int32."""
    b = x.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, (b >> 16) | 0x40, ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).int()


def bf_bits_dev(t):
    return t.contiguous().view(torch.int16).int() & 0xFFFF


def _check_flat(flat):
    torch.cuda.synchronize()
    assert torch.equal(bf_bits_dev(flat.half), rne_dev(flat.params))
    for key, (so, do, r, c, ld, _) in zip(flat.t_off, flat._desc_list):
        tv = flat.tview(key)                                          # [cols, ld]
        want = rne_dev(flat.params[so:so + r * c].view(r, c)).t()
        got = bf_bits_dev(tv)
        assert torch.equal(got[:, :r], want), key
        assert not bool(got[:, r:].any()), key                        # padding columns: zero


MODELS = {
    "headline_L12": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=30522),
    "bert_large_L24": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, vocab_size=30522),
    "golden_H128": dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512, vocab_size=30522),
    "golden_H64": dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128, vocab_size=2048),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_flat_transposed_copies_equal_the_rounded_transpose(ops, name):
    """FlatParams at the model's shapes: after refresh() (special values planted in every weight) and after one AdamW step whose
    transposed copies run on the side stream, every tview(key) is RNE(W).T bit for bit with zero padding columns, and half = RNE(params)."""
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    from msa_amd.trainer import build_optimizer, default_args
    with torch.device(DEV):
        m = MMBertForPretraining(MMBertConfig(**MODELS[name]))
    m.bert.set_joint_embeddings("mosei")
    m.to(DEV)
    m._ensure_ready(DEV)
    flat = m._flat
    flat._desc_list = [tuple(int(v) for v in row[:2]) + (int(row[2]) & 0xFFFFFFFF, int(row[2]) >> 32, int(row[3]) & 0xFFFFFFFF, int(row[3]) >> 32)
                       for row in flat._descs.cpu().numpy()]
    assert len(flat._desc_list) == 4 * MODELS[name]["num_hidden_layers"] + 2
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        flat.params.normal_(0.0, 0.05, generator=g)
        sp = torch.from_numpy(L.SPECIAL_F32.view(np.int32)).to(DEV).view(torch.float32)
        for so, _, r, c, _, _ in flat._desc_list:                     # specials at the start and the end of every matrix
            flat.params[so:so + sp.numel()] = sp
            flat.params[so + r * c - sp.numel():so + r * c] = sp
    flat.refresh()
    _check_flat(flat)
    with torch.no_grad():
        flat.params.normal_(0.0, 0.05, generator=g)
    flat.refresh()
    opt, sched = build_optimizer(m, default_args(learning_rate=1e-3), 10)
    sched.step()
    with torch.no_grad():
        flat.grads.normal_(0.0, 1.0, generator=g)
    flat.grads_dirty = True
    opt.step()
    flat.wait_transposes()
    _check_flat(flat)


# ------------------------------------------------------------------------------------------------ masks
def test_dropout_mask_past_the_grid_cap_equals_the_rng_model(ops):
    for seed, site, p in ((1234, 17, 0.1), (7, 3, 0.5)):
        drop = ops.make_drop(p, seed, site)
        assert drop[0] == L.rng_stream(seed, site) and drop[1] == L.dropout_thr16(p)
        out = torch.full((L.DROPOUT_N + PAD,), 0xEE, dtype=torch.uint8, device=DEV)
        check(lib().mmbert_dropout_mask(ops._stream(), out.data_ptr(), L.DROPOUT_N, drop[0], drop[1]), "mmbert_dropout_mask")
        torch.cuda.synchronize()
        g = bits(out)
        assert np.array_equal(g[:L.DROPOUT_N], L.dropout_mask_ref(L.DROPOUT_N, drop[0], drop[1])) and (g[L.DROPOUT_N:] == 0xEE).all()


@pytest.mark.parametrize("nspecial", [0, 1, 2, 3])
def test_mlm_mask_equals_the_rng_model(ops, nspecial):
    ids0 = L.mlm_ids(L.MLM_N, seed=nspecial)
    special = [101, 102, 0][:nspecial]
    for p_sel, p_rep in ((0.15, 0.8), (0.0, 0.8), (1.0, 0.0), (1.0, 1.0), (0.15, 1.0)):
        if nspecial < 3 and (p_sel, p_rep) != (0.15, 0.8):
            continue
        ids = torch.from_numpy(ids0).to(DEV)
        labels = ops.mlm_mask(ids, p_sel, 99, special_ids=special, mask_id=103, p_replace=p_rep)
        torch.cuda.synchronize()
        want_ids, want_lab = L.mlm_ref(ids0, L.rng_stream(99, 4242), round(p_sel * 65536), round(p_rep * 65536), L.mlm_specials(special), 103)
        assert np.array_equal(bits(ids), want_ids) and np.array_equal(bits(labels), want_lab), (p_sel, p_rep)


def test_attention_dropout_mask_at_the_fused_shape(ops):
    S, heads = 1050, 12
    base = ops.SeqLayout([S] * 4, heads, DEV)
    eb = base.elem_base_host[3]
    drop = ops.make_drop(0.1, 42, 9)
    got = ops.attn_dropout_mask(S, eb, 11, drop, DEV)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), L.attn_dropout_mask_ref(S, eb, 11, drop[0], drop[1]))
