"""CPU: the exact reference of tests/layout_ref.py against forms independent of it, its ports against it at every shape the GPU
file (tests/test_layout_gpu.py) uses, and value-level mutants of the ports that those shapes must catch."""
import numpy as np
import pytest
import torch

from tests import layout_ref as L


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 or b.dtype == np.float32:
        a, b = L.f32_bits(a), L.f32_bits(b)
    return a.shape == b.shape and bool((a == b).all())


def _same_prologue(x, y):
    return all(_eq(x[k], y[k]) for k in x)


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _pro(name):
    return _cached(("pro", name), lambda: L.prologue_case(name))


def _pro_ref(name):
    return _cached(("proref", name), lambda: L.prologue_ref(*_pro(name)))


# ------------------------------------------------------------------------------------------------ the reference against independent forms
@pytest.mark.parametrize("name", list(L.PROLOGUE_CASES))
def test_prologue_reference_equals_the_torch_formulation(name):
    """The element-wise torch form of test_kernels_gpu.test_step_prologue_matches_the_torch_formulation (and its row-set twin),
    written over the whole padded layout at once."""
    segs, lens, B, labels, V, rowset = _pro(name)
    ref = _pro_ref(name)
    kb, kbp, valid_t, kv_t, rank_t = [], [], [], [], []
    lab_t = torch.from_numpy(labels) if labels is not None else torch.full((B * sum(lens),), -100, dtype=torch.int64)
    row = 0
    for p, S in enumerate(lens):
        m = torch.ones(B, S)
        cov = torch.zeros(B, S, dtype=torch.bool)
        for arr, sp, off in segs:
            if sp != p:
                continue
            a = torch.from_numpy(arr)[:, :max(0, min(arr.shape[1], S - off))]
            n = a.shape[1]
            take = ~cov[:, off:off + n]
            m[:, off:off + n] = torch.where(take, a, m[:, off:off + n])
            cov[:, off:off + n] = True
        bias = (1.0 - m) * -10000.0
        slots = (S + 127) // 128 * 128
        kb.append(torch.nn.functional.pad(bias, (0, slots - S), value=-1.0e30).reshape(-1))
        live = bias > -10000.0
        pos = torch.arange(S)
        kv = torch.where(live.any(1), torch.where(live, pos + 1, 0).amax(1), torch.tensor(S))
        lab = lab_t[row:row + B * S].view(B, S)
        lab_end = torch.where(lab != -100, pos + 1, 0).amax(1)
        kv_t.append(kv)
        if rowset:
            act = live | (lab != -100) | ~live.any(1, keepdim=True)
            act[:, 0] = True
            valid_t.append(act.sum(1))
            key = torch.where(act, 0, 1) * S + pos                  # active first, order kept
            order = key.argsort(1)
            rk = torch.empty_like(order)
            rk.scatter_(1, order, pos.expand(B, S).contiguous())
            rank_t.append(rk.reshape(-1))
            kbp.append(torch.nn.functional.pad(bias.gather(1, order), (0, slots - S), value=-1.0e30).reshape(-1))
        else:
            valid_t.append(torch.maximum(kv, lab_end))
        row += B * S
    assert _eq(ref["key_bias"], torch.cat(kb).numpy())
    assert _eq(ref["kv_len"], torch.cat(kv_t).numpy()) and _eq(ref["valid"], torch.cat(valid_t).numpy())
    ok = (lab_t >= 0) & (lab_t < V)
    assert _eq(ref["idx"], ok.nonzero().reshape(-1).numpy())
    assert int(ref["words"][-3]) == int(ok.sum()) and int(ref["words"][-1]) == int(((lab_t != -100) & ~ok).sum())
    if rowset:
        assert _eq(ref["rank"], torch.cat(rank_t).numpy()) and _eq(ref["key_bias_perm"], torch.cat(kbp).numpy())


def test_key_bias_rounds_twice_like_the_reference():
    """m = 3e-8: (1 - m) rounds to 1 - 2^-24 and the product to -9999.999 (a live key); ONE rounding would give -10000. m = 1: -0."""
    kb = L.key_bias(np.array([3e-8, 1.0, 0.0, 0.3], np.float32))
    assert kb[0] > np.float32(-10000.0) and L.f32_bits(kb[1]) == 0x80000000 and kb[2] == np.float32(-10000.0)
    assert kb[3] == np.float32(np.float32(0.7) * np.float32(-10000.0))


@pytest.mark.parametrize("name", list(L.SPLIT_CASES))
def test_split_layout_reference_equals_the_host_form(name):
    from msa_amd import ops
    lens, valid, heads = L.split_case(name)
    base = ops.SeqLayout(lens, heads, "cpu")
    rows = base._rows_f
    nq_max = sum((n + rows - 1) // rows for n in lens)
    nf_max = nq_max + len(lens)
    ref = L.split_layout_ref(lens, valid, heads, rows, nf_max, nq_max)
    h = ops.SplitLayout(base, valid, "cpu")
    f = ref[:4 * nf_max].reshape(4, nf_max)
    q = ref[4 * nf_max:4 * nf_max + 4 * nq_max].reshape(4, nq_max)
    nf, nq, ra = ref[-4:-1]
    assert (nf, nq, ra) == (h.nftiles, h.ntiles, h.rows_a)
    for j, n in enumerate(("ftile_seq", "ftile_r0", "ftile_qshift", "ftile_qend")):
        assert _eq(f[j, :nf], getattr(h, n).numpy()), n
    for j, n in enumerate(("tile_seq", "tile_r0", "qtile_qshift", "qtile_qend")):
        assert _eq(q[j, :nq], getattr(h, n).numpy()), n
    ns = len(lens)
    tail = ref[4 * nf_max + 4 * nq_max:]
    assert _eq(tail[:ns], h.seq_start.numpy()) and _eq(tail[ns:2 * ns], h.kv_len.numpy())
    for mode, kw in ((0, {}), (1, dict(dedupe=True)), (2, dict(drop=True))):
        hm = ops.SplitLayout(base, valid, "cpu", **kw)
        perm, inv, owned, _ = L.split_rows_ref(lens, valid, mode)
        assert _eq(inv, hm.inv.numpy()), mode
        assert _eq(perm[owned], hm.perm.numpy()[owned]), mode
        assert owned.all() or mode == 2


def test_row_movement_reference_equals_torch_index_ops():
    g = torch.Generator().manual_seed(3)
    lab = L.active_labels(70400)
    assert _eq(L.active_rows_ref(lab, 30522), ((torch.from_numpy(lab) >= 0) & (torch.from_numpy(lab) < 30522)).nonzero().reshape(-1).numpy())
    rows, extra, mp = torch.randperm(900, generator=g)[:50], torch.randperm(900, generator=g)[:7], torch.randperm(900, generator=g)
    assert _eq(L.compact_ref(rows.numpy(), extra.numpy(), mp.numpy()), mp[torch.cat((rows, extra))].numpy())
    src = torch.randint(0, 256, (300, 12), generator=g, dtype=torch.uint8)
    idx = torch.randint(0, 300, (1000,), generator=g)
    assert _eq(L.copy_rows(src.numpy(), idx.numpy()), src.index_select(0, idx).numpy())
    a, b = torch.randint(-5, 5, (70000,), generator=g), torch.randint(-9, 9, (3,), generator=g)
    assert _eq(L.pack_ref([a.numpy(), (4, 77), b.numpy()]), torch.cat((a, torch.full((4,), 77), b)).numpy())
    # scatter: zeros().index_copy_() of the current list, earlier lists invisible
    table = np.zeros(500, np.int64)
    l1, l2 = np.array([5, 9, 400]), np.array([9, 100])
    table = L.stamp_table_ref(table, l1, 7)
    table = L.stamp_table_ref(table, l2, L.next_stamp(7))
    take = L.scatter_ref(table, 8, 2, 450)
    want = torch.full((450,), -1, dtype=torch.int64).index_copy_(0, torch.tensor([9, 100]), torch.tensor([0, 1]))
    assert _eq(take, want.numpy())
    assert L.next_stamp(0xFFFFFFEF) == 0xFFFFFFF0 and L.next_stamp(0xFFFFFFF0) == 1 and L.next_stamp(0) == 1


def test_rne_equals_torch_on_everything_but_nan():
    rng = np.random.default_rng(0)
    bits = np.concatenate((rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32), L.SPECIAL_F32))
    bits = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]
    t = torch.from_numpy(bits.view(np.int32)).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert _eq(L.bf16_rne(bits), t)
    nan = np.array([0x7F800001, 0xFFBFFFFF, 0x7FC12345], np.uint32)
    assert _eq(L.bf16_rne(nan), np.array([0x7FC0, 0xFFFF, 0x7FC1], np.uint16))


def test_rng_reference_equals_the_library_host_functions():
    from msa_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    seeds = rng.integers(0, 2 ** 63, size=10000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, size=10000).astype(np.uint64)
    sites = rng.integers(0, 2 ** 32, size=10000, dtype=np.uint64)
    ps = np.concatenate((rng.random(10000 - 8).astype(np.float32), np.array([0, 1, 0.1, 0.5, 1e-9, 0.99999, 2.0, -1], np.float32)))
    for s, t, p in zip(seeds.tolist(), sites.tolist(), ps.tolist()):
        assert lib.mmbert_rng_stream(s, t) == L.rng_stream(s, t), (s, t)
        assert lib.mmbert_dropout_thr16(p) == L.dropout_thr16(p), p


def test_keep_rule_has_the_documented_drop_probability():
    v = np.arange(65536)
    for thr in (0, 1, 6554, 32768, 65535):
        assert int((~L.keep16(v, thr)).sum()) == thr
        assert _eq(L.keep16_port(v, thr), L.keep16(v, thr))


# ------------------------------------------------------------------------------------------------ ports equal the reference
def _split_port_vs_ref(name, mut=None):
    lens, valid, heads = L.split_case(name)
    rows = 128
    nq_max = sum((n + rows - 1) // rows for n in lens)
    nf_max = nq_max + len(lens)
    ref = _cached(("slref", name), lambda: L.split_layout_ref(lens, valid, heads, rows, nf_max, nq_max))
    return _eq(ref, L.split_layout_port(lens, valid, heads, rows, nf_max, nq_max, mut))


def _split_rows_vs_ref(name, mode, use_rank, mut=None):
    lens, valid, heads = L.split_case(name)
    rank = L.seq_ranks(lens, 9) if use_rank else None
    perm, inv, owned, st = L.split_rows_ref(lens, valid, mode, rank)
    rs = np.repeat(np.arange(len(lens)), lens)
    rp = np.concatenate([np.arange(n) for n in lens])
    pp, pi, po = L.split_rows_port(rs, rp, st["start_a"], st["start_b"], st["v"], mode, st["rows_a"], st["n_packed"], rank, mut)
    return _eq(inv, pi) and _eq(owned, po) and _eq(perm[owned], pp[po])


def _active_vs_ref(M, mut=None):
    lab = L.active_labels(M)
    return _eq(L.active_rows_ref(lab, 30522), L.active_rows_port(lab, 30522, mut))


def _scatter_vs_ref(mut=None):
    table, stamp, nlist, nrows = L.scatter_case()
    return _eq(L.scatter_ref(table, stamp, nlist, nrows), L.scatter_port(table, stamp, nlist, nrows, mut))


def _gather_vs_ref(width, vec16, mut=None):
    rng = np.random.default_rng(width)
    src = rng.integers(0, 256, size=(97, width), dtype=np.uint8)
    idx = rng.integers(0, 97, size=300)
    return _eq(L.copy_rows(src, idx), L.gather_port(src, idx, vec16, mut))


def _pack_vs_ref(mut=None):
    segs = L.pack_case()
    return _eq(L.pack_ref(segs), L.pack_port(segs, mut))


def _cast_vs_ref(mut=None):
    bits = L.cast_bits()
    return _eq(L.bf16_rne(bits), L.cast_port(bits, mut))


def _transpose_vs_ref(which, bf16src=False, mut=None):
    descs, ntiles, src_bits, dst0 = L.transpose_case(which, bf16src)
    return _eq(L.transpose_ref(src_bits, dst0, descs, bf16src), L.transpose_port(src_bits, dst0, descs, ntiles, bf16src, mut))


def _dropout_vs_ref(mut=None):
    stream, thr = L.rng_stream(1234, 17), L.dropout_thr16(0.1)
    return _eq(L.dropout_mask_ref(L.DROPOUT_N, stream, thr), L.dropout_mask_port(L.DROPOUT_N, stream, thr, mut))


def _mlm_vs_ref(n_special, mut=None, p_sel=0.15, p_rep=0.8):
    ids = _cached(("mlmids",), lambda: L.mlm_ids(L.MLM_N))
    sp = L.mlm_specials([101, 102, 0][:n_special])
    stream = L.rng_stream(99, 4242)
    a = L.mlm_ref(ids, stream, round(p_sel * 65536), round(p_rep * 65536), sp, 103)
    b = L.mlm_port(ids, stream, round(p_sel * 65536), round(p_rep * 65536), sp, 103, mut)
    return _eq(a[0], b[0]) and _eq(a[1], b[1])


def _prologue_vs_ref(name, mut=None):
    return _same_prologue(_pro_ref(name), L.prologue_port(*_pro(name), mut=mut))


CHECKS = {
    **{f"prologue[{n}]": (lambda n=n: _prologue_vs_ref(n)) for n in L.PROLOGUE_CASES},
    **{f"split_layout[{n}]": (lambda n=n: _split_port_vs_ref(n)) for n in L.SPLIT_CASES},
    **{f"split_rows[{n},{m},{r}]": (lambda n=n, m=m, r=r: _split_rows_vs_ref(n, m, r)) for n in ("headline_12", "three_heads_zero", "large_16")
       for m in (0, 1, 2) for r in (False, True)},
    **{f"active_rows[{M}]": (lambda M=M: _active_vs_ref(M)) for M in L.ACTIVE_M},
    "scatter": _scatter_vs_ref,
    **{f"gather[{w},{v}]": (lambda w=w, v=v: _gather_vs_ref(w, v)) for w in (4, 12, 16, 20, 1536, 6144) for v in (False, True) if not (v and w % 16)},
    "pack": _pack_vs_ref,
    "cast": _cast_vs_ref,
    **{f"transpose[{w},{b}]": (lambda w=w, b=b: _transpose_vs_ref(w, b)) for w in L.TRANSPOSE_CASES for b in (False, True)},
    "dropout": _dropout_vs_ref,
    **{f"mlm[{k}]": (lambda k=k: _mlm_vs_ref(k)) for k in range(4)},
}


@pytest.mark.parametrize("name", list(CHECKS))
def test_port_equals_the_reference(name):
    assert CHECKS[name]()


# ------------------------------------------------------------------------------------------------ mutants: (name, shape that kills it)
MUTANTS = [
    ("no_base_carry_rank", "fused_rowset (S = 1050: rank past position 255)", lambda m: _prologue_vs_ref("fused_rowset", m)),
    ("no_base_carry_idx", "headline (S = 550: labelled rows past position 255)", lambda m: _prologue_vs_ref("headline", m)),
    ("valid_ignores_last_lab", "special (a label past the last live key)", lambda m: _prologue_vs_ref("special", m)),
    ("no_every_rule", "special_rowset (a sequence without a live key)", lambda m: _prologue_vs_ref("special_rowset", m)),
    ("no_position0_rule", "special_rowset (a masked, unlabelled position 0)", lambda m: _prologue_vs_ref("special_rowset", m)),
    ("bad_label_counted", "headline (labels -1, V, V + 9, int64 min)", lambda m: _prologue_vs_ref("headline", m)),
    ("last_segment_wins", "overlap (overlapping segments)", lambda m: _prologue_vs_ref("overlap", m)),
    ("uncovered_reads_zero", "overlap (positions no segment covers)", lambda m: _prologue_vs_ref("overlap", m)),
    ("bias_one_rounding", "frac (m = 3e-8, m = 1)", lambda m: _prologue_vs_ref("frac", m)),
    ("live_key_ge", "chunks (masked keys at exactly -10000)", lambda m: _prologue_vs_ref("chunks", m)),
    ("xs_doubled", "headline_12 (12 heads: xs = 2)", lambda m: _split_port_vs_ref("headline_12", m)),
    ("rank_tie_reversed", "eight_heads_ties (equal valid counts)", lambda m: _split_port_vs_ref("eight_heads_ties", m)),
    ("regionB_first_row_off_by_one", "headline_12 (region-B tiles)", lambda m: _split_port_vs_ref("headline_12", m)),
    ("no_minus_one_fill", "headline_12 (unused list entries)", lambda m: _split_port_vs_ref("headline_12", m)),
    ("mode1_owner_off_by_one", "split_rows mode 1, three_heads_zero", lambda m: _split_rows_vs_ref("three_heads_zero", 1, False, m)),
    ("rank_ignored", "split_rows mode 0 with rank, headline_12", lambda m: _split_rows_vs_ref("headline_12", 0, True, m)),
    ("no_base_carry_active", "active_rows M = 1025", lambda m: _active_vs_ref(1025, m)),
    ("stale_stamp_accepted", "scatter (an earlier list's entries in the table)", _scatter_vs_ref),
    ("no_nlist_check", "scatter (current stamp, entry index >= nlist)", _scatter_vs_ref),
    ("gather_drops_tail", "gather, 12-byte rows (4-byte path)", lambda m: _gather_vs_ref(12, False, m)),
    ("pack_one_pass", "pack (a segment of more than 65 536)", _pack_vs_ref),
    ("cast_truncates", "cast (RNE ties and round-ups)", _cast_vs_ref),
    ("cast_flushes_subnormals", "cast (fp32 subnormals)", _cast_vs_ref),
    ("cast_canonical_nan", "cast (NaN payloads)", _cast_vs_ref),
    ("padding_unwritten", "transpose edge (dst_ld > rows)", lambda m: _transpose_vs_ref("edge", False, m)),
    ("search_one_early", "transpose many (tile0 boundaries)", lambda m: _transpose_vs_ref("many", False, m)),
    ("transpose_truncates", "transpose edge (RNE)", lambda m: _transpose_vs_ref("edge", False, m)),
    ("keep_gt", "dropout (halves equal to the threshold)", _dropout_vs_ref),
    ("halves_swapped", "dropout (odd / even elements)", _dropout_vs_ref),
    ("dropout_one_pass", "dropout (n past the 4096 x 256 grid)", _dropout_vs_ref),
    ("mlm_halves_swapped", "mlm (3 special ids)", lambda m: _mlm_vs_ref(3, m)),
    ("third_special_ignored", "mlm (3 special ids)", lambda m: _mlm_vs_ref(3, m)),
    ("mlm_one_pass", "mlm (n past the 1024 x 256 grid)", lambda m: _mlm_vs_ref(3, m)),
]


def test_there_are_enough_mutants():
    assert len(MUTANTS) >= 20 and len({m for m, _, _ in MUTANTS}) == len(MUTANTS)


@pytest.mark.parametrize("j", range(len(MUTANTS)), ids=[f"{m} -- {c}" for m, c, _ in MUTANTS])
def test_mutant_fails_the_reference(j):
    mut, case, run = MUTANTS[j]
    assert not run(mut), f"mutant {mut} survives {case}"
