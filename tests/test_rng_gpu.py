"""GPU: the counter-based generator on the device, bit for bit against the integer reference of tests/rng_ref.py (which never calls
the library): the flat dropout mask, the attention index scheme, the masks the forward, dQ and dK/dV attention kernels themselves
apply (read back exactly through one-hot coded K, V and dctx), and the MLM mask.  Every comparison is ``rng_ref.check_equal``: equality, no tolerance.
Buffers written through the C ABI sit inside sentinel canaries that must come back untouched.
(tests/test_rng_reference_cpu.py shows on the CPU that these cases reject wrong generators, and holds the stream-pair survey.)"""

import numpy as np
import pytest
import torch

from tests import rng_cases as C
from tests import rng_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
CANARY_U8 = 0xA5
CANARY_I64 = 0x5A5A5A5A5A5A5A5A
CANARY_BF16 = 0x7FA5                  # a NaN bit pattern no output takes


@pytest.fixture(scope="module")
def ops():
    from msa_amd import ops as o
    return o


def lib():
    from msa_amd import _lib
    return _lib.load()


def _guarded(n, dtype, canary):
    """A device buffer of PAD + n + PAD elements filled with ``canary``; returns (buffer, the n-element view in the middle)."""
    buf = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _canaries_intact(buf, n, canary, what):
    b = buf.cpu().numpy()
    assert (b[:PAD] == canary).all() and (b[PAD + n:] == canary).all(), f"{what}: wrote outside its {n} elements"


# ------------------------------------------------------------------------------------------------ flat masks
def _flat_mask(ops, n, stream, thr):
    """mmbert_dropout_mask through ops.dropout_mask and through the C ABI into a guarded buffer: the same bytes, canaries intact."""
    buf, out = _guarded(n, torch.uint8, CANARY_U8)
    code = lib().mmbert_dropout_mask(ops._stream(), out.data_ptr(), n, stream, thr)
    assert code == 0, code
    via_ops = ops.dropout_mask(n, (stream, thr, R.drop_scale(thr)), DEV)
    torch.cuda.synchronize()
    _canaries_intact(buf, n, CANARY_U8, f"dropout_mask n {n}")
    assert torch.equal(out, via_ops)
    return via_ops.cpu().numpy()


@pytest.mark.parametrize("n", C.DROPOUT_N)
def test_dropout_mask_equals_the_reference(ops, n):
    """n in {1, 2, 3, 255, 256, 257, 2^20 + 1} x thr16 in {1, 6554, 32767, 32768, 32769, 65535} x streams {0, 0xFFFFFFFF, two derived}."""
    for stream in C.dropout_streams():
        for thr in C.DROPOUT_THR:
            R.check_equal(_flat_mask(ops, n, stream, thr), R.keep(stream, 0, n, thr), f"n {n} stream {stream:#x} thr16 {thr}")


def test_dropout_mask_across_index_2_to_32(ops):
    """A flat mask of 2^32 + 257 elements, compared in the window of 513 elements around index 2^32: the pair index is (idx >> 1) of
    the 64-bit index (an index cut to 32 bits first repeats the start of the stream there).  The only case whose size is its point: it allocates
    4.3 GB of device memory, twice in turn -- do not parametrise over it or copy it."""
    idx0, n = C.WINDOW
    total = idx0 + n
    stream = C.dropout_streams()[2]
    for thr in (6554, 32768):
        out = ops.dropout_mask(total, (stream, thr, R.drop_scale(thr)), DEV)
        got = out[idx0:].cpu().numpy()
        head = out[:n].cpu().numpy()
        del out
        R.check_equal(got, R.keep(stream, idx0, n, thr), f"window at 2^32, thr16 {thr}")
        R.check_equal(head, R.keep(stream, 0, n, thr), f"start of the same mask, thr16 {thr}")


def test_host_stream_and_threshold_on_this_machine(ops):
    """The host functions as loaded beside the GPU (the CPU file compares them at every seed, site and p of its lists)."""
    for seed, site in ((0, 0), (2 ** 64 - 1, 2 ** 32 - 1), (7 * 1000003 + 1, 1001)):
        assert ops.rng_stream(seed, site) == R.rng_stream(seed, site)
    for p in (1 / 65536, 0.1, 0.5, 1.0):
        d = ops.make_drop(p, 7000022, 8)
        assert d == (R.rng_stream(7000022, 8), R.thr16(p), R.drop_scale(R.thr16(p)))


# ------------------------------------------------------------------------------------------------ attention index scheme
@pytest.mark.parametrize("heads", C.ATTN_HEADS)
@pytest.mark.parametrize("S", C.ATTN_S)
def test_attn_dropout_mask_equals_the_reference_index_scheme(ops, S, heads):
    """S in {1, 3, 4, 5, 63, 64, 65, 130} x heads in {1, 3, 12} x elem_base in {0, 4, 2^31 - 4, 2^31, the last base whose heads end at or
    below 2^32}, every head of each; thr16 6554 and 32768."""
    stream = C.dropout_streams()[3]
    for thr in (6554, 32768):
        drop = (stream, thr, R.drop_scale(thr))
        for base in C.attn_bases(S, heads):
            got = torch.stack([ops.attn_dropout_mask(S, base, h, drop, DEV) for h in range(heads)]).cpu().numpy()
            R.check_equal(got, R.attn_keep(stream, base, S, heads, thr), f"S {S} heads {heads} base {base:#x} thr16 {thr}")


def test_seq_layout_bases_equal_the_reference(ops):
    for lens, heads in (([5, 130, 64, 257, 63, 65, 1, 3], 3), ([50] * 4 + [550] * 8, 12)):
        lay = ops.SeqLayout(lens, heads, DEV)
        bases, _ = R.seq_elem_bases(lens, heads)
        assert lay.elem_base_host == bases and lay.elem_base.cpu().tolist() == R.base_bits32(bases)


# ------------------------------------------------------------------------------------------------ masks read back from the attention kernels
def _readback(ops, lens, heads, p, tails=None, use_kv=False, bases=None, forward=None):
    """Forward and backward on the read-back inputs (tests/rng_cases.py): the keep flags decoded from ctx (along the keys), from dV
    (along the queries) and, on the second set of inputs, from dQ equal the reference's, for every sequence and head.  ``tails``: per sequence the count of trailing keys masked
    by key_bias; ``bases``: elem_base of every sequence in place of the layout's own; ``forward``: another way to run the forward."""
    H = heads * 64
    thr = R.thr16(p)
    drop = ops.make_drop(p, 7000022, 8)
    assert drop == (R.rng_stream(7000022, 8), thr, R.drop_scale(thr))
    layout = ops.SeqLayout(lens, heads, DEV)
    if bases is not None:
        layout.elem_base = torch.tensor(R.base_bits32(bases), dtype=torch.int32, device=DEV)
        layout.elem_base_host = list(bases)
    bases = layout.elem_base_host
    live = [np.ones(S, dtype=bool) for S in lens]
    for s, t in enumerate(tails or []):
        if t:
            live[s][lens[s] - t:] = False
    bias = torch.from_numpy(np.concatenate([np.where(l, 0.0, -10000.0) for l in live])).float().to(DEV)
    kb = ops.pad_key_bias(bias, layout)
    kv = ops.attn_kv_len(kb, layout) if use_kv else None
    want = [R.attn_keep(drop[0], bases[s], S, heads, thr) * live[s][None, None, :] for s, S in enumerate(lens)]

    def run(inputs, fwd):
        qkv_h, dctx_h = inputs
        qkv = torch.from_numpy(qkv_h).to(DEV).to(torch.bfloat16)
        dctx = torch.from_numpy(dctx_h).to(DEV).to(torch.bfloat16)
        M = qkv.shape[0]
        cbuf, ctx = _guarded(M * H, torch.int16, CANARY_BF16)
        dbuf, dqkv = _guarded(M * 3 * H, torch.int16, CANARY_BF16)
        ctx, dqkv = ctx.view(torch.bfloat16).view(M, H), dqkv.view(torch.bfloat16).view(M, 3 * H)
        if fwd is None:
            _, lse = ops.attn_fwd(qkv, kb, layout, H, drop=drop, ctx=ctx, kv_len=kv)
        else:
            lse = fwd(qkv, kb, layout, drop, ctx, kv)
        ops.attn_bwd(qkv, ctx, dctx, lse, kb, layout, H, drop=drop, dqkv=dqkv, kv_len=kv)
        torch.cuda.synchronize()
        _canaries_intact(cbuf, M * H, CANARY_BF16, "attn_fwd ctx")
        _canaries_intact(dbuf, M * 3 * H, CANARY_BF16, "attn_bwd dqkv")
        out = ctx.float().cpu().numpy(), dqkv.float().cpu().numpy()
        assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
        return out

    # ctx prints the forward kernel's mask along the keys, dV the dK/dV kernel's along the queries
    ctx_h, d_h = run(C.readback_inputs(lens, heads), forward)
    s0 = 0
    for s, S in enumerate(lens):
        for h in range(heads):
            cols = slice(64 * h, 64 * h + 64)
            what = f"seq {s} (S {S}, base {bases[s]:#x}) head {h} p {p}"
            R.check_equal(C.decode_ctx(ctx_h[s0:s0 + S, cols], live[s], drop[2], "ctx " + what), want[s][h], "forward mask, " + what)
            R.check_equal(C.decode_dv(d_h[s0:s0 + S, 2 * H + 64 * h:2 * H + 64 * h + 64], live[s], drop[2], "dV " + what), want[s][h],
                          "backward (dV) mask, " + what)
        s0 += S
    if forward is not None:
        return
    # dQ prints the dQ kernel's own regeneration of the mask (second set of inputs)
    ctx_h, d_h = run(C.readback_inputs_dq(lens, heads), None)
    s0 = 0
    for s, S in enumerate(lens):
        for h in range(heads):
            what = f"seq {s} (S {S}, base {bases[s]:#x}) head {h} p {p}"
            got = C.decode_dq(d_h[s0:s0 + S, 64 * h:64 * h + 64], ctx_h[s0:s0 + S, 64 * h], live[s], drop[2], "dQ " + what)
            R.check_equal(got, want[s][h], "backward (dQ) mask, " + what)
        s0 += S


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S", [5, 63, 64, 65, 130, 257])
def test_attention_kernels_apply_the_reference_mask(ops, S, p):
    """Two sequences of length S (the second at a non-zero elem_base), 3 heads."""
    _readback(ops, [S, S], 3, p)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_kernels_apply_the_reference_mask_packed_mixed_lengths(ops, p):
    """Mixed lengths in one launch at 12 heads, dense and with kv_len."""
    lens = [5, 130, 64, 257, 63, 65, 1, 3, 320]
    _readback(ops, lens, 12, p)
    _readback(ops, lens, 12, p, use_kv=True)


@pytest.mark.parametrize("use_kv", [False, True], ids=["dense", "kv_len"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_kernels_apply_the_reference_mask_with_masked_key_tails(ops, p, use_kv):
    """A tail of keys masked by key_bias (ending inside a 64-key tile, on a tile boundary, one key, none): the live keys' flags are
    the reference's at their own indices, the masked keys carry no weight."""
    _readback(ops, [130, 257, 65, 64, 200], 3, p, tails=[1, 57, 20, 0, 72], use_kv=use_kv)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_kernels_apply_the_reference_mask_at_bases_from_2_to_31(ops, p):
    """The small layout once more with elem_base / elem_base_host overwritten: 2^31, a base in the upper half, the last base that fits
    below 2^32, and one whose rows cross 2^31 (bases >= 2^31 travel as negative int32 bit patterns)."""
    lens, heads = [5, 65, 130, 63], 3
    bases = [2 ** 31, 0xC0000000 + 4 * 12345, R.last_base(130, heads), 2 ** 31 - 4 * 1000]
    _readback(ops, lens, heads, p, bases=bases)


def test_composite_layer_forward_applies_the_reference_mask(ops):
    """mmbert_layer_fwd (the model's one-call-per-layer path) on the same small layout: x holds the read-back code, Wqkv is 0 but for an
    identity in its V block, so the layer's own QKV GEMM produces Q = K = 0 and V = the code, and its attention launch writes the
    decodable context into ``actx`` (everything behind the attention runs on zero weights and is not looked at)."""
    heads, I = 3, 256
    H = heads * 64

    def forward(qkv, kb, layout, drop, ctx, kv):
        M = qkv.shape[0]
        bf, f32 = torch.bfloat16, torch.float32
        z = lambda *shape, dt=bf: torch.zeros(shape, device=DEV, dtype=dt)
        x = qkv[:, 2 * H:].contiguous()
        Wqkv = z(3 * H, H)
        Wqkv[2 * H:] = torch.eye(H, device=DEV, dtype=bf)
        t = dict(Wqkv=Wqkv, Wo=z(H, H), W1=z(I, H), W2=z(H, I), bqkv=z(3 * H, dt=f32), bo=z(H, dt=f32), b1=z(I, dt=f32), b2=z(H, dt=f32),
                 ln1_g=torch.ones(H, device=DEV), ln1_b=z(H, dt=f32), ln2_g=torch.ones(H, device=DEV), ln2_b=z(H, dt=f32),
                 qkv=z(M, 3 * H), lse=z(M, heads, dt=f32), z1=z(M, H), y1=z(M, H), g=z(M, I), z2=z(M, H), y2=z(M, H))
        a = ops._LayerFwd()
        for k, v in t.items():
            setattr(a, k, v.data_ptr())
        a.x, a.ldx, a.rows, a.H, a.I, a.ln_eps = x.data_ptr(), x.stride(0), M, H, I, 1e-12
        a.actx, a.ldy2 = ctx.data_ptr(), H
        a.tile_queue = ops._tile_queue(torch.device(DEV))
        ops._set_drop(a.att, drop)
        ops._set_drop(a.h1, None)
        ops._set_drop(a.h2, None)
        AL = ops.attn_layout_struct(kb, layout, backward=False)
        if kv is not None:
            AL.kv_len = kv.data_ptr()
        ops.layer_fwd(AL, a)
        torch.cuda.synchronize()
        assert torch.equal(t["qkv"], qkv), "the layer's QKV GEMM did not reproduce the read-back inputs"
        return t["lse"]

    _readback(ops, [5, 65, 130, 257], heads, 0.1, tails=[0, 20, 1, 57], use_kv=True, forward=forward)


# ------------------------------------------------------------------------------------------------ MLM mask
MLM_CASES = C.mlm_cases()


def _mlm_run(ops, case):
    ids_h, kw = case["ids"], case["kw"]
    n = ids_h.size
    want_ids, want_lab = R.mlm_mask(ids_h, **kw)
    # (1) ops.mlm_mask, ids inside a guarded buffer
    ibuf, ids = _guarded(n, torch.int64, CANARY_I64)
    ids.copy_(torch.from_numpy(ids_h))
    labels = ops.mlm_mask(ids, kw["p_select"], kw["seed"], special_ids=kw["special_ids"], mask_id=kw["mask_id"], p_replace=kw["p_replace"], site=kw["site"])
    torch.cuda.synchronize()
    _canaries_intact(ibuf, n, CANARY_I64, "mlm_mask ids")
    R.check_equal(ids.cpu().numpy(), want_ids, case["name"] + " ids")
    R.check_equal(labels.cpu().numpy(), want_lab, case["name"] + " labels")
    # (2) the C entry point with the labels guarded as well
    ibuf, ids = _guarded(n, torch.int64, CANARY_I64)
    lbuf, lab = _guarded(n, torch.int64, CANARY_I64)
    ids.copy_(torch.from_numpy(ids_h))
    sp = list(kw["special_ids"]) + [-1] * (3 - len(kw["special_ids"]))
    code = lib().mmbert_mlm_mask(ops._stream(), ids.data_ptr(), lab.data_ptr(), n, R.rng_stream(kw["seed"], kw["site"]), R.mlm_thr(kw["p_select"]),
                                 R.mlm_thr(kw["p_replace"]), sp[0], sp[1], sp[2], kw["mask_id"])
    assert code == 0, code
    torch.cuda.synchronize()
    _canaries_intact(ibuf, n, CANARY_I64, "mmbert_mlm_mask ids")
    _canaries_intact(lbuf, n, CANARY_I64, "mmbert_mlm_mask labels")
    R.check_equal(ids.cpu().numpy(), want_ids, case["name"] + " ids (C ABI)")
    R.check_equal(lab.cpu().numpy(), want_lab, case["name"] + " labels (C ABI)")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 64 * 50])
def test_mlm_mask_equals_the_reference(ops, n):
    """Per n: p_select in {0, 0.15, 1.0} x p_replace in {0, 0.8, 1.0 (threshold 65536: the unsigned compare)}, 0 to 3 special ids, ids equal
    to mask_id on input, sites 4242 and 17; ids and labels element for element."""
    cases = [c for c in MLM_CASES if c["name"].startswith(f"n{n}-")]
    assert len(cases) == 9
    for c in cases:
        _mlm_run(ops, c)


@pytest.mark.parametrize("name", ["boundary-select", "boundary-replace"])
def test_mlm_mask_at_a_half_equal_to_the_threshold(ops, name):
    """One element's deciding half EQUALS the threshold: not selected (low half) / not replaced (high half) -- where '<' and '<=' part."""
    _mlm_run(ops, next(c for c in MLM_CASES if c["name"] == name))
