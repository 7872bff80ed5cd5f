"""The cases of tests/test_rng_gpu.py and the codecs of its mask read-back, beside (not inside) the integer reference tests/rng_ref.py.

Not a test module (pytest does not collect it): ``from tests import rng_cases as C``.

The read-back code (``readback_inputs`` / ``decode_ctx`` / ``decode_dv``) turns the attention kernels into exact mask printers: with
Q = 0 every live key of a row weighs 1/n, and V holds key j as the one-hot column j mod 64 with weight 2^(j div 64), so
ctx[i][c] * n / dropout scale is the integer whose bit g is the keep flag of key c + 64 g.  At most 5 groups (S <= 320) are used:
the integer is <= 31 and the two bf16 roundings on the way (the dropped P of the backward, every output; at most 2^-8 relative
each) move it by less than 31 * 2^-7 = 0.25, so the nearest integer is exact.  dctx coded the same way over the queries makes dV
print the mask along the query axis; ``readback_inputs_dq`` / ``decode_dq`` do the same for dQ.
"""
from __future__ import annotations

import numpy as np

from tests.rng_ref import U64, last_base, mlm_thr, pair_bits, rng_stream


def seed_with_half(value, site, n, high, first=1):
    """The first seed >= ``first`` under which some element of an n-element MLM draw at ``site`` has its low (``high``: high) half equal
    to ``value`` -- the one word at which ``<`` and ``<=`` part (a chance of n / 65536 per seed); returns (seed, element)."""
    q = np.arange(n, dtype=np.uint64)
    for seed in range(first, first + 4096):
        h = pair_bits(rng_stream(seed, site), q)
        half = (h >> U64(16)) if high else (h & U64(0xFFFF))
        at = np.nonzero(half == U64(value))[0]
        if at.size:
            return seed, int(at[0])
    raise AssertionError("no seed found")


# ------------------------------------------------------------------------------------------------ masks read back from the attention kernels
READBACK_MAX_S = 320                 # 5 groups of 64: integers <= 31 (see the module docstring)
READBACK_RESIDUAL = 0.25 + 1.0 / 64  # |value - nearest integer| a correct kernel stays below


def readback_code(S):
    """float32 [S, 64]: row j = 2^(j div 64) at column j mod 64."""
    assert S <= READBACK_MAX_S
    c = np.zeros((S, 64), dtype=np.float32)
    j = np.arange(S)
    c[j, j % 64] = 2.0 ** (j // 64)
    return c


def readback_inputs(lens, heads):
    """(qkv [M, 3H], dctx [M, H]) as float32 arrays (exact in bf16): Q = K = 0, V and dctx hold ``readback_code`` in every head."""
    code = np.concatenate([np.tile(readback_code(S), (1, heads)) for S in lens])
    H = heads * 64
    qkv = np.zeros((code.shape[0], 3 * H), dtype=np.float32)
    qkv[:, 2 * H:] = code
    return qkv, code.copy()


def _decode(block, live_n, scale, what):
    """[rows, 64] values -> their integers; asserts that they ARE integers times the constant."""
    x = np.asarray(block, dtype=np.float64) * live_n / scale
    k = np.rint(x)
    res = float(np.abs(x - k).max()) if x.size else 0.0
    assert res < READBACK_RESIDUAL, f"{what}: value {res:.3f} away from an integer multiple of scale / n: not a mask read-back"
    return k.astype(np.int64)


def _bits_to_flags(k, S):
    """int [rows, 64] -> [rows, S]: flag of position t = bit (t div 64) of column t mod 64."""
    t = np.arange(S)
    return ((k[:, t % 64] >> (t // 64)) & 1).astype(np.uint8)


def decode_ctx(ctx_block, live, scale, what=""):
    """One (sequence, head) block [S, 64] of the forward's context -> uint8 [S, S]: decoded keep flag of (query i, key j), 0 at the keys
    that are not ``live`` (bool [S]: P = 0 there); every bit outside the live keys must be 0."""
    S = live.size
    k = _decode(ctx_block, int(live.sum()), scale, what)
    flags = _bits_to_flags(k, S)
    flags = flags * live[None, :].astype(np.uint8)
    assert np.array_equal(_pack_rows(flags, S), k), f"{what}: weight outside the live keys"
    return flags


def decode_dv(dv_block, live, scale, what=""):
    """One (sequence, head) block [S keys, 64] of dV -> uint8 [S queries, S keys] (0 in the columns of keys that are not live)."""
    S = live.size
    k = _decode(dv_block, int(live.sum()), scale, what)
    assert not k[~live].any(), f"{what}: dV of a masked key is not 0"
    flags = _bits_to_flags(k, S)                                                 # [key, query]
    assert np.array_equal(k, _pack_rows(flags, S)), f"{what}: weight outside the sequence's queries"
    return flags.T * live[None, :].astype(np.uint8)


def _pack_rows(flags, S):
    packed = np.zeros((flags.shape[0], 64), dtype=np.int64)
    for g in range((S + 63) // 64):
        seg = flags[:, 64 * g:min(S, 64 * g + 64)].astype(np.int64)
        packed[:, :seg.shape[1]] += seg << g
    return packed


# ------------------------------------------------------------------------------------------------ the cases of tests/test_rng_gpu.py
# (in a module of their own so that tests/test_rng_reference_cpu.py can show, without a GPU, that they reject wrong generators)
DROPOUT_N = [1, 2, 3, 255, 256, 257, 2 ** 20 + 1]
DROPOUT_THR = [1, 6554, 32767, 32768, 32769, 65535]
WINDOW = (2 ** 32 - 256, 513)        # (idx0, n): the elements around index 2^32 of a flat mask of 2^32 + 257 elements
ATTN_S = [1, 3, 4, 5, 63, 64, 65, 130]
ATTN_HEADS = [1, 3, 12]


def dropout_streams():
    return [0, 0xFFFFFFFF, rng_stream(7 * 1000003 + 1, 0), rng_stream(7 * 1000003 + 1, 1001)]


def attn_bases(S, heads):
    return [0, 4, 2 ** 31 - 4, 2 ** 31, last_base(S, heads)]


def mlm_cases():
    """dicts name / ids / kw (the arguments of ``mlm_mask`` behind ids).  ids are drawn from 95 .. 109 so that the special ids, mask_id = 103
    itself and plain ids are all frequent; the site alternates between the trainer's 4242 and 17.  The two boundary cases take the first
    seed under which one element's deciding half EQUALS the threshold (``seed_with_half``): there ``<`` and ``<=`` part."""
    g = np.random.default_rng(11)
    specials = [(), (101,), (101, 102), (101, 102, 100)]
    out, k = [], 0
    for n in (1, 255, 256, 257, 64 * 50):
        for ps in (0.0, 0.15, 1.0):
            for pr in (0.0, 0.8, 1.0):
                sp = specials[k % 4]
                site = 4242 if k % 2 == 0 else 17
                ids = g.integers(95, 110, size=n).astype(np.int64)
                ids[0] = 103
                out.append(dict(name=f"n{n}-sel{ps}-rep{pr}-sp{len(sp)}-site{site}", ids=ids,
                                kw=dict(p_select=ps, p_replace=pr, seed=1000 + k, site=site, special_ids=sp, mask_id=103)))
                k += 1
    n = 64 * 50
    seed, _ = seed_with_half(mlm_thr(0.15), 17, n, high=False)
    ids = np.full(n, 2000, dtype=np.int64)
    out.append(dict(name="boundary-select", ids=ids, kw=dict(p_select=0.15, p_replace=0.8, seed=seed, site=17, special_ids=(101, 102), mask_id=103)))
    seed, _ = seed_with_half(mlm_thr(0.8), 4242, n, high=True)
    out.append(dict(name="boundary-replace", ids=ids.copy(), kw=dict(p_select=1.0, p_replace=0.8, seed=seed, site=4242, special_ids=(), mask_id=103)))
    return out


# The dQ kernel regenerates the mask on its own (per-row seeds, four consecutive keys per lane), so it gets a read-back of its own.
# Q = 0 leaves the scores at 0 whatever K holds: K carries the code over the keys, V and dctx are the unit column 0 of every head.
# Then dP[i][j] = keep * scale, delta[i] = ctx[i][0] (the kernel's own bf16 context), dS[i][j] = (keep * scale - delta[i]) / n on the
# live keys, and   dQ[i][c] * 8 n = scale * m - delta[i] * W[c],   m the integer of the keep flags of keys c + 64 g as before, W[c] the
# same sum over all live keys of the column.  Roundings: bf16 dS (two distinct values per row) and the bf16 output, <= 31 * 2^-7 again.
def readback_inputs_dq(lens, heads):
    """(qkv [M, 3H], dctx [M, H]) float32: Q = 0, K = ``readback_code`` in every head, V = dctx = 1 in column 0 of every head."""
    code = np.concatenate([np.tile(readback_code(S), (1, heads)) for S in lens])
    H = heads * 64
    qkv = np.zeros((code.shape[0], 3 * H), dtype=np.float32)
    qkv[:, H:2 * H] = code
    unit = np.zeros((code.shape[0], H), dtype=np.float32)
    unit[:, ::64] = 1.0
    qkv[:, 2 * H:] = unit
    return qkv, unit.copy()


def decode_dq(dq_block, ctx_col0, live, scale, what=""):
    """One (sequence, head) block [S, 64] of dQ and column 0 of the kernel's context for the same block [S] -> uint8 [S, S] decoded
    keep flags of (query i, key j), 0 at the keys that are not live."""
    S = live.size
    n = int(live.sum())
    W = _pack_rows(live[None, :].astype(np.uint8), S)[0].astype(np.float64)
    x = (np.asarray(dq_block, dtype=np.float64) * 8.0 * n + np.asarray(ctx_col0, dtype=np.float64)[:, None] * W[None, :]) / scale
    k = np.rint(x)
    res = float(np.abs(x - k).max()) if x.size else 0.0
    assert res < READBACK_RESIDUAL, f"{what}: value {res:.3f} away from an integer: not a mask read-back"
    k = k.astype(np.int64)
    flags = _bits_to_flags(k, S) * live[None, :].astype(np.uint8)
    assert (k >= 0).all() and np.array_equal(_pack_rows(flags, S), k), f"{what}: weight outside the live keys"
    return flags
