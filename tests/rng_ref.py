"""An independent integer reference of the counter-based generator behind every dropout mask and the MLM mask, and the exact
comparison the GPU file (tests/test_rng_gpu.py) makes against it (its cases and read-back codecs: tests/rng_cases.py).

Not a test module (pytest does not collect it): ``from tests import rng_ref as R``.  numpy integers only; it never calls the
library.  Written from the definition in csrc/common.h and csrc/rowwise.hip:

    hash32(x)            x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16          (mod 2^32)
    rng_stream(seed, site) = hash32(a ^ b * 0x9E3779B1 ^ hash32(site * 0x85EBCA6B + 0x27D4EB2F)),
                         a = hash32(low word of seed ^ 0xA511E9B3), b = hash32(high word of seed + 0x7F4A7C15)
    thr16(p)             0 for p <= 0, else trunc(min(float32(p) * 65536 + 0.5, 65535)): drop probability thr16 / 65536
    pair_bits(stream, q) x = q * 0x9E3779B1 + stream; x ^= x >> 16; x *= 0x2C1B3C6D; x ^= x >> 16           (mod 2^32)
    keep(element idx)    word = pair_bits(stream, (idx >> 1) mod 2^32), idx a 64-bit index; its half = the low 16 bits for an even
                         idx, the high 16 for an odd one; kept iff the half read as SIGNED 16-bit >= thr16 - 32768

Attention: the keep flag of P[i][j] of sequence s, head h is that of element elem_base[s] + h*S*Spad + i*Spad + j, Spad = S rounded up
to 4, the bases laid out back to back over the sequences (each rounded up to 4) as ops.SeqLayout does.

MLM mask: element i draws ONE word, pair_bits(stream, i mod 2^32); it is selected iff its id is no special id and the low half,
UNSIGNED, is < round(p_select * 65536); a selected element is replaced by mask_id iff the high half, unsigned, is <
round(p_replace * 65536) (65536 for p = 1: every half is below it).  labels = the original id where selected, -100 elsewhere.

``rho`` is the Pearson correlation of two 0/1 vectors from their counts, the statistic of the stream-pair survey
(tests/test_rng_reference_cpu.py).
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
WEYL = 0x9E3779B1
PAIR_MUL = 0x2C1B3C6D
U64 = np.uint64


def _u(x):
    return np.asarray(x, dtype=np.uint64) & U64(M32)


def hash32(x):
    """The two-multiply finaliser that derives streams (arrays or ints, computed in 64-bit integers and reduced mod 2^32)."""
    x = _u(x)
    x = x ^ (x >> U64(16))
    x = (x * U64(0x85EBCA6B)) & U64(M32)
    x = x ^ (x >> U64(13))
    x = (x * U64(0xC2B2AE35)) & U64(M32)
    x = x ^ (x >> U64(16))
    return x


def rng_stream(seed64: int, site32: int) -> int:
    seed64, site32 = int(seed64) & 0xFFFFFFFFFFFFFFFF, int(site32) & M32
    a = int(hash32((seed64 & M32) ^ 0xA511E9B3))
    b = int(hash32(((seed64 >> 32) + 0x7F4A7C15) & M32))
    c = int(hash32((site32 * 0x85EBCA6B + 0x27D4EB2F) & M32))
    return int(hash32(a ^ ((b * WEYL) & M32) ^ c))


def thr16(p) -> int:
    p = float(np.float32(p))                               # the C entry point takes a float
    if p <= 0.0:
        return 0
    return int(min(p * 65536.0 + 0.5, 65535.0))


def drop_scale(t16: int) -> float:
    return 1.0 / (1.0 - t16 / 65536.0)


def pair_bits(stream, pair_idx):
    """The 32-bit word of pair ``pair_idx`` (ints or arrays, taken mod 2^32) as uint64 values below 2^32."""
    x = (_u(pair_idx) * U64(WEYL) + _u(stream)) & U64(M32)
    x = x ^ (x >> U64(16))
    x = (x * U64(PAIR_MUL)) & U64(M32)
    x = x ^ (x >> U64(16))
    return x


def _signed16(v):
    v = np.asarray(v, dtype=np.int64) & 0xFFFF
    return np.where(v >= 32768, v - 65536, v)


def keep_at(stream, idx, t16):
    """Keep flags (uint8) of the elements with the 64-bit indices ``idx`` (any shape)."""
    idx = np.asarray(idx, dtype=np.uint64)
    h = pair_bits(stream, idx >> U64(1))
    half = np.where((idx & U64(1)) == 1, h >> U64(16), h & U64(0xFFFF))
    return (_signed16(half) >= _signed16((int(t16) - 32768) & 0xFFFF)).astype(np.uint8)


def keep(stream, idx0, n, t16):
    """Keep flags of the n elements idx0, idx0 + 1, ... (idx0 a 64-bit element index)."""
    return keep_at(stream, np.arange(n, dtype=np.uint64) + U64(int(idx0)), t16)


# ------------------------------------------------------------------------------------------------ attention index scheme
def ceil4(x: int) -> int:
    return (x + 3) // 4 * 4


def seq_elem_bases(lens, heads):
    """elem_base of every sequence as ops.SeqLayout lays them out, and the end of the index space."""
    out, e = [], 0
    for S in lens:
        out.append(e)
        e = ceil4(e + heads * S * ceil4(S))
    return out, e


def last_base(S, heads):
    """The largest multiple of 4 at which the last head of a sequence of length S still ends at or below 2^32."""
    return (2 ** 32 - heads * S * ceil4(S)) // 4 * 4


def attn_keep(stream, elem_base, S, heads, t16):
    """[heads, S, S] keep flags of one sequence (element (h, i, j) at elem_base + h*S*Spad + i*Spad + j)."""
    Spad = ceil4(S)
    h, i, j = np.meshgrid(np.arange(heads, dtype=np.uint64), np.arange(S, dtype=np.uint64), np.arange(S, dtype=np.uint64), indexing="ij")
    return keep_at(stream, U64(int(elem_base)) + h * U64(S * Spad) + i * U64(Spad) + j, t16)


def base_bits32(bases):
    """uint32 bases as the int32 bit patterns they travel as."""
    return [b - 2 ** 32 if b >= 2 ** 31 else b for b in bases]


# ------------------------------------------------------------------------------------------------ MLM mask
def mlm_thr(p) -> int:
    return int(round(p * 65536))


def mlm_mask(ids, p_select, p_replace, seed, site, special_ids, mask_id):
    """(new ids, labels) as int64 arrays of ids' shape; element i of the flattened ids draws word i."""
    ids = np.asarray(ids, dtype=np.int64)
    flat = ids.reshape(-1)
    h = pair_bits(rng_stream(seed, site), np.arange(flat.size, dtype=np.uint64))
    lo, hi = (h & U64(0xFFFF)).astype(np.int64), (h >> U64(16)).astype(np.int64)
    special = np.isin(flat, np.asarray(list(special_ids), dtype=np.int64)) if len(special_ids) else np.zeros(flat.size, dtype=bool)
    sel = ~special & (lo < mlm_thr(p_select))
    labels = np.where(sel, flat, -100)
    out = np.where(sel & (hi < mlm_thr(p_replace)), np.int64(mask_id), flat)
    return out.reshape(ids.shape), labels.reshape(ids.shape)


# ------------------------------------------------------------------------------------------------ the statistic of the survey
def rho_counts(n, na, nb, nab):
    """Pearson correlation of two 0/1 vectors of length n with na and nb ones, nab of them common (arrays or numbers)."""
    n, na, nb, nab = (np.asarray(x, dtype=np.float64) for x in (n, na, nb, nab))
    return (n * nab - na * nb) / np.sqrt(na * (n - na) * nb * (n - nb))


def rho(a, b):
    a, b = np.asarray(a).reshape(-1) != 0, np.asarray(b).reshape(-1) != 0
    return float(rho_counts(a.size, a.sum(), b.sum(), (a & b).sum()))


def stream_halves(streams, pair0, npairs):
    """int16 [len(streams), 2 * npairs]: the signed halves of the words pair0 .. pair0 + npairs - 1 of every stream in element order (the
    fast form for the survey: wrapping uint32 arithmetic; tests/test_rng_reference_cpu.py holds it to ``pair_bits``)."""
    assert np.little_endian
    q = (np.arange(pair0, pair0 + npairs, dtype=np.uint64) * U64(WEYL)).astype(np.uint32)
    x = q[None, :] + np.asarray(streams, dtype=np.uint64).astype(np.uint32)[:, None]
    x ^= x >> np.uint32(16)
    x *= np.uint32(PAIR_MUL)
    x ^= x >> np.uint32(16)
    return x.view(np.int16)                                  # little endian: the low half is the even element


# ------------------------------------------------------------------------------------------------ exact comparison
def check_equal(got, want, what=""):
    """THE comparison of the GPU file: integer arrays equal element for element (no tolerance)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype.kind in "iub" and want.dtype.kind in "iub", (what, got.dtype, want.dtype)
    bad = np.nonzero(got.astype(np.int64) != want.astype(np.int64))
    if bad[0].size:
        first = [tuple(int(b[k]) for b in bad) for k in range(min(5, bad[0].size))]
        raise AssertionError(f"{what}: {bad[0].size} of {got.size} elements differ, first at {first}")
