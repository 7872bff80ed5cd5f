"""A float64 reference for the embedding-stage kernels (csrc/rowwise.hip) and the bounds their outputs are checked against.

Not a test module (pytest does not collect it): ``from tests import embed_ref as E``.

``gather`` / ``scatter`` / ``rows_sum`` / ``pair_fwd`` / ``pair_bwd`` with ``emu=False`` are the reference: plain float64 torch on the
CPU, on the exact inputs the kernels get (fp32 tables and weights; bf16 d, J and dJ; float64 pair features rounded to fp32 first, as
the reference's ``.float()`` does, REF:MMBertEmbedding.py:62,64).  With id' = id for 0 <= id < V and 0 otherwise, tt' = (tt != 0)
(0 without token types):

    gather     out[i] = bf16(word[id'_i] + type[tt'_i] + pos[i mod T])
    scatter    gword[id] = prior + sum_{i: id_i = id, 0 < id < V} d[i]     (row 0 = padding_idx: never written)
               gpos[p]   = prior + sum_{i mod T = p} d[i];   gtype[t] = prior + sum_{tt'_i = t} d[i]
    run sums   dst[row_of(key)] += sum_{i: key_i = key} src[i]   (mmbert_id_runs_sum_rows; row_of = key, or its index in ``union``)
    rows_to_block  block[pos(id)] += rows[i]                     (ids outside (0, V) or not in the union skipped)
    pair fwd   out[b*(T'+P) + T' + p, h] = bf16(relu(sum_k W[h,k] f[b,p,k] + bias[h]))   (T', base shift: ops._pair_rows)
    pair bwd   g = dJ * [J_bf16 > 0];  dW[h,k] = prior + sum_r g[r,h] f[r,k];  db[h] = prior + sum_r g[r,h]

Each returns ``rowwise_ref.Ref`` objects (value, ``acc``, ``exact``), checked by ``rowwise_ref.check``:

    elementwise   |got - ref| <= C_OUT u_out |ref| + C_ACC 2^-24 acc          (C_OUT = 2, C_ACC = 1; u_out 2^-8 bf16, 2^-23 fp32)
    normwise      per row, with TAU_OUT = 0.8, TAU_ACC = 0.25 (rowwise_ref)

The ``acc`` of a sum follows the order the kernel documents.  A serial fp32 chain carries the running error bound of its own
partial sums, sum_j |S_j| (the prior included where the chain starts on it); a fold of partials the same over the fold's partial
sums; one add onto the prior |prior + t|.  The two products carry gemm_ref's sqrt(L) sum|a b| for an MFMA chain of length L:

    gather     acc = |word| + |type| + |pos| + |out|                  (two fp32 adds, any association: -ffast-math)
    gpos       chain over the position's rows (i ascending) from 0, then one add onto the prior          (one adder per address)
    gtype      per-position chains from 0, then atomic: a chain of the partials onto the prior (arrival order);
               deterministic: a fold of the slab in position order from 0, then one add onto the prior
    gword      atomic: one chain onto the prior per id (arrival order); deterministic (id_runs_sum_rows): per 8192-row launch,
               G strided chains (G = min(8, 1024 / (H/4))) from 0, folded in g order, one add onto the destination
    pair fwd   acc = F_CHAIN (sqrt(D) sum_k |W f| + |pre|)            (f32 MFMA chain over ascending k within 128-wide chunks, bias)
    pair bwd   acc = F_CHAIN (sqrt(rows per wave) sum_r |g f| + the four waves' fold + the slabs' range-order fold + |prior + t|)

Arrival-order chains are modelled in ascending row order; the emulation replays them ascending, descending and in random orders.
Relu needs no case of its own (1-Lipschitz: the pre-activation's bound covers it); an output whose pre-activation lies more than
its bound below zero must be +0 exactly (``exact``).  Rows of gword never referenced (row 0 included), gpos rows at or past
min(T, n) and a token-type row no row has keep their prior bit for bit.

``emu=True`` is the emulation, for calibration only: the same sums with one fp32 rounding per add in the documented order, bf16
stores by RNE.  The library is built with -ffast-math, so nothing asserts bit equality with it.  It takes value-only mutations
(``Mutation``) that the CPU test uses to show the bounds are tight.

Calibration (tests/test_embed_reference_cpu.py: every case there, both modes, the atomic sums replayed ascending, descending and
in two random orders) and the MI355X over tests/test_embed_gpu.py (both modes).  Largest ratios (elementwise / normwise) with

    C_OUT = 2, C_ACC = 1, TAU_OUT = 0.8, TAU_ACC = 0.25, F_CHAIN = 2

    output       emulation      MI355X
    gather       0.50  0.47     0.50  0.47
    gword        0.21  0.19     0.21  0.19
    gpos         0.10  0.07     0.14  0.11
    gtype        0.03  0.03     0.03  0.04
    run sums     0.21  0.17     0.30  0.21     (rows_to_block, scatter_add_rows_ordered)
    pair out     0.50  0.45     0.50  0.46
    dW           0.29  0.44     0.32  0.47
    db           0.03  0.02     0.06  0.06

The bf16 outputs sit at 0.5: their final rounding, as in gemm_ref (C_OUT = 2).  What the calibration forced.  The running error
bound of a chain can be reached by a single add: a partial sum just above a power of two rounds by 2^-24 of itself and the next
add cancels it (two word rows of opposite sign onto the prior reached 0.96 at F_CHAIN = 1), hence F_CHAIN = 2.  An atomic chain's
order is not known, and the bound of one order does not hold for another (the ascending model against the descending replay:
4.1), hence the order-free m |prior| + sqrt(m) sum |x| for arrival-order chains.  The products' sqrt(L) sum |a b| is a typical
size, not a bound: the rows scaled by 2^10 carry most of a weight gradient's column, every later add of their chain rounds at
their size, and a row of dW shares it (normwise 0.51 at F_CHAIN = 1 over a 96-row chain).

The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math

import torch

from tests.gemm_ref import CUS, Canary, _bf, _f32  # noqa: F401  (Canary re-exported for the tests)
from tests.rowwise_ref import C_ACC, EPS24, U_BF16, U_F32, Mutation, Ref, _hook, check, ratios  # noqa: F401  (check, ratios too)

RUNS_MAXN = 8192             # ops.scatter_add_rows_ordered: rows per launch of mmbert_id_runs_sum_rows (its LDS list)
BATCH = 8                    # embed_scatter_kernel: a position's rows in batches of 8
PAIR_NT = 5                  # pair_wgrad_kernel: 16-column tiles per workgroup (grid.z slices beyond)
CLS, SEP, MASK = 101, 102, 103
F_CHAIN = 2.0                # sums: acc = F_CHAIN sum_j |S_j| (a single add can reach its bound: see the module docstring)


# ------------------------------------------------------------------------------------------------ launch geometry (csrc/rowwise.hip)
def runs_groups(H):
    """G of mmbert_id_runs_sum_rows: row groups of H / 4 column threads in a workgroup of at most 1024 (at least 64) threads."""
    ct = H // 4
    g = max(1, min(8, 1024 // ct))
    return max(64, g * ct) // ct


def pair_bwd_split(n, D, H, cus=CUS):
    """(rows per range, ranges S) of mmbert_pair_proj_bwd: about one workgroup per CU, ranges a multiple of 64 rows."""
    htiles, zt = (H + 63) // 64, ((D + 1 + 15) // 16 + PAIR_NT - 1) // PAIR_NT
    want = max(1, (cus + htiles * zt - 1) // (htiles * zt))
    rp = max(64, ((n + want - 1) // want + 63) // 64 * 64)
    return rp, (n + rp - 1) // rp


def pair_rows(B, P, T, seq_len=None, offset=None):
    """Output rows of the pair block in launch order: b*(T+P) + T + p, or b*seq_len + offset + p."""
    b, p = torch.arange(B)[:, None], torch.arange(P)[None, :]
    rows = b * (T + P) + T + p if seq_len is None else b * seq_len + offset + p
    return rows.reshape(-1)


# ------------------------------------------------------------------------------------------------ chains
def _order(loc, order):
    """Rows grouped by ``loc`` (ascending), each group's rows ascending, descending or in a random order (an int seed).
    Returns (perm, rank): the rows in that order and each one's place in its group."""
    n = loc.numel()
    if order == "asc":
        tie = torch.arange(n)
    elif order == "desc":
        tie = -torch.arange(n)
    else:
        tie = torch.randperm(n, generator=torch.Generator().manual_seed(int(order)))
    o = torch.argsort(tie, stable=True)
    o = o[torch.argsort(loc[o], stable=True)]
    ls = loc[o]
    counts = torch.bincount(ls, minlength=int(ls.max()) + 1 if n else 0)
    starts = torch.cumsum(counts, 0) - counts
    rank = torch.arange(n) - starts[ls]
    return o, rank


def _chain(X, loc, K, start=None, order="asc", emu=False, arrival=False):
    """Per group k < K the fp32 chain start[k] + X[rows of k] (one rounding per add, in ``order``).  Returns (value, acc): the
    emulated fp32 values or the exact float64 ones, and acc = F_CHAIN sum_j |S_j| over the exact partial sums (the start included),
    or with ``arrival`` (atomics: the order is not known) F_CHAIN (m |start| + sqrt(m) sum_i |x_i|) for a chain of m terms."""
    H = X.shape[1]
    st = torch.zeros(K, H, dtype=torch.float64) if start is None else start.to(torch.float64)
    if loc.numel() == 0:
        return st.clone(), torch.zeros(K, H, dtype=torch.float64)
    perm, rank = _order(loc, order)
    if emu:
        v = st.clone()
        ls = loc[perm]
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            g = ls[sel]
            v[g] = _f32(v[g] + X[perm[sel]])
        return v, None
    if arrival:
        m = torch.bincount(loc, minlength=K).to(torch.float64)[:, None]
        ax = torch.zeros(K, X.shape[1], dtype=torch.float64).index_add_(0, loc, X.abs())
        val = st + torch.zeros(K, X.shape[1], dtype=torch.float64).index_add_(0, loc, X)
        return val, F_CHAIN * (m * st.abs() + m.sqrt() * ax)
    Xs, ls = X[perm], loc[perm]
    cs = torch.cumsum(Xs, 0)
    first = rank == 0
    base = torch.zeros(K, H, dtype=torch.float64)
    base[ls[first]] = cs[first] - Xs[first]
    S = st[ls] + cs - base[ls]
    acc = F_CHAIN * torch.zeros(K, H, dtype=torch.float64).index_add_(0, ls, S.abs())
    val = st + torch.zeros(K, H, dtype=torch.float64).index_add_(0, loc, X)
    return val, acc


def _fold(parts, start=None, emu=False):
    """fp32 fold of parts [K, G, H] in g order from 0 (from ``start`` when given).  Returns (value, acc = sum_j |prefix_j|)."""
    if emu:
        t = torch.zeros_like(parts[:, 0]) if start is None else start.clone()
        for g in range(parts.shape[1]):
            t = _f32(t + parts[:, g])
        return t, None
    pre = torch.cumsum(parts, 1)
    if start is not None:
        pre = pre + start[:, None]
    return pre[:, -1] if parts.shape[1] else start, F_CHAIN * pre.abs().sum(1)


def _det_runs(X, loc, ok, K, start, G, emu=False, mutation=None):
    """mmbert_id_runs_sum_rows through ops.scatter_add_rows_ordered: per launch of RUNS_MAXN rows (of all n, valid or not), each key's
    rows (ascending) in G strided chains from 0, the chains folded in g order, one add onto the destination; launches in order.
    Returns (value, acc)."""
    n, H = X.shape[0], X.shape[1]
    cur, acc = start.clone(), torch.zeros(K, H, dtype=torch.float64)
    seen = torch.zeros(K, dtype=torch.bool)
    for li, off in enumerate(range(0, n, RUNS_MAXN)):
        sel = off + torch.nonzero(ok[off:off + RUNS_MAXN]).flatten()
        lc, Xc = loc[sel], X[sel]
        perm, rank = _order(lc, "asc")
        rk = torch.empty_like(rank)
        rk[perm] = rank                                               # each row's place in its key's list (ascending i)
        P, a1 = _chain(Xc, lc * G + rk % G, K * G, emu=emu)
        t, a2 = _fold(P.view(K, G, H), emu=emu)
        here = torch.zeros(K, dtype=torch.bool)
        here[lc] = True
        add = _hook(mutation, "launch_add", here, seen=seen, launch=li)
        if emu:
            cur = torch.where(add[:, None], _f32(cur + t), cur)
        else:
            cur = torch.where(add[:, None], cur + t, cur)
            acc += torch.where(here[:, None], a1.view(K, G, H).sum(1) + a2 + F_CHAIN * cur.abs(), torch.zeros_like(cur))
        seen |= here
    return cur, acc


# ------------------------------------------------------------------------------------------------ mutations
def padding_row_written():
    return Mutation("gradient reaches padding row 0", {"word_valid": lambda ok, ctx: (ctx["ids"] >= 0) & (ctx["ids"] < ctx["V"])})


def out_of_range_from_last_row():
    return Mutation("out-of-range id read from row V-1",
                    {"gather_id": lambda idp, ctx: torch.where((ctx["ids"] < 0) | (ctx["ids"] >= ctx["V"]), ctx["V"] - 1, idp)})


def position_shifted_on_one_sequence(seq=1):
    def f(pos, ctx):
        i, T = torch.arange(pos.numel()), ctx["T"]
        return torch.where(i // T == seq, (i + 1) % T, pos)
    return Mutation(f"position (i+1) mod T on sequence {seq}", {"pos_of_row": f})


def token_types_swapped_at(p=3):
    return Mutation(f"token types swapped at position {p}",
                    {"tt": lambda tt, ctx: torch.where(torch.arange(tt.numel()) % ctx["T"] == p, 1 - tt, tt)})


def prior_overwritten(what):
    return Mutation(f"{what}: prior overwritten", {f"prior_{what}": lambda x, ctx: torch.zeros_like(x)})


def word_run_row_dropped(id_):
    """The last row of id_'s run carries no word gradient."""
    def f(keep, ctx):
        ids = ctx["ids"]
        hit = torch.nonzero(ids == id_).flatten()
        keep = keep.clone()
        keep[hit[-1]] = False
        return keep
    return Mutation(f"one row of the id {id_} run dropped", {"word_rows": f})


def last_partial_batch_dropped():
    """The rows of a position past its last full batch of 8 are lost from the position loop (position, type and atomic word sums)."""
    def f(live, ctx):
        n, T = live.numel(), ctx["T"]
        i = torch.arange(n)
        m = torch.bincount(i % T, minlength=T)[i % T]
        return live & ((i // T) < (m // BATCH) * BATCH)
    return Mutation("last partial 8-row batch of a position dropped", {"scatter_rows": f})


def split_run_counted_once():
    return Mutation("a run split at the 8192-row launch boundary counted once",
                    {"launch_add": lambda here, ctx: here & ~ctx["seen"] if ctx["launch"] > 0 else here})


def chunk_last_k_lost(k=127):
    return Mutation(f"feature k = {k} (last of a 128-wide chunk) lost",
                    {"fwd_kmask": lambda m, ctx: torch.where(torch.arange(m.numel()) == k, 0.0, m)})


def bias_neighbour():
    return Mutation("bias from the neighbouring column", {"bias": lambda b, ctx: torch.cat([b[1:], b[-1:]])})


def features_bf16():
    return Mutation("features rounded to bf16 instead of fp32", {"feat": lambda f, ctx: _bf(f)})


def last_range_dropped():
    return Mutation("the last row range dropped from the slab sum", {"slab_keep": lambda k, ctx: torch.arange(k.numel()) < k.numel() - 1})


def second_zslice_lost():
    return Mutation("the second z-slice's columns lost", {"zslice": lambda c, ctx: c & (torch.arange(c.numel()) < PAIR_NT * 16)})


def last_range_wave_lost():
    """The last wave that holds rows of the last (short) range loses them."""
    def f(g, ctx):
        n, rp, S = ctx["n"], ctx["rp"], ctx["S"]
        rpw = rp // 4
        w = (n - 1 - (S - 1) * rp) // rpw
        lo = (S - 1) * rp + w * rpw
        g = g.clone()
        g[lo:min(lo + rpw, n)] = 0.0
        return g
    return Mutation("one wave's rows of the last range lost", {"pair_g": f})


# ------------------------------------------------------------------------------------------------ the embedding stage
def _idp(ids, V, mutation=None):
    idp = torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids))
    return _hook(mutation, "gather_id", idp, ids=ids, V=V)


def _ttp(tts, n, T, mutation=None):
    tt = torch.zeros(n, dtype=torch.long) if tts is None else (tts != 0).long()
    return _hook(mutation, "tt", tt, T=T)


def _pos(n, T, mutation=None):
    return _hook(mutation, "pos_of_row", torch.arange(n) % T, T=T)


def gather(ids, tts, word, type_, pos, T, *, emu=False, mutation=None):
    """mmbert_embed_gather on CPU tensors: ids / tts int64 [n], fp32 tables.  Ref [n, H] (bf16 out), or the emulated tensor."""
    n, V = ids.numel(), word.shape[0]
    w = word.to(torch.float64)[_idp(ids, V, mutation)]
    t = type_.to(torch.float64)[_ttp(tts, n, T, mutation)]
    p = pos.to(torch.float64)[_pos(n, T, mutation)]
    if emu:
        return _bf(_f32(_f32(w + t) + p))
    val = w + t + p
    return Ref(val, w.abs() + t.abs() + p.abs() + val.abs(), 0.0, U_BF16)


def _touched_rows(ids, V):
    """Word rows a Ref compares: every id in the batch clamped into the table, plus rows 0 and V-1."""
    return torch.unique(torch.cat([ids.clamp(0, V - 1), torch.tensor([0, V - 1])]))


def rows_sum(keys, src, dst0, V, *, union=None, det=False, order="asc", live=None, emu=False, mutation=None, what="rows"):
    """dst0[row_of(key_i)] += src[i] (ids outside (0, V), or not in ``union``, skipped): the scatter's word rows (``union`` None:
    row_of = key, dst0 = the word table), mmbert_rows_to_block and ops.scatter_add_rows_ordered (``union``: row_of = the key's index,
    dst0 = the [U, H] block).  ``det``: the ordered kernel's association; else one atomic per row in ``order``.  ``live``: rows the
    caller's loop reaches.  Returns a Ref on the compared rows (``rows``), or (rows, emulated values)."""
    keys = keys.reshape(-1).long()
    X = src.to(torch.float64)
    H = X.shape[1]
    ok = _hook(mutation, "word_valid", (keys > 0) & (keys < V), ids=keys, V=V)
    if live is not None:
        ok = ok & live
    ok = _hook(mutation, "word_rows", ok, ids=keys)
    if union is None:
        rows = _touched_rows(keys, V)
        dest = keys.clamp(0, V - 1)
    else:
        union = union.long()
        rows = torch.arange(union.numel())
        dest = torch.searchsorted(union, keys).clamp(max=max(union.numel() - 1, 0))
        ok = ok & (union[dest] == keys) if union.numel() else torch.zeros_like(ok)
    loc = torch.searchsorted(rows, dest)
    K = rows.numel()
    prior = _hook(mutation, f"prior_{what}", dst0[rows].to(torch.float64))
    sel = torch.nonzero(ok).flatten()
    if det:
        val, acc = _det_runs(X, loc, ok, K, prior, runs_groups(H), emu=emu, mutation=mutation)
    else:
        val, acc = _chain(X[sel], loc[sel], K, start=prior, order=order, emu=emu, arrival=True)
    if emu:
        return rows, val
    hit = torch.zeros(K, dtype=torch.bool)
    hit[loc[sel]] = True
    exact = torch.where(hit[:, None], torch.full_like(val, float("nan")), dst0[rows].to(torch.float64))
    return Ref(val, acc, 0.0, U_F32, rows, exact)


def scatter(ids, tts, d, T, gword0, gtype0, gpos0, *, V=None, det=False, order="asc", emu=False, mutation=None):
    """mmbert_embed_scatter (+ the ordered word rows of ops.embed_scatter in deterministic mode) on CPU tensors: ids / tts int64 [n],
    d bf16 [n, H], priors fp32 (gword0 None: no word rows; V from ``V``).  Returns {"gword": Ref (rows: _touched_rows), "gtype": Ref
    [2, H], "gpos": Ref [rows of gpos0, H]}, or the emulated tensors (gword: (rows, values))."""
    n, H = d.shape
    ids = ids.reshape(-1).long()
    V = gword0.shape[0] if gword0 is not None else int(V)
    X = d.to(torch.float64)
    live = _hook(mutation, "scatter_rows", torch.ones(n, dtype=torch.bool), T=T)
    pos = _pos(n, T, mutation)
    tt = _ttp(tts, n, T, mutation)
    out = {}
    if gword0 is not None:
        out["gword"] = rows_sum(ids, d, gword0, V, det=det, order=order, live=None if det else live, emu=emu, mutation=mutation,
                                what="gword")
    sel = torch.nonzero(live).flatten()
    # positions: one chain per position from 0 (i ascending), one add onto the prior
    Tp = gpos0.shape[0]
    pprior = _hook(mutation, "prior_gpos", gpos0.to(torch.float64))
    ps, pacc = _chain(X[sel], pos[sel], Tp, emu=emu)
    nwg = min(T, n)
    w = torch.arange(Tp) < nwg
    gpos = torch.where(w[:, None], _f32(pprior + ps) if emu else pprior + ps, pprior)
    # token types: per-position chains from 0, then the partials onto the prior (atomics) or a position-order fold (deterministic)
    tprior = _hook(mutation, "prior_gtype", gtype0.to(torch.float64))
    tp, tacc = _chain(X[sel], (pos[sel] * 2 + tt[sel]), 2 * nwg, emu=emu)
    parts = tp.view(nwg, 2, H).transpose(0, 1)                        # [type, position, H]
    pacc_t = None if emu else tacc.view(nwg, 2, H).sum(0)
    if det:
        t, facc = _fold(parts, emu=emu)
        gtype = _f32(tprior + t) if emu else tprior + t
        if not emu:
            facc = facc + F_CHAIN * gtype.abs()
    else:
        ploc = torch.arange(2)[:, None].expand(2, nwg).reshape(-1)
        gtype, facc = _chain(parts.reshape(2 * nwg, H), ploc, 2, start=tprior, order=order, emu=emu, arrival=True)
    if emu:
        out.update(gtype=gtype, gpos=gpos)
        return out
    tused = torch.zeros(2, dtype=torch.bool)
    tused[tt[sel]] = True
    texact = torch.where(tused[:, None], torch.full_like(gtype, float("nan")), gtype0.to(torch.float64))
    out["gtype"] = Ref(gtype, pacc_t + facc, 0.0, U_F32, None, texact)
    pex = torch.where(w[:, None], torch.full_like(gpos, float("nan")), gpos0.to(torch.float64))
    out["gpos"] = Ref(gpos, pacc + F_CHAIN * gpos.abs(), 0.0, U_F32, None, pex)
    return out


# ------------------------------------------------------------------------------------------------ the pair projections
def _feat(feat, mutation=None):
    """Pair features [B, P, D] (fp32 or float64) as the kernels read them: rounded to fp32 (``.float()``), as float64 [n, D]."""
    B, P, D = feat.shape
    return _hook(mutation, "feat", feat.reshape(B * P, D).to(torch.float32).to(torch.float64))


def pair_fwd(feat, W, bias, *, rows=None, emu=False, mutation=None):
    """mmbert_pair_proj_fwd on CPU tensors: feat [B, P, D], W [H, D] / bias [H] fp32.  Ref [B*P, H] on the output ``rows`` (the
    caller's pair_rows), or the emulated bf16 values."""
    f = _feat(feat, mutation)
    D = f.shape[1]
    Wd = W.to(torch.float64) * _hook(mutation, "fwd_kmask", torch.ones(D, dtype=torch.float64))[None, :]
    b = _hook(mutation, "bias", bias.to(torch.float64))
    if emu:
        acc = torch.zeros(f.shape[0], W.shape[0], dtype=torch.float64)
        for k in range(D):
            acc = _f32(acc + f[:, k:k + 1] * Wd[None, :, k])
        return _bf(_f32(acc + b[None, :]).clamp(min=0.0))
    pre = f @ Wd.t() + b[None, :]
    acc = F_CHAIN * (math.sqrt(D) * (f.abs() @ W.to(torch.float64).abs().t()) + pre.abs())
    val = pre.clamp(min=0.0)
    exact = torch.where(pre + C_ACC * EPS24 * acc < 0, torch.zeros_like(pre), torch.full_like(pre, float("nan")))
    return Ref(val, acc, 0.0, U_BF16, rows, exact)


def pair_bwd(feat, J, dJ, dW0, db0, *, cus=CUS, emu=False, mutation=None):
    """mmbert_pair_proj_bwd on CPU tensors: feat [B, P, D], J / dJ bf16 [B*P, H] (the pair block's rows, in launch order), priors
    dW0 [H, D] / db0 [H] fp32.  Returns {"dW": Ref, "db": Ref}, or the emulated tensors.  ``cus``: the device's compute units (the
    row ranges)."""
    f = _feat(feat, mutation)
    n, D = f.shape
    H = J.shape[1]
    F1 = torch.cat([f, torch.ones(n, 1, dtype=torch.float64)], 1)     # column D = 1: the bias gradient
    rp, S = pair_bwd_split(n, D, H, cus)
    rpw = rp // 4
    g = dJ.to(torch.float64) * (J.to(torch.float64) > 0)
    g = _hook(mutation, "pair_g", g, n=n, rp=rp, S=S)
    Gp = torch.zeros(S * rp, H, dtype=torch.float64)
    Fp = torch.zeros(S * rp, D + 1, dtype=torch.float64)
    Gp[:n], Fp[:n] = g, F1
    Gp, Fp = Gp.view(S * 4, rpw, H), Fp.view(S * 4, rpw, D + 1)
    keep = _hook(mutation, "slab_keep", torch.ones(S, dtype=torch.bool))
    cols = _hook(mutation, "zslice", torch.ones(D + 1, dtype=torch.bool))
    prior = torch.cat([_hook(mutation, "prior_dW", dW0.to(torch.float64)), _hook(mutation, "prior_db", db0.to(torch.float64))[:, None]], 1)
    if emu:
        acc = torch.zeros(S * 4, H, D + 1, dtype=torch.float64)
        for r in range(rpw):
            acc = _f32(acc + Gp[:, r, :, None] * Fp[:, r, None, :])
        w4 = acc.view(S, 4, H, D + 1)
        slab = _f32(_f32(_f32(w4[:, 0] + w4[:, 1]) + w4[:, 2]) + w4[:, 3])
        t = torch.zeros(H, D + 1, dtype=torch.float64)
        for s in range(S):
            if keep[s]:
                t = _f32(t + slab[s])
        out = torch.where(cols[None, :], _f32(prior + t), prior)
        return {"dW": out[:, :D], "db": out[:, D]}
    part = torch.bmm(Gp.transpose(1, 2), Fp)                           # [S*4, H, D+1]: the waves' exact partial products
    chain = F_CHAIN * math.sqrt(rpw) * (g.abs().t() @ F1.abs())
    w4 = part.view(S, 4, H, D + 1)
    wfold = torch.cumsum(w4, 1)[:, 1:].abs().sum((0, 1))
    slab = w4.sum(1)
    sfold = torch.cumsum(slab, 0).abs().sum(0)
    val = prior + slab.sum(0)
    acc = chain + F_CHAIN * (wfold + sfold + val.abs())
    return {"dW": Ref(val[:, :D], acc[:, :D], 0.0, U_F32), "db": Ref(val[:, D], acc[:, D], 0.0, U_F32)}


# ------------------------------------------------------------------------------------------------ test inputs
def make_ids(B, T, V, seed, *, mask_frac=0.12, odd=True):
    """Token ids [B*T] as the step sees them: [CLS] = 101 at every position 0, a [SEP] after 0.5 T .. T - 2 word tokens, padding
    tails of id 0, about ``mask_frac`` of the words [MASK] = 103; with ``odd`` a few ids V - 1 and ids out of range (-1, V, V + 7:
    the kernels map them to row 0).  Token types [B*T]: 0 on the first half of the words, 1 on the rest and the [SEP], 0 on padding."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, T, dtype=torch.long)
    tts = torch.zeros(B, T, dtype=torch.long)
    lo = min(1000, V - 1)
    for b in range(B):
        L = int(torch.randint(max(1, T // 2), max(2, T - 1), (1,), generator=g))
        w = torch.randint(lo, V, (L,), generator=g)
        w[torch.rand(L, generator=g) < mask_frac] = MASK
        ids[b, 0] = CLS
        ids[b, 1:1 + L] = w[:T - 2]
        ids[b, min(1 + L, T - 1)] = SEP
        tts[b, 1 + L // 2:min(2 + L, T)] = 1
    ids = ids.reshape(-1)
    if odd and ids.numel() > 64:
        words = torch.nonzero(ids >= lo).flatten()
        pick = words[torch.randperm(words.numel(), generator=g)[:6]]
        ids[pick] = torch.tensor([V - 1, V - 1, -1, V, V + 7, V - 1])[:pick.numel()]
    return ids, tts.reshape(-1)


def make_tables(V, H, Tpos, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.05 * torch.randn(V, H, generator=g), 0.05 * torch.randn(2, H, generator=g), 0.05 * torch.randn(Tpos, H, generator=g))


def make_d(n, H, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(n, H, generator=g)).to(torch.bfloat16)


def make_pair(B, P, D, H, seed, *, dtype=torch.float32, zero_rows=True, scaled_rows=True):
    """feat [B, P, D] (``dtype``): N(0, 1) rows, trailing rows of zeros per sample (masked frames), rows scaled by 2^+10 / 2^-10;
    W [H, D] with the reference's Linear init scale, bias [H]."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, P, D, generator=g, dtype=torch.float64)
    if zero_rows and P > 2:
        for b in range(B):
            f[b, P - 1 - b % max(1, P // 4):] = 0.0
    if scaled_rows and P > 4:
        f[:, 1] *= 2.0 ** 10
        f[:, 2] *= 2.0 ** -10
    W = torch.randn(H, D, generator=g) / math.sqrt(D)
    bias = 0.1 * torch.randn(H, generator=g)
    return f.to(dtype), W, bias
