"""An exact reference for the kernels of csrc/rowwise.hip that do no accumulation: the step prologue, the valid-first split layout and
its row maps, the row-movement kernels, the casts and transposes, and the counter RNG behind the dropout and MLM masks.

Not a test module (pytest does not collect it): ``from tests import layout_ref as L``.

Every output of these kernels is a copy, an index, a count, one rounding or one mask conversion, so it must match bit for bit and
the reference needs no error analysis.  It is plain numpy (int64, and bit-level floats through ``view``), written from the rules the
kernels document, never by calling ``msa_amd.ops``:

    prologue     key bias (1 - f32(m)) * -10000 in two fp32 roundings (the reference's extended attention mask), -1e30 in the padding
                 slots up to ceil128(S); a position no segment covers reads m = 1, where segments overlap the first one wins.
                 live key: bias > -10000.  kv_len = 1 + the last live key, S when there is none.  labelled: label != -100; counted:
                 0 <= label < V; bad: labelled and not counted.  valid = max(kv_len, 1 + the last labelled position).
                 idx = the counted rows, ascending; words = valid[0..nseq) | #counted | #counted position-0 rows | #bad.
                 row-set mode: active = position 0, or a live key, or labelled, or every position of a sequence without a live key;
                 valid = #active; rank = position in the order (active rows, then the others, each group in its order); the key
                 bias again in that order, -1e30 behind S.
    split layout v = min(valid, len); start_a / start_b exclusive prefix sums of v / len - v (start_b behind rows_a); region-A tiles
                 (s, k < ceil(v / rows)), region-B tiles (s, k < ceil((len - v) / rows)), each list sorted by (r // xs, k, r % xs),
                 r = stable rank of -v, xs = 8 / gcd(heads, 8); unused entries sequence -1 (and 0 in the other three fields).
    split rows   p = rank or position; p < v: row start_a + p (own); mode 0: start_b + p - v (own); mode 1: start_b, owned by p == v;
                 mode 2: rows_a (owned by none).  inv[i] = that row, perm[row] = i where owned; nothing else is written.
    row movement active_rows = the counted rows ascending; compact_rows out[i] = map[cat(rows, extra)[i]] and, with an inverse,
                 table[out[i]] = stamp << 32 | i; scatter_rows_zero dst[r] = src[i] when table[r] holds the current stamp and
                 i < nlist, a zero row otherwise; gather_rows and pack_i64 are byte copies (pack: constant runs for fill segments).
    casts        f32 -> bf16: round to nearest even on the bit pattern; subnormals are kept (no flush); a NaN keeps its sign and its
                 upper payload bits and is made quiet: (bits >> 16) | 0x40.  bf16 -> f32: bits << 16 (NaNs unchanged).
                 (Both measured on gfx950: v_cvt_pk_bf16_f32, fp32 denormals on.)
    transpose    dst[c][r] = cast(src[r][c]) for r < rows, c < cols; zero for rows <= r < min(dst_ld, ceil64(rows)) (the last row
                 tile's padding); nothing else.  A bf16 source goes through fp32 (exact), so only its NaNs change: made quiet.
    RNG          hash32 / pair_mix as in common.h; pair_bits(stream, j) = pair_mix(j * 0x9E3779B1 + stream); element idx uses half
                 (idx & 1) of pair_bits(stream, idx >> 1), low half first; keep iff (half ^ 0x8000) >= thr16 (the signed compare of
                 common.h, stated unsigned; thr16 <= 65535, mmbert_dropout_thr16's cap).  mlm: ONE word per element, pair_bits(stream, i): low half < sel_thr selects (never a
                 special id), high half < rep_thr replaces the id by mask_id; labels = id where selected, -100 elsewhere.

Next to the reference, numpy ports of each kernel's ALGORITHM (``*_port``): the 256-wide chunks with their ballot prefix and the
carried ``base``, the per-sequence rank / place loops of split_layout, the stamp test, the vec16 / 4-byte copy loops, the grid-stride
loops with the launch's grid cap, the full / edge tile split and the binary search over ``tile0``.  Each port takes ``mut``: the name
of one value-level mutation (``MUTANTS``) that tests/test_layout_reference_cpu.py applies to show that the shapes used here and on the
GPU (``*_CASES``) catch it.
"""
from __future__ import annotations

import math

import numpy as np

NO_KEY = np.float32(-1.0e30)
U32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ bits and casts
def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def bf16_rne(bits32):
    """uint32 fp32 bit patterns -> uint16 bf16 bit patterns (the measured gfx950 rule: RNE, subnormals kept, NaN quieted)."""
    b = np.asarray(bits32, dtype=np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    rne = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (b >> 16) | 0x40, rne).astype(np.uint16)


def bf16_to_f32_bits(bits16):
    return np.asarray(bits16, dtype=np.uint32) << 16


def cast_port(bits32, mut=None):
    """cast_f32_bf16_kernel's f2bf as a port (the mutants: truncation, NaN payload dropped, subnormals flushed)."""
    b = np.asarray(bits32, dtype=np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    if mut == "cast_truncates":
        out = b >> 16
    else:
        out = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    if mut == "cast_flushes_subnormals":
        out = np.where((b & 0x7F800000) == 0, (b >> 16) & 0x8000, out)
    q = (b >> 16) | 0x40 if mut != "cast_canonical_nan" else (b >> 16) & 0x8000 | 0x7FC0
    return np.where(nan, q, out & 0xFFFF).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ step prologue
def key_bias(m32):
    m32 = np.asarray(m32, dtype=np.float32)
    return ((np.float32(1.0) - m32).astype(np.float32) * np.float32(-10000.0)).astype(np.float32)


def _seq_mask(segs, p, b, S, first_wins=True):
    """fp32 mask of sequence b of pass p: 1 where no segment covers; ``segs`` = [(fp32 [B, len], pass, offset)]."""
    m = np.ones(S, dtype=np.float32)
    done = np.zeros(S, dtype=bool)
    order = segs if first_wins else segs[::-1]
    for arr, sp, off in order:
        if sp != p:
            continue
        n = arr.shape[1]
        lo, hi = max(off, 0), min(off + n, S)
        if lo >= hi:
            continue
        pos = np.arange(lo, hi)
        take = ~done[pos]
        m[pos[take]] = np.asarray(arr[b, pos[take] - off], dtype=np.float32)
        done[pos] = True
    return m


def prologue_ref(segs, pass_lens, B, labels, vocab, rowset=False):
    """The documented rule of mmbert_prologue (both modes) on fp32 masks: a dict of numpy arrays in the kernel's output layout."""
    npass = len(pass_lens)
    nseq = npass * B
    slots = [(S + 127) // 128 * 128 for S in pass_lens]
    kb_all = np.full(sum(B * s for s in slots), NO_KEY, dtype=np.float32)
    kbp_all = kb_all.copy()
    tokens = sum(B * S for S in pass_lens)
    rank = np.zeros(tokens, dtype=np.int64)
    kv, valid, cnt, first, bad = (np.zeros(nseq, dtype=np.int64) for _ in range(5))
    idx = []
    row, slot = 0, 0
    for p, S in enumerate(pass_lens):
        for b in range(B):
            s = p * B + b
            r0, k0 = row + b * S, slot + b * slots[p]
            bias = key_bias(_seq_mask(segs, p, b, S))
            kb_all[k0:k0 + S] = bias
            live = bias > np.float32(-10000.0)
            kv[s] = (np.nonzero(live)[0][-1] + 1) if live.any() else S
            lab = labels[r0:r0 + S] if labels is not None else np.full(S, -100, dtype=np.int64)
            labelled = lab != -100
            ok = (lab >= 0) & (lab < vocab)
            cnt[s], first[s], bad[s] = ok.sum(), int(S > 0 and ok[0]), (labelled & ~ok).sum()
            idx.extend((r0 + np.nonzero(ok)[0]).tolist())
            last_lab = np.nonzero(labelled)[0][-1] if labelled.any() else -1
            valid[s] = max(kv[s], last_lab + 1)
            if rowset:
                active = live | labelled | (not live.any())
                if S:
                    active[0] = True
                order = np.concatenate((np.nonzero(active)[0], np.nonzero(~active)[0]))
                rank[r0 + order] = np.arange(S)
                kbp_all[k0:k0 + S] = bias[order]
                valid[s] = active.sum()
        row += B * S
        slot += B * slots[p]
    words = np.concatenate((valid, [cnt.sum(), first.sum(), bad.sum()]))
    out = dict(key_bias=kb_all, kv_len=kv, valid=valid, seq_cnt=np.concatenate((cnt, first, bad)), idx=np.asarray(idx, dtype=np.int64),
               words=words)
    if rowset:
        out.update(rank=rank, key_bias_perm=kbp_all)
    return out


def _ballot_chunks(act, base0, mut=None, carry="rank"):
    """The kernels' 256-position chunk loop: per 64-lane wave a ballot and the popcount of the lanes below, per workgroup the wave
    counts in front, and ``base`` carried from chunk to chunk.  Returns the exclusive prefix count of every position."""
    n = act.size
    out = np.zeros(n, dtype=np.int64)
    base = base0
    for p0 in range(0, max(n, 1), 256):
        a = np.zeros(256, dtype=np.int64)
        seg = act[p0:p0 + 256]
        a[:seg.size] = seg
        w = a.reshape(4, 64)
        before = np.cumsum(w, axis=1) - w                           # popcount(ballot & lanes below)
        wsum = w.sum(axis=1)
        off = base + np.concatenate(([0], np.cumsum(wsum)[:-1]))
        out[p0:p0 + seg.size] = (off[:, None] + before).reshape(-1)[:seg.size]
        if mut != f"no_base_carry_{carry}":
            base += int(wsum.sum())
    return out


def prologue_port(segs, pass_lens, B, labels, vocab, rowset=False, mut=None):
    """prologue_seq_kernel + prologue_rows_kernel as a numpy port (per workgroup = sequence)."""
    npass = len(pass_lens)
    nseq = npass * B
    slots = [(S + 127) // 128 * 128 for S in pass_lens]
    kb_all = np.full(sum(B * s for s in slots), NO_KEY, dtype=np.float32)
    kbp_all = kb_all.copy()
    tokens = sum(B * S for S in pass_lens)
    rank = np.zeros(tokens, dtype=np.int64)
    kv, valid, cnt, first, bad = (np.zeros(nseq, dtype=np.int64) for _ in range(5))
    idx = np.zeros(max(tokens, 1), dtype=np.int64)
    row_of = []
    row, slot = 0, 0
    for p, S in enumerate(pass_lens):
        for b in range(B):
            s = p * B + b
            r0, k0 = row + b * S, slot + b * slots[p]
            row_of.append((r0, S))
            m = _seq_mask(segs, p, b, S, first_wins=mut != "last_segment_wins")
            if mut == "uncovered_reads_zero":
                cov = np.zeros(S, dtype=bool)
                for arr, sp, off in segs:
                    if sp == p:
                        cov[max(off, 0):min(off + arr.shape[1], S)] = True
                m = np.where(cov, m, np.float32(0))
            if mut == "bias_one_rounding":
                bias = (m.astype(np.float64) * 10000.0 - 10000.0).astype(np.float32)
            else:
                bias = ((np.float32(1.0) - m).astype(np.float32) * np.float32(-10000.0)).astype(np.float32)
            kb_all[k0:k0 + S] = bias
            pos = np.arange(S)
            live = bias > np.float32(-10000.0) if mut != "live_key_ge" else bias >= np.float32(-10000.0)
            last_key = pos[live].max() if live.any() else -1
            lab = labels[r0:r0 + S] if labels is not None else None
            if lab is not None:
                labelled = lab != -100
                ok = (lab >= 0) & (lab < vocab) if mut != "bad_label_counted" else labelled
                last_lab = pos[labelled].max() if labelled.any() else -1
                cnt[s], first[s], bad[s] = ok.sum(), int(S > 0 and ok[0]), (labelled & ~ok).sum()
            else:
                labelled = np.zeros(S, dtype=bool)
                last_lab = -1
            kv[s] = S if last_key < 0 else last_key + 1
            if not rowset:
                valid[s] = max(kv[s], last_lab + 1) if mut != "valid_ignores_last_lab" else kv[s]
                continue
            every = last_key < 0 and mut != "no_every_rule"
            active = every | live | labelled
            if S and mut != "no_position0_rule":
                active[0] = True
            nact = int(active.sum())
            valid[s] = nact
            ab = _ballot_chunks(active, 0, mut, "rank")
            np_ = np.where(active, ab, nact + (pos - ab))
            rank[r0 + pos] = np_
            inside = (np_ >= 0) & (np_ < slots[p])                    # (a mutant may place a row outside the sequence's slots)
            kbp_all[k0 + np_[inside]] = bias[inside]
        row += B * S
        slot += B * slots[p]
    if labels is not None:
        base_of = np.concatenate(([0], np.cumsum(cnt)[:-1]))
        for s, (r0, S) in enumerate(row_of):
            if cnt[s] == 0:
                continue
            lab = labels[r0:r0 + S]
            ok = (lab >= 0) & (lab < vocab) if mut != "bad_label_counted" else lab != -100
            at = _ballot_chunks(ok, int(base_of[s]), mut, "idx")
            idx[at[ok]] = r0 + np.nonzero(ok)[0]
    words = np.concatenate((valid, [cnt.sum(), first.sum(), bad.sum()]))
    n = int(cnt.sum())
    out = dict(key_bias=kb_all, kv_len=kv, valid=valid, seq_cnt=np.concatenate((cnt, first, bad)), idx=idx[:n], words=words)
    if rowset:
        out.update(rank=rank, key_bias_perm=kbp_all)
    return out


def prologue_case(name):
    """Deterministic prologue inputs shared by the CPU and GPU tests: (fp32 masks as [(array [B, len], pass, offset)], pass_lens, B,
    labels int64 or None, vocab, rowset)."""
    c = PROLOGUE_CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, lens, V = c["B"], c["lens"], c.get("V", 30522)
    segs = []
    for p, S in enumerate(lens):
        for (off, n, kind) in c["segs"](p, S):
            if kind == "text":
                keep = rng.integers(1, n + 1, size=B)
                arr = (np.arange(n)[None, :] < keep[:, None]).astype(np.float32)
            elif kind == "ones":
                arr = np.ones((B, n), dtype=np.float32)
            elif kind == "zeros":
                arr = np.zeros((B, n), dtype=np.float32)
            elif kind == "frac":
                arr = rng.choice(np.array([0.0, 1.0, 0.3, 0.7, 3e-8, 1e-9, 0.123456, 0.999, -0.5, 2.0, 1.0 / 35, 34.0 / 35], np.float32),
                                 size=(B, n))
            else:                                                  # "pairs": a live prefix of random length, a few dead frames inside
                keep = rng.integers(0, n + 1, size=B)
                arr = (np.arange(n)[None, :] < keep[:, None]).astype(np.float32)
                arr[rng.random((B, n)) < 0.05] = 0.0
            segs.append((arr, p, off))
    tokens = B * sum(lens)
    lab = c.get("labels", "mlm")
    if lab is None:
        labels = None
    else:
        labels = np.full(tokens, -100, dtype=np.int64)
        if lab == "mlm":
            sel = rng.random(tokens) < 0.15
            labels[sel] = rng.integers(0, V, size=int(sel.sum()))
            extra = rng.integers(0, tokens, size=8)
            labels[extra] = np.array([-1, V, V + 9, np.iinfo(np.int64).min, 0, V - 1, -101, 5])[:extra.size]
            labels[0] = 7                                              # a labelled position-0 row
        elif lab == "all":
            labels[:] = rng.integers(0, V, size=tokens)
        elif lab == "sparse":
            sel = rng.random(tokens) < 0.02
            labels[sel] = rng.integers(0, V, size=int(sel.sum()))
    if "edit" in c:
        c["edit"](segs, labels, B, lens)
    return segs, lens, B, labels, V, c.get("rowset", False)


def _text_pairs(T, parts):
    def f(p, S):
        if p == 0:
            return [(0, T, "text")]
        return [(0, T, "ones")] + [(o, n, "pairs") for o, n in parts[p - 1]]
    return f


def _thirds(S):
    return [(0, S // 3, "text"), (S // 3, S // 3, "pairs"), (2 * (S // 3), S - 2 * (S // 3), "pairs")]


def _edit_special(segs, labels, B, lens):
    """Sequence 0 of pass 0: every key masked; sequence 1: only position 0 live; labels past the last live key of sequence 2;
    sequence 3: position 0 masked and unlabelled while later keys are live."""
    arr = segs[0][0]
    arr[0, :] = 0.0
    if B > 1:
        arr[1, :] = 0.0
        arr[1, 0] = 1.0
    if B > 3:
        arr[3, :] = 1.0
        arr[3, 0] = 0.0
        if labels is not None:
            labels[3 * lens[0]] = -100
    if labels is not None and B > 2:
        S = lens[0]
        labels[2 * S + S - 1] = 3
        labels[0 * S:1 * S] = -100
        labels[1 * S + 1] = 11


def _edit_overlap(segs, labels, B, lens):
    segs.append((np.zeros((B, 40), dtype=np.float32), 0, 5))       # overlaps the first segment: the first one wins
    segs.append((np.full((B, 7), 0.5, dtype=np.float32), 1, lens[1] - 7))


PROLOGUE_CASES = {
    # the real step's segment sets (synthetic values): headline, bert-large, the fused 1050-row sequence, B = 128 three passes
    "headline": dict(seed=1, B=16, lens=[50, 550, 550], segs=_text_pairs(50, [[(50, 500)], [(50, 500)]])),
    "bert_large": dict(seed=2, B=32, lens=[40, 80, 80], segs=_text_pairs(40, [[(40, 40)], [(40, 40)]])),
    "fused_rowset": dict(seed=3, B=4, lens=[1050], rowset=True,
                         segs=lambda p, S: [(0, 50, "text"), (50, 500, "pairs"), (550, 500, "pairs")]),
    "b128": dict(seed=4, B=128, lens=[50, 114, 97], segs=_text_pairs(50, [[(50, 64)], [(50, 47)]])),
    # synthetic: chunk edges (S in 1, 127..129, 255..257, 513), fractional masks, uncovered and overlapping segments
    "chunks": dict(seed=5, B=3, lens=[1, 127, 128, 129], segs=lambda p, S: [(0, S, "pairs")]),
    "chunks2": dict(seed=6, B=3, lens=[255, 256, 257, 513], segs=lambda p, S: _thirds(S)),              # 4 passes, 12 segments
    "chunks2_rowset": dict(seed=6, B=3, lens=[255, 256, 257, 513], rowset=True, segs=lambda p, S: _thirds(S)),
    "frac": dict(seed=7, B=4, lens=[300, 70], segs=lambda p, S: [(0, S - 9, "frac")]),
    "frac_rowset": dict(seed=7, B=4, lens=[300, 70], rowset=True, segs=lambda p, S: [(0, S - 9, "frac")]),
    "overlap": dict(seed=8, B=3, lens=[60, 90, 45, 300], segs=lambda p, S: [(0, 20, "text"), (30, S - 40, "pairs")], edit=_edit_overlap),
    "special": dict(seed=9, B=4, lens=[270, 40], segs=lambda p, S: [(0, S, "pairs")], edit=_edit_special),
    "special_rowset": dict(seed=9, B=4, lens=[270, 40], rowset=True, segs=lambda p, S: [(0, S, "pairs")], edit=_edit_special),
    "nolabels": dict(seed=10, B=5, lens=[300], labels=None, segs=lambda p, S: [(0, S, "pairs")]),
    "all_labelled": dict(seed=11, B=2, lens=[260, 7], labels="all", rowset=True, segs=lambda p, S: [(0, S, "zeros")]),
    "all_ignored": dict(seed=12, B=2, lens=[200], labels="none", segs=lambda p, S: [(0, S, "pairs")]),
}


# ------------------------------------------------------------------------------------------------ split layout and row maps
def xs_of(heads):
    return 8 // math.gcd(heads, 8)


def split_layout_ref(lens, valid, heads, rows, nf_max, nq_max):
    """The int32 output of mmbert_split_layout by the documented rule (sorted tile keys)."""
    lens = np.asarray(lens, dtype=np.int64)
    ns = lens.size
    v = np.minimum(np.asarray(valid, dtype=np.int64), lens)
    xs = xs_of(heads)
    start_a = np.concatenate(([0], np.cumsum(v)[:-1])) if ns else v
    rows_a = int(v.sum())
    start_b = rows_a + np.concatenate(([0], np.cumsum(lens - v)[:-1]))
    rk = np.empty(ns, dtype=np.int64)
    rk[sorted(range(ns), key=lambda s: (-v[s], s))] = np.arange(ns)

    def tiles(count, regionB):
        t = [(rk[s] // xs, k, rk[s] % xs, s) for s in range(ns) for k in range(-(-int(count[s]) // rows))]
        t.sort()
        out = []
        for _, k, _, s in t:
            if regionB:
                out.append((s, v[s] + k * rows, start_b[s] - v[s], lens[s]))
            else:
                out.append((s, k * rows, start_a[s], v[s]))
        return out

    A, Bt = tiles(v, False), tiles(lens - v, True)
    f, q = A + Bt, A

    def block(lst, nmax):
        a = np.zeros((4, nmax), dtype=np.int64)
        a[0, :] = -1
        for j, e in enumerate(lst):
            a[:, j] = e
        return a.reshape(-1)

    return np.concatenate((block(f, nf_max), block(q, nq_max), start_a, v, start_b, [len(f), len(q), rows_a, 0])).astype(np.int64)


def split_layout_port(lens, valid, heads, rows, nf_max, nq_max, mut=None):
    """split_layout_kernel as a port: per-sequence rank and prefix sums by walking the others, tiles placed by counting."""
    ln = np.asarray(lens, dtype=np.int64)
    ns = ln.size
    v = np.minimum(np.asarray(valid, dtype=np.int64), ln)
    xs = xs_of(heads) * (2 if mut == "xs_doubled" else 1)
    rk, sa, sb = np.zeros(ns, np.int64), np.zeros(ns, np.int64), np.zeros(ns, np.int64)
    for s in range(ns):
        t = np.arange(ns)
        tie = (t < s) if mut != "rank_tie_reversed" else (t > s)
        rk[s] = int(((v > v[s]) | ((v == v[s]) & tie)).sum())
        sa[s] = int(v[:s].sum())
        sb[s] = int((ln[:s] - v[:s]).sum())
    rows_a = int(v.sum())
    sb += rows_a
    out = np.zeros(4 * nf_max + 4 * nq_max + 3 * ns + 4, dtype=np.int64)
    f = out[:4 * nf_max].reshape(4, nf_max)
    q = out[4 * nf_max:4 * nf_max + 4 * nq_max].reshape(4, nq_max)

    def place(regionB, base):
        cntr = (ln - v) if regionB else v
        ntr = np.zeros(ns, np.int64)
        ntr[rk] = (cntr + rows - 1) // rows
        for s in range(ns):
            r = rk[s]
            n = ntr[r]
            g, m = r // xs, r % xs
            before = int(ntr[:g * xs].sum())
            for k in range(n):
                pos = before
                for m2 in range(xs):
                    if g * xs + m2 >= ns:
                        break
                    n2 = ntr[g * xs + m2]
                    pos += min(n2, k) + (1 if (n2 > k and m2 < m) else 0)
                first = (v[s] + (1 if mut == "regionB_first_row_off_by_one" else 0)) if regionB else 0
                shift = sb[s] - v[s] if regionB else sa[s]
                end = ln[s] if regionB else v[s]
                f[:, base + pos] = (s, first + k * rows, shift, end)
                if not regionB:
                    q[:, pos] = (s, k * rows, shift, end)
        return int(ntr.sum())

    nA = place(False, 0)
    nf = nA + place(True, nA)
    f[0, nf:] = -1 if mut != "no_minus_one_fill" else 0
    f[1:, nf:] = 0
    q[0, nA:] = -1 if mut != "no_minus_one_fill" else 0
    q[1:, nA:] = 0
    tail = out[4 * nf_max + 4 * nq_max:]
    tail[:ns], tail[ns:2 * ns], tail[2 * ns:3 * ns] = sa, v, sb
    tail[3 * ns:] = (nf, nA, rows_a, 0)
    return out


def split_rows_ref(lens, valid, mode, rank=None):
    """(perm, inv, owned) of mmbert_split_rows over the packed rows of ``lens``, with the starts of the same layout (mode 2: rows_a as
    the region-B start); perm entries that no row owns are reported by ``owned`` = False (the kernel leaves them alone)."""
    lens = np.asarray(lens, dtype=np.int64)
    v = np.minimum(np.asarray(valid, dtype=np.int64), lens)
    start_a = np.concatenate(([0], np.cumsum(v)[:-1]))
    rows_a = int(v.sum())
    if mode == 0:
        start_b = rows_a + np.concatenate(([0], np.cumsum(lens - v)[:-1]))
        n_packed = int(lens.sum())
    elif mode == 1:
        start_b = rows_a + np.concatenate(([0], np.cumsum(np.minimum(lens - v, 1))[:-1]))
        n_packed = rows_a + int(np.minimum(lens - v, 1).sum())
    else:
        start_b = np.full_like(start_a, rows_a)
        n_packed = rows_a
    M = int(lens.sum())
    inv = np.zeros(M, dtype=np.int64)
    perm = np.zeros(n_packed + 1, dtype=np.int64)
    owned = np.zeros(n_packed + 1, dtype=bool)
    i = 0
    for s, n in enumerate(lens):
        for pos in range(n):
            p = int(rank[i]) if rank is not None else pos
            if p < v[s]:
                r, own = start_a[s] + p, True
            elif mode == 0:
                r, own = start_b[s] + p - v[s], True
            elif mode == 1:
                r, own = start_b[s], p == v[s]
            else:
                r, own = rows_a, False
            inv[i] = r
            if own:
                perm[r], owned[r] = i, True
            i += 1
    return perm[:n_packed], inv, owned[:n_packed], dict(start_a=start_a, start_b=start_b, v=v, rows_a=rows_a, n_packed=n_packed)


def split_rows_port(row_seq, row_pos, start_a, start_b, valid, mode, rows_a, n_packed, rank=None, mut=None):
    """split_rows_kernel, vectorised over the threads."""
    s = np.asarray(row_seq, dtype=np.int64)
    p = np.asarray(rank if rank is not None and mut != "rank_ignored" else row_pos, dtype=np.int64)
    v = np.asarray(valid, dtype=np.int64)[s]
    sa, sb = np.asarray(start_a, np.int64)[s], np.asarray(start_b, np.int64)[s]
    inA = p < v
    n = np.full(s.size, rows_a, dtype=np.int64)
    own = inA.copy()
    n[inA] = sa[inA] + p[inA]
    if mode == 0:
        n[~inA] = sb[~inA] + p[~inA] - v[~inA]
        own[:] = True
    elif mode == 1:
        n[~inA] = sb[~inA]
        own |= p == (v + 1 if mut == "mode1_owner_off_by_one" else v)
    perm = np.zeros(n_packed + 1, dtype=np.int64)
    owned = np.zeros(n_packed + 1, dtype=bool)
    perm[n[own]] = np.nonzero(own)[0]
    owned[n[own]] = True
    return perm[:n_packed], n, owned[:n_packed]


SPLIT_CASES = {
    # (lens, valid, heads); valid generated where None
    "headline_12": dict(lens=[50] * 16 + [550] * 32, heads=12, seed=1),
    "large_16": dict(lens=[40] * 32 + [80] * 64, heads=16, seed=2),
    "two_heads_384": dict(lens=[300] * 128 + [57] * 256, heads=2, seed=3),
    "one_head_1024": dict(lens=None, heads=1, seed=4),
    "eight_heads_ties": dict(lens=[129] * 40 + [1] * 8, heads=8, seed=5, ties=True),
    "three_heads_zero": dict(lens=[64, 65, 1, 300, 128, 127], heads=3, seed=6, valid=[0, 65, 1, 0, 200, 64]),
    "four_heads_1": dict(lens=[550], heads=4, seed=7, valid=[600]),
}


def split_case(name):
    c = SPLIT_CASES[name]
    rng = np.random.default_rng(c["seed"])
    lens = c["lens"] if c["lens"] is not None else rng.integers(1, 200, size=1024).tolist()
    if "valid" in c:
        valid = list(c["valid"])
    elif c.get("ties"):
        valid = rng.choice([0, 64, 128, 129, 1], size=len(lens)).tolist()
    else:
        valid = [int(rng.integers(0, n + 1)) for n in lens]
        for j in range(0, len(lens), 7):
            valid[j] = lens[j] + int(rng.integers(0, 3))             # valid = len and valid > len
    return lens, valid, c["heads"]


# ------------------------------------------------------------------------------------------------ row movement
def active_rows_ref(labels, V):
    labels = np.asarray(labels, dtype=np.int64)
    return np.nonzero((labels >= 0) & (labels < V))[0]


def active_rows_port(labels, V, mut=None):
    """active_rows_kernel: 1024-row chunks, 16 waves, base carried."""
    labels = np.asarray(labels, dtype=np.int64)
    M = labels.size
    act = (labels >= 0) & (labels < V)
    out = np.zeros(max(M, 1), dtype=np.int64)
    base = 0
    for i0 in range(0, M, 1024):
        a = np.zeros(1024, dtype=np.int64)
        seg = act[i0:i0 + 1024]
        a[:seg.size] = seg
        w = a.reshape(16, 64)
        before = np.cumsum(w, axis=1) - w
        off = base + np.concatenate(([0], np.cumsum(w.sum(1))[:-1]))
        at = (off[:, None] + before).reshape(-1)[:seg.size]
        out[at[seg]] = i0 + np.nonzero(seg)[0]
        if mut != "no_base_carry_active":
            base += int(w.sum())
    return out[:base] if mut != "no_base_carry_active" else out[:int(act.sum())]


ACTIVE_M = [0, 1, 1023, 1024, 1025, 2400, 18400, 70400, 300000]


def active_labels(M, seed=0, V=30522):
    rng = np.random.default_rng(seed + M)
    lab = np.full(M, -100, dtype=np.int64)
    sel = rng.random(M) < 0.15
    lab[sel] = rng.integers(0, V, size=int(sel.sum()))
    if M > 10:
        lab[rng.integers(0, M, size=5)] = [-1, V, V + 9, np.iinfo(np.int64).min, V - 1]
    if M > 1023:
        lab[1023] = 5                                                 # both sides of the first chunk edge
    if M > 1024:
        lab[1024] = 6
    return lab


def next_stamp(stamp):
    """RowInverse.next: never 0, wraps after 0xFFFFFFF0."""
    return stamp % 0xFFFFFFF0 + 1


def compact_ref(rows, extra, row_map=None):
    r = np.concatenate((np.asarray(rows, dtype=np.int64), np.asarray(extra, dtype=np.int64)))
    return np.asarray(row_map, dtype=np.int64)[r] if row_map is not None else r


def stamp_table_ref(table, out, stamp):
    t = np.array(table, dtype=np.int64, copy=True)
    t[out] = ((np.uint64(stamp) << np.uint64(32)) | np.arange(out.size, dtype=np.uint64)).view(np.int64)
    return t


def scatter_ref(table, stamp, nlist, nrows):
    """Which list entry every destination row r < nrows takes (-1: a zero row)."""
    t = np.asarray(table[:nrows], dtype=np.int64).view(np.uint64)
    hit = ((t >> np.uint64(32)) == np.uint64(stamp)) & ((t & np.uint64(U32)) < np.uint64(nlist))
    return np.where(hit, (t & np.uint64(U32)).astype(np.int64), -1)


def scatter_port(table, stamp, nlist, nrows, mut=None):
    v = np.asarray(table[:nrows], dtype=np.int64)
    i = (v & U32).astype(np.int64)
    i = np.where(i >= 2 ** 31, i - 2 ** 32, i)                        # (int) of the low half
    stamp_hi = np.array([int(stamp) << 32], dtype=np.uint64).view(np.int64)[0]
    same = (v & ~np.int64(U32)) == stamp_hi
    if mut == "stale_stamp_accepted":
        same = np.ones_like(same)
    ok = i < nlist if mut != "no_nlist_check" else np.ones_like(same)
    return np.where(same & ok, i, -1)


def copy_rows(src, idx):
    """Byte rows: ``src`` uint8 [n, row_bytes] -> rows ``idx`` (-1: zeros)."""
    src = np.asarray(src, dtype=np.uint8)
    out = np.zeros((len(idx), src.shape[1]), dtype=np.uint8)
    ok = np.asarray(idx) >= 0
    out[ok] = src[np.asarray(idx)[ok]]
    return out


def gather_port(src, idx, vec16, mut=None):
    """gather_rows_kernel on byte rows: 16-byte pieces (vec16) or 4-byte pieces up to row_bytes."""
    src = np.asarray(src, dtype=np.uint8)
    rb = src.shape[1]
    out = np.zeros((len(idx), rb), dtype=np.uint8)
    step = 16 if vec16 else 4
    end = rb - rb % 16 if mut == "gather_drops_tail" else rb
    for b in range(0, end, step):
        out[:, b:b + step] = src[idx, b:b + step]
    return out


def pack_ref(segments):
    """segments: int64 arrays or (count, fill) -> the concatenation."""
    parts = [np.asarray(s, dtype=np.int64).reshape(-1) if not isinstance(s, tuple) else np.full(s[0], s[1], dtype=np.int64) for s in segments]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def pack_port(segments, mut=None):
    """pack_i64_kernel: grid (min(ceil(most / 256), 256), nseg), a grid-stride loop per segment."""
    cnts = [len(s) if not isinstance(s, tuple) else s[0] for s in segments]
    offs = np.concatenate(([0], np.cumsum(cnts)[:-1])).astype(np.int64)
    out = np.full(int(sum(cnts)), -7, dtype=np.int64)
    most = max(cnts) if cnts else 0
    grid = min(max((most + 255) // 256, 1), 256)
    for k, s in enumerate(segments):
        n = cnts[k]
        i = np.arange(grid * 256, dtype=np.int64)
        while True:
            i = i[i < n]
            if i.size == 0:
                break
            out[offs[k] + i] = np.asarray(s, dtype=np.int64).reshape(-1)[i] if not isinstance(s, tuple) else s[1]
            if mut == "pack_one_pass":
                break
            i = i + grid * 256
    return out


# ------------------------------------------------------------------------------------------------ transposes
def tdesc(src_off, dst_off, rows, cols, dst_ld, tile0):
    return (int(src_off), int(dst_off), int(rows), int(cols), int(dst_ld), int(tile0))


def tdesc_raw(descs):
    """[n, 4] int64: the TransDesc struct {long long src_off, dst_off; int rows, cols, dst_ld, tile0} as ops expects it."""
    raw = np.zeros((len(descs), 4), dtype=np.int64)
    for j, (so, do, r, c, ld, t0) in enumerate(descs):
        raw[j] = (so, do, np.int64(r) | (np.int64(c) << 32), np.int64(ld) | (np.int64(t0) << 32))
    return raw


def build_descs(mats):
    """[(src_off, dst_off, rows, cols, dst_ld)] -> descriptors with their first-tile numbers, and the tile total."""
    out, t0 = [], 0
    for so, do, r, c, ld in mats:
        out.append(tdesc(so, do, r, c, ld, t0))
        t0 += ((r + 63) // 64) * ((c + 63) // 64)
    return out, t0


def transpose_ref(src_bits, dst_bits, descs, src_bf16=False):
    """uint32 (fp32) or uint16 (bf16) source bits, uint16 destination bits (updated copy returned)."""
    dst = np.array(dst_bits, dtype=np.uint16, copy=True)
    src = np.asarray(src_bits)
    for so, do, r, c, ld, _ in descs:
        if r == 0 or c == 0:
            continue
        a = src[so:so + r * c].reshape(r, c)
        bits = bf16_rne(bf16_to_f32_bits(a) if src_bf16 else a.astype(np.uint32))
        view = dst[do:do + c * ld].reshape(c, ld)
        view[:, :r] = bits.T
        view[:, r:min(ld, (r + 63) // 64 * 64)] = 0
    return dst


def transpose_port(src_bits, dst_bits, descs, ntiles, src_bf16=False, mut=None):
    """transpose_cast_kernel: per 64 x 64 tile, the descriptor by binary search over tile0, the full (aligned interior) or edge path."""
    dst = np.array(dst_bits, dtype=np.uint16, copy=True)
    src = np.asarray(src_bits)
    nd = len(descs)
    for blk in range(ntiles):
        lo, hi = 0, nd - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if (blk > descs[mid][5]) if mut == "search_one_early" else (blk >= descs[mid][5]):
                lo = mid
            else:
                hi = mid - 1
        so, do, rows, cols, ld, t0 = descs[lo]
        tl = blk - t0
        tc = (cols + 63) >> 6
        r0, c0 = (tl // tc) << 6, (tl % tc) << 6
        full = (r0 + 64 <= rows and c0 + 64 <= cols and r0 + 64 <= ld and not (cols & 3) and not (ld & 7) and not (so & 3) and not (do & 7))
        r = np.arange(64)[:, None]
        c = np.arange(64)[None, :]

        def cvt(x):
            x = bf16_to_f32_bits(x) if src_bf16 else x.astype(np.uint32)
            return cast_port(x, "cast_truncates" if mut == "transpose_truncates" else None)
        if full:
            t = src[so + (r0 + r) * cols + c0 + c]
            dst[do + (c0 + c.T) * ld + r0 + r.T] = cvt(t).T
            continue
        inside = (r0 + r < rows) & (c0 + c < cols)
        t = np.zeros((64, 64), dtype=src.dtype)
        t[inside] = src[(so + (r0 + r) * cols + c0 + c)[inside]]
        bound = rows if mut == "padding_unwritten" else ld
        w = (c0 + c < cols) & (r0 + r < bound)                       # [r, c]
        val = np.where(r0 + r < rows, cvt(t), 0).astype(np.uint16)
        dst[(do + (c0 + c) * ld + r0 + r)[w]] = val[w]
    return dst


# ------------------------------------------------------------------------------------------------ counter RNG
def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & U32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & U32
    x ^= x >> np.uint64(16)
    return x


def pair_mix(x):
    x = np.asarray(x, dtype=np.uint64) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x2C1B3C6D)) & U32
    x ^= x >> np.uint64(16)
    return x


def pair_bits(stream, j):
    return pair_mix((np.asarray(j, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(stream)) & U32)


def keep16(v16, thr16):
    """The documented keep rule stated unsigned: keep iff (v ^ 0x8000) >= thr16 (drop probability thr16 / 65536)."""
    return (np.asarray(v16, dtype=np.int64) ^ 0x8000) >= np.int64(thr16)


def keep16_port(v16, thr16, mut=None):
    """mmb_keep16 as written: the halves read as SIGNED int16 against thr16 - 32768."""
    a = np.asarray(v16, dtype=np.uint16).view(np.int16).astype(np.int64)
    t = np.int64(np.array([(thr16 - 32768) & 0xFFFF], dtype=np.uint16).view(np.int16)[0])
    return a > t if mut == "keep_gt" else a >= t


def keep(stream, idx, thr16, port=False, mut=None):
    idx = np.asarray(idx, dtype=np.uint64)
    h = pair_bits(stream, idx >> np.uint64(1))
    hi = (idx & np.uint64(1)) == 1
    if mut == "halves_swapped":
        hi = ~hi
    v = np.where(hi, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return keep16_port(v, thr16, mut) if port else keep16(v, thr16)


def rng_stream(seed, site):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a = int(hash32((seed & U32) ^ 0xA511E9B3))
    b = int(hash32(((seed >> 32) + 0x7F4A7C15) & U32))
    c = int(hash32((site * 0x85EBCA6B + 0x27D4EB2F) & U32))
    return int(hash32(a ^ ((b * 0x9E3779B1) & U32) ^ c))


def dropout_thr16(p):
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    return int(min(p * 65536.0 + 0.5, 65535.0))


def dropout_mask_ref(n, stream, thr16):
    return keep(stream, np.arange(n, dtype=np.uint64), thr16).astype(np.uint8)


def dropout_mask_port(n, stream, thr16, mut=None):
    """dropout_mask_kernel: grid min(ceil(n / 256), 4096) x 256, grid-stride."""
    out = np.full(n, 0xEE, dtype=np.uint8)
    step = min(max((n + 255) // 256, 1), 4096) * 256
    i = np.arange(min(step, n), dtype=np.uint64)
    while i.size:
        out[i.astype(np.int64)] = keep(stream, i, thr16, port=True, mut=mut)
        if mut == "dropout_one_pass":
            break
        i = i + np.uint64(step)
        i = i[i < np.uint64(n)]
    return out


def attn_dropout_mask_ref(S, elem_base, head, stream, thr16):
    spad = (S + 3) // 4 * 4
    i = np.arange(S, dtype=np.uint64)[:, None]
    j = np.arange(S, dtype=np.uint64)[None, :]
    return keep(stream, np.uint64(elem_base) + (np.uint64(head * S) + i) * np.uint64(spad) + j, thr16).astype(np.uint8)


def mlm_ref(ids, stream, sel_thr16, rep_thr16, specials, mask_id):
    ids = np.asarray(ids, dtype=np.int64)
    h = pair_bits(stream, np.arange(ids.size, dtype=np.uint64))
    special = np.isin(ids, np.asarray(specials, dtype=np.int64))
    sel = ~special & ((h & np.uint64(0xFFFF)).astype(np.int64) < sel_thr16)
    rep = sel & ((h >> np.uint64(16)).astype(np.int64) < rep_thr16)
    return np.where(rep, np.int64(mask_id), ids), np.where(sel, ids, np.int64(-100))


def mlm_port(ids, stream, sel_thr16, rep_thr16, specials, mask_id, mut=None):
    """mlm_mask_kernel: grid min(ceil(n / 256), 1024) x 256, grid-stride; specials = the three ids the kernel gets."""
    ids = np.asarray(ids, dtype=np.int64)
    n = ids.size
    new, lab = ids.copy(), np.full(n, -77, dtype=np.int64)
    step = min(max((n + 255) // 256, 1), 1024) * 256
    s0, s1, s2 = specials
    i = np.arange(min(step, n), dtype=np.int64)
    while i.size:
        h = pair_bits(stream, i.astype(np.uint64))
        lo, hi = (h & np.uint64(0xFFFF)).astype(np.int64), (h >> np.uint64(16)).astype(np.int64)
        if mut == "mlm_halves_swapped":
            lo, hi = hi, lo
        idv = ids[i]
        special = (idv == s0) | (idv == s1) | ((idv == s2) if mut != "third_special_ignored" else False)
        sel = ~special & (lo < sel_thr16)
        lab[i] = np.where(sel, idv, -100)
        new[i] = np.where(sel & (hi < rep_thr16), mask_id, idv)
        if mut == "mlm_one_pass":
            break
        i = i + step
        i = i[i < n]
    return new, lab


def mlm_specials(special_ids):
    """The three ids ops.mlm_mask hands the kernel for 0..3 special ids."""
    sp = list(special_ids)
    return sp + [sp[0] if sp else -1] * (3 - len(sp))


MLM_N = 600_001                # past the 1024 x 256 grid cap (262 144)
DROPOUT_N = 2 * 4096 * 256 + 7  # past the 4096 x 256 grid cap


def mlm_ids(n, seed=0, V=30522):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, V, size=n).astype(np.int64)
    for sid in (101, 102, 0, 103):
        ids[rng.integers(0, n, size=max(n // 50, 1))] = sid
    return ids


# ------------------------------------------------------------------------------------------------ shared inputs
SPECIAL_F32 = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,          # +-0, +-inf, +-FLT_MAX (rounds to inf)
    0x3F808000, 0x3F818000, 0x3F80C000, 0x3F807FFF, 0xBF808000, 0xBF818000,          # RNE ties to even (down / up), round up / down
    0x7F7F7FFF, 0x7F7F8000, 0x00000001, 0x80000001, 0x00008000, 0x00018000,          # near overflow; subnormals and their ties
    0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00017FFF, 0x0000FFFF, 0x00007FFF,
    0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF800001, 0x7FC12345, 0x7FFFFFFF, 0xFFFFFFFF,   # quiet / signalling NaNs
], dtype=np.uint32)
SPECIAL_BF16 = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0x0001, 0x8001, 0x007F, 0x0040, 0x7FC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFFF,
                         0x3F80, 0xC2F7], dtype=np.uint16)
SENTINEL_BF16 = 0x7FA5      # a signalling-NaN bf16 pattern no kernel output takes


def cast_bits(n=4096, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    x[:SPECIAL_F32.size] = SPECIAL_F32
    ties = (rng.standard_normal(256).astype(np.float32).view(np.uint32) & 0xFFFF0000) | 0x8000
    x[SPECIAL_F32.size:SPECIAL_F32.size + 256] = ties
    return x


def seq_ranks(lens, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(n) for n in lens]).astype(np.int64)


def scatter_case():
    """A stamped table over 3000 rows: the current list (stamp 0xFFFFFFF0 - 1 ... past the wrap), an earlier list's entries, and
    entries that carry the current stamp with an index >= nlist; scatter asks for 2800 rows."""
    rng = np.random.default_rng(4)
    table = np.zeros(3000, dtype=np.int64)
    old = rng.permutation(3000)[:600]
    table = stamp_table_ref(table, old, 0xFFFFFFF0)
    stamp = next_stamp(0xFFFFFFF0)
    cur = rng.permutation(3000)[:200]
    table = stamp_table_ref(table, cur, stamp)
    hi = rng.permutation(np.setdiff1d(np.arange(2800), cur))[:9]
    table[hi] = np.array([(stamp << 32) | (200 + k) for k in range(9)], dtype=np.uint64).view(np.int64)
    return table, stamp, 200, 2800


def pack_case(seed=0):
    rng = np.random.default_rng(seed)
    sizes = [70001, 0, 5, 65536, 65537, 1, 300, 0, 257, 1000, 12, 3]
    segs = []
    for k, n in enumerate(sizes):
        if k in (1, 4, 9):
            segs.append((n, int(rng.integers(-5, 30000))))
        else:
            segs.append(rng.integers(-2 ** 62, 2 ** 62, size=n, dtype=np.int64))
    return segs


def _edge_mats():
    mats, so, do = [], 0, 0
    shapes = [(1, 1), (63, 64), (64, 64), (65, 63), (100, 129), (129, 100), (64, 128), (128, 192), (63, 1), (1, 65)]
    for j, (r, c) in enumerate(shapes):
        for ld in sorted({r, r + 5, (r + 63) // 64 * 64 + 16}):
            for mis in (0, 1):
                s_, d_ = so + (1 if mis and j % 2 else 0), do + (3 if mis and j % 2 == 0 else 0)
                mats.append((s_, d_, r, c, ld))
                so = s_ + r * c + 4
                do = d_ + c * ld + 24
    return mats, so, do


def _many_mats(seed=3):
    rng = np.random.default_rng(seed)
    mats, so, do = [], 0, 0
    for j in range(100):
        r, c = (0, 0) if j in (17, 18, 60) else (int(rng.integers(1, 140)), int(rng.integers(1, 140)))
        if j % 3 == 0 and r:
            r, c = (r + 63) // 64 * 64, (c + 63) // 64 * 64             # aligned: the full path
        ld = r + (8 if j % 4 == 1 else 0)
        so, do = (so + 3) // 4 * 4, (do + 7) // 8 * 8
        mats.append((so, do, r, c, max(ld, 0)))
        so += r * c + 4
        do += c * max(ld, 0) + 16
    return mats, so, do


TRANSPOSE_CASES = {"edge": _edge_mats, "many": _many_mats}


def transpose_case(which, bf16src=False, seed=0):
    """(descriptors, total tiles, source bits, sentinel-filled destination bits) of a synthetic descriptor set."""
    mats, nsrc, ndst = TRANSPOSE_CASES[which]()
    descs, ntiles = build_descs(mats)
    rng = np.random.default_rng(seed)
    if bf16src:
        src = bf16_rne(rng.standard_normal(nsrc).astype(np.float32).view(np.uint32))
        src[rng.integers(0, nsrc, size=min(nsrc, 3000))] = np.resize(SPECIAL_BF16, min(nsrc, 3000))
    else:
        src = rng.standard_normal(nsrc).astype(np.float32).view(np.uint32).copy()
        src[rng.integers(0, nsrc, size=min(nsrc, 3000))] = np.resize(SPECIAL_F32, min(nsrc, 3000))
    dst = np.full(ndst + 64, SENTINEL_BF16, dtype=np.uint16)
    return descs, ntiles, src, dst
