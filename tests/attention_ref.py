"""A float64 reference for the attention kernels (csrc/attention.hip) and a scale-aware check of their outputs.

Not a test module (pytest does not collect it): ``from tests.attention_ref import reference, emulate, check, ...``.

``reference`` is plain float64 torch on the CPU, per sequence and head, on the same bf16 inputs the kernels get:

    scores = q.k^T / 8 + key_bias        P = softmax(scores)        ctx = (P * keep * drop_scale) . V
    lse    = logsumexp(scores)           (natural log)
    dV = Pd^T.dO     dP = (dO.V^T) * keep * drop_scale     dS = P * (dP - delta),  delta = rowsum(dO * ctx)
    dQ = dS.K / 8    dK = dS^T.Q / 8

with the reference model's additive key bias ``(1 - mask) * -10000`` (exp(-10000) is an exact 0 in float64 as well).  The
backward is written out instead of taken from autograd: the mutations below need to reach inside it, and it keeps the memory
of the headline shape in bounds (sequences of one length are batched in chunks).  It always works on the UNPACKED sequences in
their original row order; outputs of a packed layout are compared after mapping them back (``unpack``).

``emulate`` is the same computation with the roundings the kernels document -- scores accumulated in fp32 on top of the bias
in two 32-term MFMA steps, bf16 P before P.V with the denominator summed from those rounded P, the LSE assembled in fp32,
delta from the bf16 context, the backward's P recomputed from that LSE, bf16 dS and dropped P in front of the dQ / dK / dV
products, bf16 outputs.  It exists only to calibrate the bounds of ``check`` on the CPU.

``check`` splits every output into blocks of (sequence, head) -- ctx columns h*64.., the dQ / dK / dV columns of head h, LSE
column h -- and asserts per block

    normwise     ||got - ref||_F <= TAU[kind] * ||ref||_F
    elementwise  |got - ref|     <= KAPPA[kind] * max|ref_block|
    LSE          |got - ref|     <= LSE_ABS + LSE_RHO * rho + LSE_ULPS * 2^-24 * |ref|     (per row, see below)

A block whose reference is exactly zero must come out exactly zero.

Calibration (tests/test_attention_reference_cpu.py, ``CALIBRATION_CASES``): ``emulate`` against ``reference`` over heads
1, 3, 12, 16 on the packed edge lengths 1 ... 257 with every key-bias pattern, S = 550 / 1050, and a forced-rescale case
(score std ~ 8, keys spiked against chosen queries), p in {0, 0.1}.  Largest ratios the emulation reached, and the bounds set
at about twice those:

    kind   normwise err/||ref||  -> TAU      elementwise err/max|ref|  -> KAPPA
    ctx    2.4e-3                   5e-3     4.5e-3                       1e-2
    dq     1.9e-3                   4e-3     4.7e-3                       1e-2
    dk     1.9e-3                   4e-3     4.9e-3                       1.25e-2
    dv     3.9e-3                   8e-3     6.3e-3                       1.25e-2

(the largest ones at the short and the fully masked sequences).  Two refinements the emulation forced:

* LSE.  The denominator summed from bf16 P moves the LSE of a row by about 2^-9 * rho, rho = sqrt(sum of P^2 over all but the
  largest key) -- measured 1.5e-3 at S = 3; at S = 550 (rho ~ 0.07) it is of the order of 1e-4.  One absolute bound of 1e-4 would reject a correct kernel on short rows,
  one of 2e-3 would miss a lost key on long ones, so the bound is per row: LSE_ABS + LSE_RHO * rho + LSE_ULPS * 2^-24 * |LSE|
  (the last term: fp32 rounding of scores and LSE around -10000 in a fully masked sequence).  Emulation: (err - LSE_ABS -
  LSE_ULPS ulps) / rho <= 7.0e-3 -> LSE_RHO = 1.4e-2.
* dQ / dK.  When a row's P is (nearly) one-hot, dP - delta cancels and the exact dQ / dK are ~0: the kernel's are rounding noise
  of the cancelled terms (S = 1: 7 % of the exact value).  Their norms are therefore taken as at least those of the rounding
  scale ``dq_mag`` / ``dk_mag`` = sqrt((P * (|dP| + sum|dO * O|))^2 . K^2) / 8 (resp. with Q), which the reference returns; on
  rows without cancellation it is about the size of the exact result.

The smallest margin of a mutation is recorded in the CPU test's docstring.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

SCALE = 0.125                     # 1/sqrt(64)
MASKED = -10000.0                 # the reference's additive bias of a masked key

TAU = {"ctx": 5e-3, "dq": 4e-3, "dk": 4e-3, "dv": 8e-3}
KAPPA = {"ctx": 1e-2, "dq": 1e-2, "dk": 1.25e-2, "dv": 1.25e-2}
LSE_ABS = 1e-6
LSE_RHO = 1.4e-2
LSE_ULPS = 16.0

KINDS = ("ctx", "lse", "dq", "dk", "dv")

_LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
_LN2_32 = float(torch.tensor(0.6931471805599453, dtype=torch.float32))


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _f32(x):
    return x.to(torch.float32).to(x.dtype)


# ------------------------------------------------------------------------------------------------ mutations
@dataclass
class Mutation:
    """A subtle perturbation of the reference.  ``blocks``: the (sequence, head) blocks it changes (None: every block)."""
    name: str
    blocks: set | None
    scale: float = 1.0                                     # softmax scale multiplier
    bias: dict = field(default_factory=dict)               # (seq, head) -> callable(bias [S]) -> bias [S]
    keep_from_head: dict = field(default_factory=dict)     # (seq, head) -> head whose dropout mask it uses
    delta_zero: dict = field(default_factory=dict)         # (seq, head) -> first row of a 16-row block whose delta is left out
    dv_unscaled: set = field(default_factory=set)          # (seq, head): dV without the dropout scale


def drop_key(seq, head, key):
    """One unmasked key of one (sequence, head) left out of the softmax and of P.V."""
    def f(b):
        assert float(b[key]) > MASKED, "drop_key needs an unmasked key"
        b = b.clone()
        b[key] = -math.inf
        return b
    return Mutation(f"drop key {key} of seq {seq} head {head}", {(seq, head)}, bias={(seq, head): f})


def move_mask(seq, key, heads):
    """The -10000 of masked key ``key`` moved to its neighbour ``key + 1`` (every head)."""
    def f(b):
        assert float(b[key]) <= MASKED and float(b[key + 1]) > MASKED, "move_mask needs a masked key followed by an unmasked one"
        b = b.clone()
        b[key], b[key + 1] = b[key + 1].clone(), b[key].clone()
        return b
    return Mutation(f"mask of key {key} of seq {seq} moved to key {key + 1}", {(seq, h) for h in range(heads)},
                    bias={(seq, h): f for h in range(heads)})


def neighbour_dropout(seq, head, heads):
    """One head of one sequence uses the dropout mask of the neighbouring head."""
    other = head ^ 1 if (head ^ 1) < heads else head - 1
    return Mutation(f"seq {seq} head {head} uses the dropout mask of head {other}", {(seq, head)}, keep_from_head={(seq, head): other})


def softmax_scale(factor=1.0 + 2.0 ** -5):
    return Mutation(f"softmax scale x {factor}", None, scale=factor)


def drop_delta(seq, head, row0):
    """The delta = rowsum(dO * O) term left out for the 16 query rows row0 ... row0 + 15 of one (sequence, head)."""
    return Mutation(f"delta left out for rows {row0}..{row0 + 15} of seq {seq} head {head}", {(seq, head)}, delta_zero={(seq, head): row0})


def dv_without_dropout_scale(seq, head):
    return Mutation(f"dV of seq {seq} head {head} without the dropout scale", {(seq, head)}, dv_unscaled={(seq, head)})


# ------------------------------------------------------------------------------------------------ reference
def _starts(lens):
    out, s = [], 0
    for n in lens:
        out.append(s)
        s += n
    return out


def _core(q, k, v, bias, keep, dscale, do, emu, scale, hooks):
    """q, k, v, do [n, h, S, 64]; bias [n, h, S]; keep [n, h, S, S] (0 / 1) or None -- all float64."""
    qk = q @ k.transpose(-1, -2)
    if emu:
        # the kernels' score: bias as the initial fp32 accumulator, + q.k/8 in two 32-term MFMA steps, one fp32 rounding each
        # (forward and dQ kernels; Q carries the 1/8, exact in bf16)
        lo = (q[..., :32] @ k[..., :32].transpose(-1, -2)) * scale
        s = _f32(_f32(bias[..., None, :] + lo) + (qk * scale - lo))
    else:
        s = qk * scale + bias[..., None, :]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    if emu:
        e = _bf(e)                                         # P packed to bf16 before P.V; the denominator sums those
    l = e.sum(-1, keepdim=True)
    if emu:
        lse = _f32(_f32(_f32(_f32(m) * _LOG2E32) + _f32(torch.log2(_f32(l)))) * _LN2_32)[..., 0]
    else:
        lse = (m + torch.log(l))[..., 0]
    kd = keep * dscale if keep is not None else None
    o = ((e * kd) if kd is not None else e) @ v / l
    if emu:
        o = _bf(o)
    # LSE rounding scale of a row: the bf16 rounding of P adds sqrt(sum P^2) * 2^-9 / sqrt(3) to the log of the denominator on
    # average (the maximal term, exp(0) = 1, is exact)
    pr = e / l
    rho = (pr.pow(2).sum(-1) - pr.amax(-1).pow(2)).clamp_min(0.0).sqrt()
    if do is None:
        return o, lse, None, None, None, rho, (None, None)
    if emu:
        p = torch.exp(s - lse[..., None])                  # dQ kernel: P recomputed from the stored LSE
        # dK/dV kernel: accumulator starts at (bias - lse)/scale, + q.k (unscaled) in two steps, then exp2(s * scale * log2e)
        acc = _f32(_f32(bias[..., None, :] / scale) + _f32(-lse[..., None] / scale))
        qlo = q[..., :32] @ k[..., :32].transpose(-1, -2)
        acc = _f32(_f32(acc + qlo) + (qk - qlo))
        p_kv = torch.exp(acc * scale)
    else:
        p = e / l
        p_kv = p
    delta = (do * o).sum(-1, keepdim=True)                 # emulation: from the bf16 context, as the dQ kernel reads it
    for (i, h), r0 in hooks.get("delta_zero", ()):
        delta[i, h, r0:r0 + 16] = 0.0
    dp = do @ v.transpose(-1, -2)
    if kd is not None:
        dp = dp * kd
    ds = p * (dp - delta)
    ds_kv = p_kv * (dp - delta) if emu else ds
    if not emu:
        # rounding scale of dQ / dK: what the sums would be without the cancellation between dP and delta (a row whose P is
        # one-hot has dS ~ 0, and its dQ is rounding noise of that size; see check)
        w = (p * (dp.abs() + (do * o).abs().sum(-1, keepdim=True))).pow(2)
        mags = ((w @ k.pow(2)).sqrt() * scale, (w.transpose(-1, -2) @ q.pow(2)).sqrt() * scale)
    pd = p_kv * kd if kd is not None else p_kv
    if emu:
        ds, ds_kv, pd = _bf(ds), _bf(ds_kv), _bf(pd)
    dq = ds @ k * scale
    dk = ds_kv.transpose(-1, -2) @ q * scale
    dv = pd.transpose(-1, -2) @ do
    for i, h in hooks.get("dv_unscaled", ()):
        dv[i, h] = dv[i, h] / dscale
    if emu:
        dq, dk, dv = _bf(dq), _bf(dk), _bf(dv)
        mags = (None, None)
    return o, lse, dq, dk, dv, rho, mags


def reference(qkv_bf16, key_bias, lens, heads, drop_masks=None, drop_scale=1.0, dctx=None, *, mutation: Mutation | None = None,
              _emulate=False, chunk_elems=1 << 24):
    """float64 outputs in the original row order: dict ctx [M, H], lse [M, heads] and, with ``dctx``, dq / dk / dv [M, H].

    ``qkv_bf16`` [M, 3H] (q | k | v, head h at columns h*64), ``key_bias`` [M] additive (0 or -10000), ``lens`` the sequence
    lengths back to back, ``drop_masks`` per sequence a [heads, S, S] keep mask (0 / 1) or None, ``dctx`` [M, H] or None."""
    mut = mutation or Mutation("none", set())
    M = qkv_bf16.shape[0]
    H = heads * 64
    assert qkv_bf16.shape[1] == 3 * H and sum(lens) == M
    x = qkv_bf16.detach().cpu().to(torch.bfloat16).double()
    kb = key_bias.detach().cpu().double().reshape(-1)
    do_all = dctx.detach().cpu().to(torch.bfloat16).double() if dctx is not None else None
    starts = _starts(lens)
    out = {"ctx": torch.zeros(M, H, dtype=torch.float64), "lse": torch.zeros(M, heads, dtype=torch.float64),
           "lse_rho": torch.zeros(M, heads, dtype=torch.float64)}
    if dctx is not None:
        for kname in ("dq", "dk", "dv", "dq_mag", "dk_mag"):
            out[kname] = torch.zeros(M, H, dtype=torch.float64)
    by_len = {}
    for i, n in enumerate(lens):
        if n > 0:
            by_len.setdefault(n, []).append(i)
    for S, seqs in by_len.items():
        per = max(1, chunk_elems // (heads * S * S))
        for c0 in range(0, len(seqs), per):
            ids = seqs[c0:c0 + per]
            rows = torch.cat([torch.arange(starts[i], starts[i] + S) for i in ids])
            xs = x[rows].view(len(ids), S, 3, heads, 64)
            q, k, v = (xs[:, :, j].permute(0, 2, 1, 3) for j in range(3))
            bias = kb[rows].view(len(ids), 1, S).expand(len(ids), heads, S).clone()
            keep = None
            if drop_masks is not None:
                keep = torch.stack([drop_masks[i].to(torch.float64).cpu() for i in ids])
            hooks = {"delta_zero": [], "dv_unscaled": []}
            for j, i in enumerate(ids):
                for h in range(heads):
                    if (i, h) in mut.bias:
                        bias[j, h] = mut.bias[(i, h)](bias[j, h])
                    if (i, h) in mut.keep_from_head:
                        keep[j, h] = torch.as_tensor(drop_masks[i][mut.keep_from_head[(i, h)]], dtype=torch.float64)
                    if (i, h) in mut.delta_zero:
                        hooks["delta_zero"].append(((j, h), mut.delta_zero[(i, h)]))
                    if (i, h) in mut.dv_unscaled:
                        hooks["dv_unscaled"].append((j, h))
            do = do_all[rows].view(len(ids), S, heads, 64).permute(0, 2, 1, 3) if do_all is not None else None
            o, lse, dq, dk, dv, rho, mags = _core(q, k, v, bias, keep, float(drop_scale), do, _emulate, SCALE * mut.scale, hooks)
            back = lambda t: t.permute(0, 2, 1, 3).reshape(len(ids) * S, H)
            out["ctx"][rows] = back(o)
            out["lse"][rows] = lse.permute(0, 2, 1).reshape(len(ids) * S, heads)
            out["lse_rho"][rows] = rho.permute(0, 2, 1).reshape(len(ids) * S, heads)
            if do is not None:
                out["dq"][rows], out["dk"][rows], out["dv"][rows] = back(dq), back(dk), back(dv)
                if mags[0] is not None:
                    out["dq_mag"][rows], out["dk_mag"][rows] = back(mags[0]), back(mags[1])
    return out


def emulate(qkv_bf16, key_bias, lens, heads, drop_masks=None, drop_scale=1.0, dctx=None, *, mutation=None):
    """``reference`` with the kernels' documented roundings (see the module docstring); for calibrating ``check`` only."""
    return reference(qkv_bf16, key_bias, lens, heads, drop_masks, drop_scale, dctx, mutation=mutation, _emulate=True)


# ------------------------------------------------------------------------------------------------ kernel outputs
def unpack(t, layout):
    """A [packed rows, ...] kernel output in the original row order (through ``layout.inv``; identity for ops.SeqLayout)."""
    inv = getattr(layout, "inv", None)
    if inv is None:
        return t
    t2 = t
    if int(inv.max()) >= t.shape[0]:                       # drop mode: left-out rows map one past the packed matrix
        t2 = torch.cat((t, torch.zeros_like(t[:1])))
    return t2[inv.to(t.device)]


def outputs(ctx=None, lse=None, dqkv=None, layout=None):
    """Kernel outputs as a dict of float64 CPU tensors in the original row order (the keys ``check`` reads)."""
    out = {}
    if ctx is not None:
        out["ctx"] = unpack(ctx, layout).double().cpu()
    if lse is not None:
        out["lse"] = unpack(lse, layout).double().cpu()
    if dqkv is not None:
        d = unpack(dqkv, layout).double().cpu()
        H = d.shape[1] // 3
        out["dq"], out["dk"], out["dv"] = d[:, :H], d[:, H:2 * H], d[:, 2 * H:]
    return out


# ------------------------------------------------------------------------------------------------ the check
@dataclass
class Worst:
    ratio: float
    seq: int
    head: int
    kind: str
    row: int            # row index inside the sequence of the largest elementwise error
    test: str           # "norm", "elem" or "lse"


def _lens(layout):
    return list(layout) if isinstance(layout, (list, tuple)) else list(layout.lens)


def ratios(got, ref, layout, heads, rows=None):
    """Per (sequence, head, kind): the largest of the ratios error / bound (<= 1 passes).  ``rows`` (bool [M]): compare those
    rows only.  Returns {(seq, head, kind): Worst}."""
    lens = _lens(layout)
    starts = _starts(lens)
    res = {}
    for kind in KINDS:
        if kind not in got or kind not in ref:
            continue
        g_all, r_all = got[kind].double().cpu(), ref[kind].double().cpu()
        assert g_all.shape == r_all.shape, (kind, g_all.shape, r_all.shape)
        for s, (s0, n) in enumerate(zip(starts, lens)):
            if n == 0:
                continue
            g, r = g_all[s0:s0 + n], r_all[s0:s0 + n]
            if rows is not None:
                sel = rows[s0:s0 + n].cpu()
                if not bool(sel.any()):
                    continue
                g, r = g.clone(), r.clone()
                g[~sel] = 0.0
                r[~sel] = 0.0
            if kind == "lse":
                err = (g - r).abs()                                             # [n, heads]
                rho = ref["lse_rho"][s0:s0 + n].double().cpu()
                bound = LSE_ABS + LSE_RHO * rho + LSE_ULPS * 2.0 ** -24 * r.abs()
                q = torch.where(err == 0, torch.zeros_like(err), err / bound)
                q = torch.nan_to_num(q, nan=math.inf)
                if rows is not None:
                    q[~sel] = 0.0
                val, at = q.max(0)
                for h in range(heads):
                    res[(s, h, kind)] = Worst(float(val[h]), s, h, kind, int(at[h]), "lse")
                continue
            g3, r3 = g.view(n, heads, 64), r.view(n, heads, 64)
            diff = (g3 - r3)
            dn = diff.pow(2).sum((0, 2)).sqrt()
            rn = r3.pow(2).sum((0, 2)).sqrt()
            rmax = r3.abs().amax((0, 2))
            if kind + "_mag" in ref:                                            # dQ / dK: at least their rounding scale
                m3 = ref[kind + "_mag"][s0:s0 + n].double().cpu().view(n, heads, 64)
                if rows is not None:
                    m3 = m3 * sel[:, None, None]
                rn = torch.maximum(rn, m3.pow(2).sum((0, 2)).sqrt())
                rmax = torch.maximum(rmax, m3.amax((0, 2)))
            emax_row, _ = diff.abs().amax(2).max(0)                             # per head: largest error and ...
            erow = diff.abs().amax(2).argmax(0)                                 # ... its row
            for h in range(heads):
                qn = 0.0 if float(dn[h]) == 0 else float(dn[h]) / (TAU[kind] * float(rn[h])) if float(rn[h]) > 0 else math.inf
                qe = 0.0 if float(emax_row[h]) == 0 else float(emax_row[h]) / (KAPPA[kind] * float(rmax[h])) if float(rmax[h]) > 0 else math.inf
                if not (math.isfinite(float(dn[h])) and math.isfinite(float(emax_row[h]))):
                    qn = qe = math.inf
                w = Worst(qn, s, h, kind, int(erow[h]), "norm") if qn >= qe else Worst(qe, s, h, kind, int(erow[h]), "elem")
                res[(s, h, kind)] = w
    return res


def summary(res):
    """The largest ratio per output kind."""
    out = {}
    for (_, _, kind), w in res.items():
        out[kind] = max(out.get(kind, 0.0), w.ratio)
    return out


def check(got, ref, layout, heads, what="", rows=None):
    """Assert every (sequence, head) block of every output in ``got`` within its bound of ``ref`` (see the module docstring).
    ``layout``: the sequence lengths (a list) or an object with ``.lens``.  Returns the largest ratio per output kind."""
    res = ratios(got, ref, layout, heads, rows)
    assert res, f"{what}: nothing compared"
    bad = sorted((w for w in res.values() if not w.ratio <= 1.0), key=lambda w: -w.ratio)
    if bad:
        lines = [f"seq {w.seq} head {w.head} {w.kind}: ratio {w.ratio:.3g} ({w.test}), worst row {w.row}" for w in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {len(res)} blocks out of bound\n  " + "\n  ".join(lines))
    return summary(res)


# ------------------------------------------------------------------------------------------------ test inputs
EDGE_LENS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257]
PATTERNS = ("none", "random", "tail_inside", "tail_boundary", "key0_only", "all_masked")


def bias_pattern(S, pattern, g):
    """[S] additive key bias (0 / -10000) of one sequence.  ``random``: 20 % of the keys masked; ``tail_inside`` / ``tail_boundary``:
    a masked tail whose last unmasked key ends inside a 64-key tile / on a tile boundary (no tail where S leaves no room for one);
    ``key0_only``: every key but key 0 masked; ``all_masked``: every key masked (softmax over equally biased keys)."""
    b = torch.zeros(S, dtype=torch.float64)
    if pattern == "random":
        b[torch.rand(S, generator=g) < 0.2] = MASKED
    elif pattern == "tail_inside":
        kv = max(1, (2 * S) // 3)
        if kv % 64 == 0 and kv > 1:
            kv -= 1
        b[kv:] = MASKED
    elif pattern == "tail_boundary":
        kv = (S - 1) // 64 * 64
        if kv > 0:
            b[kv:] = MASKED
    elif pattern == "key0_only":
        b[1:] = MASKED
    elif pattern == "all_masked":
        b[:] = MASKED
    else:
        assert pattern == "none", pattern
    return b


def random_keep(lens, heads, p, g):
    """CPU stand-in for the kernels' dropout: per sequence a [heads, S, S] Bernoulli(1 - p) keep mask (uint8)."""
    return [(torch.rand(heads, n, n, generator=g) >= p).to(torch.uint8) for n in lens]


def make_inputs(lens, heads, patterns, seed, qk_scale=1.0):
    """qkv [M, 3H] bf16 (q and k scaled by ``qk_scale``: score std ~ qk_scale^2), key bias [M] float32 from ``patterns`` (one per
    sequence), dctx [M, H] bf16."""
    g = torch.Generator().manual_seed(seed)
    M, H = sum(lens), heads * 64
    qkv = torch.randn(M, 3 * H, generator=g)
    qkv[:, :2 * H] *= qk_scale
    bias = torch.cat([bias_pattern(n, pat, g) for n, pat in zip(lens, patterns)]).float()
    dctx = torch.randn(M, H, generator=g)
    return qkv.to(torch.bfloat16), bias, dctx.to(torch.bfloat16)


def spike_rescale(qkv, lens, heads, plan, factor=0.5):
    """Force the running maximum to jump at chosen key tiles (guide rule 26): for (seq, key, query rows) in ``plan`` the key's k
    row of every head is set to ``factor`` x the first listed query's q row, so that those queries' scores peak at that key
    (with q, k scaled to a score std of 8: |q|^2 / 8 ~ 64, the spike ~ 32 against a row maximum of ~ 22 elsewhere).
    Returns qkv (bf16)."""
    x = qkv.float().clone()
    H = heads * 64
    starts = _starts(lens)
    for seq, key, qrows in plan:
        s0 = starts[seq]
        x[s0 + key, H:2 * H] = x[s0 + qrows[0], 0:H] * factor
        for r in qrows[1:]:
            x[s0 + r, 0:H] = x[s0 + qrows[0], 0:H]
    return x.to(torch.bfloat16)
