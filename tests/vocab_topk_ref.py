"""A float64 reference for the vocabulary top-k kernel (mmbert_vocab_topk, csrc/rowwise.hip) and the check of its outputs.

Not a test module (pytest does not collect it): ``from tests import vocab_topk_ref as T``.

``reference(X, V, k, labels)`` is the definition, in plain float64 torch on the CPU, on the bf16 values the kernel loads (fp32 logits
enter rounded to bf16, as the kernel rounds them):

    order        a STABLE sort of columns 0 .. V-1 by descending value: larger value first, on equal values the lower column first
                 (-0 == +0; pad columns V .. ldv-1 take no part)
    top_ids      the first k columns of that order (exact)
    row_lse      logsumexp over columns 0 .. V-1 (float64)
    top_logprob  x[top_ids] - row_lse
    label_*      for 0 <= label < V: label_logprob = x[label] - row_lse,
                 label_rank = #{c < V : x_c > x_label} + #{c < label : x_c == x_label} (exact);
                 any other label: label_logprob = 0, label_rank = -1 (both exact)

The accuracy model of ``row_lse`` is the one tests/rowwise_ref.py states for mmbert_ce_fwd's row_lse -- acc = 2 |lse| + 12 +
4 sum_c p_c |x_c - max| in fp32 units; it is IMPORTED (``R.ce_fwd``'s ``row_lse`` Ref, evaluated with every row labelled), not copied.
A log-probability is one fp32 subtraction behind the lse: acc = acc_lse + |x - lse|.  -inf log-probabilities (a -inf logit) must be
-inf exactly.  ``check`` asserts ids and ranks equal and the fp32 outputs within ``R.ratios`` <= 1: elementwise for all three,
normwise too for the two vectors (row_lse, label_logprob: one independent error per row); a row of top_logprob is 1 .. 8 entries behind
the SAME lse, one error repeated, which the normwise criterion's averaging does not describe.  (For a group of ONE element the normwise
bound of R.ratios is (0.8 + 2) u |v| + 0.25 * 2^-24 acc against the elementwise 2 u |v| + 2^-24 acc: where acc dominates, a quarter of
it.  The MI355X at V = ldv = 8, M = 300, k = 1 -- [300, 1] rows of one entry -- has its worst entry at 0.326 of the elementwise bound,
which that formula turns into a "normwise" 1.30; the emulation's correctly rounded exp2 / log2 stay below it at 0.31.  The elementwise
bound is the model the lse itself is held to.)

``emulate(...)`` follows the kernel: the lse through ``R._lse_emu`` (ce_row_kernel's rounding and summation order), the order as the
kernel forms it -- one unsigned word per column, monotone key of the bf16 bits in the high half and 0xFFFF - column in the low half,
round j = the largest word strictly below round j - 1's winner --, log-probabilities as one fp32 subtraction.  It exists to show on
the CPU that the check accepts the kernel's arithmetic and rejects the ``MUTATIONS`` (each a one-line change of the emulation).
"""
from __future__ import annotations

import math

import torch

from tests import rowwise_ref as R
from tests.rowwise_ref import _f32

IGNORE = -100
K_MAX = 8
FAMILIES = ("gaussian", "four", "equal", "maxlast", "neginf")
LABEL_KINDS = ("col0", "last", "tied", "ignore", "vocab")


def as_loaded(X):
    """The rows as float64 after the kernel's load (fp32 rounded to bf16)."""
    return X.to(torch.bfloat16).to(torch.float64)


# ------------------------------------------------------------------------------------------------ the reference
def reference(X, V, k, labels=None):
    """X [M, ldv] CPU (bf16 or fp32), labels int64 [M] or None.  Returns a dict: ``top_ids`` int64 [M, k], ``top_logprob`` / ``row_lse``
    (R.Ref), and with labels ``label_logprob`` (R.Ref, exact 0 on rows without a vocabulary label) and ``label_rank`` int64 [M]."""
    M = X.shape[0]
    Xv = as_loaded(X)[:, :V]
    order = torch.sort(-Xv, dim=1, stable=True).indices            # descending value; equal values keep their column order
    ids = order[:, :k]
    # R.ce_fwd with every row "labelled": the float64 lse and its accuracy model.  A -inf logit enters as the most negative finite
    # bf16 value: the same lse and the same model in float64 (its probability is exactly 0), without the model's 0 * inf.
    Xs = torch.where(torch.isinf(X) & (X < 0), torch.full_like(X, -3.0e38), X)
    lse_ref = R.ce_fwd(Xs, torch.zeros(M, dtype=torch.long), V, torch.tensor([0, M]), 1, chunk=128)["row_lse"]
    lse, acc = lse_ref.val, lse_ref.acc
    out = {"top_ids": ids, "row_lse": R.Ref(lse, acc, 0.0, R.U_F32)}
    xt = Xv.gather(1, ids)
    lp = xt - lse[:, None]
    out["top_logprob"] = R.Ref(lp, acc[:, None] + lp.abs(), 0.0, R.U_F32)
    if labels is not None:
        ok = (labels >= 0) & (labels < V)
        lc = torch.where(ok, labels, torch.zeros_like(labels))
        xl = Xv.gather(1, lc[:, None])
        col = torch.arange(V)[None, :]
        rank = (Xv > xl).sum(1) + ((Xv == xl) & (col < lc[:, None])).sum(1)
        out["label_rank"] = torch.where(ok, rank, torch.full_like(rank, -1))
        llp = torch.where(ok, xl[:, 0] - lse, torch.zeros_like(lse))
        exact = torch.where(ok, torch.full_like(lse, float("nan")), torch.zeros_like(lse))
        out["label_logprob"] = R.Ref(llp, torch.where(ok, acc + llp.abs(), torch.zeros_like(acc)), 0.0, R.U_F32, None, exact)
    return out


def _ratios_inf(got, ref):
    """R.ratios, with the reference's infinite entries required bit for bit (and taken out of the norms)."""
    g = got.detach().to(torch.float64).cpu().reshape(ref.val.shape)
    inf = torch.isinf(ref.val)
    bad = int((g[inf] != ref.val[inf]).sum())
    z = torch.zeros_like(ref.val)
    r = R.ratios(torch.where(inf, z, g), R.Ref(torch.where(inf, z, ref.val), torch.where(inf, z, ref.acc), ref.extra, ref.u_out, None, ref.exact),
                 gathered=True)
    r.exact_bad += bad
    return r


def check(got, ref, what=""):
    """got: dict of the kernel's outputs (any device; ``top_ids`` / ``label_rank`` any integer dtype).  Asserts ids and ranks equal to
    the reference and lse / log-probabilities within the model; returns {name: R.Ratios} of the fp32 outputs."""
    ids = got["top_ids"].cpu().long()
    assert ids.shape == ref["top_ids"].shape, f"{what}: top_ids shape {tuple(ids.shape)}"
    nbad = int((ids != ref["top_ids"]).sum())
    assert nbad == 0, f"{what}: {nbad} top_ids differ from the stable-sort order, first at {torch.nonzero(ids != ref['top_ids'])[0].tolist()}"
    out = {}
    names = ["row_lse", "top_logprob"]
    if "label_rank" in ref:
        rk = got["label_rank"].cpu().long()
        nbad = int((rk != ref["label_rank"]).sum())
        assert nbad == 0, f"{what}: {nbad} label ranks differ, first at row {int(torch.nonzero(rk != ref['label_rank'])[0])}"
        names.append("label_logprob")
    for n in names:
        r = _ratios_inf(got[n], ref[n])
        assert r.exact_bad == 0, f"{what}: {n}: {r.exact_bad} elements differ from their exact value"
        # top_logprob: the k entries of a row share ONE lse, so their errors are one error, not k independent ones -- the normwise
        # (averaging) criterion of R.ratios has nothing to average over a row of 1 .. 8 such entries; the elementwise bound holds them
        norm = 0.0 if n == "top_logprob" else r.norm
        assert r.elem <= 1.0 and norm <= 1.0, f"{what}: {n}: elementwise ratio {r.elem:.3g} (worst at {r.where}), normwise {norm:.3g}"
        r.norm = norm
        out[n] = r
    return out


# ------------------------------------------------------------------------------------------------ the emulation
MUTATIONS = ("tie_to_higher_column", "pad_in_topk", "pad_in_lse", "rank_ge", "round_le", "round_value_only", "label_and_7")


def _keys(X, ncols):
    """Monotone 16-bit key of every column's bf16 bits (int64 [M, ldv]); columns at or past ``ncols``: 0 (below every value)."""
    bits = X.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    bits = torch.where(bits == 0x8000, torch.zeros_like(bits), bits)                 # -0 reads as +0
    key = torch.where(bits >= 0x8000, bits ^ 0xFFFF, bits | 0x8000)
    col = torch.arange(X.shape[1])[None, :]
    return torch.where(col < ncols, key, torch.zeros_like(key))


def emulate(X, V, k, labels=None, mutation=None):
    """The kernel's arithmetic on the CPU (see the module docstring); ``mutation``: one of MUTATIONS.  Returns the outputs as the
    kernel would write them (float64 holding fp32 values, int64 ids / ranks)."""
    assert mutation is None or mutation in MUTATIONS
    M, ldv = X.shape
    Xb = as_loaded(X)
    lse = R._lse_emu(Xb, V, ldv if mutation == "pad_in_lse" else V)
    key = _keys(X, ldv if mutation == "pad_in_topk" else V)
    col = torch.arange(ldv)[None, :].expand(M, ldv)
    low = col if mutation == "tie_to_higher_column" else 0xFFFF - col
    word = (key << 16) | low
    prev = torch.full((M,), 0xFFFFFFFF, dtype=torch.int64)
    ids, lps = [], []
    for _ in range(k):
        if mutation == "round_le":
            ok = word <= prev[:, None]
        elif mutation == "round_value_only":
            ok = (word >> 16) < (prev[:, None] >> 16)
        else:
            ok = word < prev[:, None]
        win = torch.where(ok, word, torch.zeros_like(word)).max(1)
        prev = win.values
        c = win.indices
        ids.append(c)
        lps.append(_f32(Xb.gather(1, c[:, None])[:, 0] - lse))
    out = {"top_ids": torch.stack(ids, 1), "top_logprob": torch.stack(lps, 1), "row_lse": lse}
    if labels is not None:
        ok = (labels >= 0) & (labels < V)
        lc = torch.where(ok, labels, torch.zeros_like(labels))
        if mutation == "label_and_7":
            bad = ~ok & (labels >= 0)
            lc = torch.where(bad, labels & 7, lc)
            ok = ok | bad
        lw = word.gather(1, lc[:, None])
        above = ((word >= lw) if mutation == "rank_ge" else (word > lw)).sum(1)
        out["label_rank"] = torch.where(ok, above, torch.full_like(above, -1))
        out["label_logprob"] = torch.where(ok, _f32(Xb.gather(1, lc[:, None])[:, 0] - lse), torch.zeros_like(lse))
    return out


# ------------------------------------------------------------------------------------------------ test inputs
def make_case(V, ldv, M, seed, dtype=torch.bfloat16):
    """(X [M, ldv] CPU bf16-representable values in ``dtype``, labels int64 [M], family index [M], label kind index [M]).  Row i is of
    family FAMILIES[(i + seed) % 5] and carries a label of kind LABEL_KINDS[(i // 5 + i + seed) % 5]:
      gaussian  3 N(0, 1);   four  drawn from four distinct bf16 values (ties dominate);   equal  one value in every column;
      maxlast   the row maximum at column V - 1, larger values in the pad columns;   neginf  a third of the columns -inf (one finite)
      col0 / last  label 0 / V - 1;  tied  a column whose value an EARLIER column shares (planted);  ignore  -100;  vocab  V (out of range).
    Pad columns V .. ldv-1 hold values above the row's maximum in every family."""
    g = torch.Generator().manual_seed(1000 * seed + V + M)
    X = (3.0 * torch.randn(M, ldv, generator=g)).to(torch.bfloat16)
    fam = (torch.arange(M) + seed) % 5
    kind = (torch.arange(M) // 5 + torch.arange(M) + seed) % 5
    four = torch.tensor([-2.0, 0.5, 1.0, 3.0], dtype=torch.bfloat16)
    labels = torch.empty(M, dtype=torch.long)
    for i in range(M):
        f = int(fam[i])
        if f == 1:
            X[i] = four[torch.randint(0, 4, (ldv,), generator=g)]
        elif f == 2:
            X[i] = 0.75
        elif f == 3:
            X[i, V - 1] = 20.0
        elif f == 4:
            X[i, torch.rand(ldv, generator=g) < 0.33] = -math.inf
            X[i, i % V] = 1.0
        X[i, V:] = 60.0 if f == 3 else 30.0
        kd = int(kind[i])
        if kd == 0:
            labels[i] = 0
        elif kd == 1:
            labels[i] = V - 1
        elif kd == 2:
            b = int(torch.randint(1, V - 1 if f == 3 else V, (1,), generator=g))      # (maxlast: column V - 1 keeps the maximum)
            a = int(torch.randint(0, b, (1,), generator=g))
            X[i, b] = X[i, a]
            labels[i] = b
        elif kd == 3:
            labels[i] = IGNORE
        else:
            labels[i] = V
    return X.to(dtype), labels, fam, kind
