"""Shared by the CPU and GPU tests of ``attn_probs_first`` (the attention probabilities of one query row per sequence): the case list,
a float64 reference, an fp32 emulation of the kernel's documented arithmetic and the check.  Not a test module (pytest does not
collect it).

``reference_probs``: float64 torch on the CPU, per (sequence, head), on the same bf16 inputs the kernel gets:

    s_k = q . k_k / 8 + key_bias[k]        p = softmax(s)        (q = the row at position ``q_pos`` of the sequence)

It returns the probabilities and the scores, both [sequences, heads, ld], ld = the longest sequence; behind a sequence's length the
probabilities are 0 and the scores -inf.

``emulate_probs``: the kernel (csrc/attention.hip, ``attn_probs_first_kernel``) in fp32 torch, in its summation order: lane c of a key's
8 lanes runs an 8-term fma chain over dims 8c .. 8c + 7 of (q / 8) and k (the products of two bf16 values are exact in fp32, so
multiply-then-add IS the fma), three cross-lane adds (lane ^ 1, ^ 2, ^ 4), + key_bias; group g of the 32 walks the keys g + 32 u + 256 t,
u < 8, one round t at a time with the online maximum m and denominator l (l *= exp2((m - m') log2e), then + exp2((s_u - m') log2e) for
u = 0 .. 7); the groups are merged pairwise over the 8 groups of a wave (^ 1, ^ 2, ^ 4), then the 4 waves in order; p_k =
exp2((s_k - m) log2e) * (1 / l).  What it cannot state: the hardware's exp2 (1 ulp) and whether the compiler contracts l * w + l' * w'.

``check_probs`` asserts per (sequence, head) block, with u = 2^-24 * max(1, max |s_ref| over the keys whose reference probability is
non-zero) -- the fp32 rounding of a score, which is what moves a probability (a fully masked sequence has |s| ~ 10000: one ulp there
is 1e-3, and its probabilities move by 5e-4 between two correct fp32 evaluations):

    L1           sum_k |p_k - p_ref,k|  <=  PHI * u                     (covers "sums to one")
    elementwise  max_k |p_k - p_ref,k|  <=  PHI * u * max_k p_ref,k
    a key whose reference probability is exactly 0 must be exactly 0 (masked keys next to an unmasked one, everything behind the length)
    nothing non-finite

Calibration (tests/test_attention_probs_reference_cpu.py): ``emulate_probs`` against ``reference_probs`` over ``CASES`` reaches at most
1.40 u in the L1 form and 2.02 u max p elementwise (both at the headline set, 576 blocks of up to 550 keys; the edge lengths reach 1.21 /
1.86 at 16 heads, the 1425-key case 0.51 / 1.14); PHI is set to about twice the larger: PHI = 4.
"""
import math

import torch

from tests import attention_first_ref as F
from tests import attention_ref as A

PHI = 4.0
U32 = 2.0 ** -24

LONG_CASE = ("long-h2", [1425, 129, 1], 2, ["tail_inside", "random", "none"], 1.0)
CASES = list(F.CASES) + [LONG_CASE]


def inputs(case):
    return F.inputs(*case)


# ------------------------------------------------------------------------------------------------ float64 reference
def reference_probs(qkv_bf16, key_bias, lens, heads, q_pos=0, *, mutation: "A.Mutation | None" = None, denom_keys=None):
    """(probs, scores), float64 [sequences, heads, max(lens)].  ``mutation``: an ``attention_ref.Mutation`` (its ``scale`` and ``bias``
    hooks: softmax_scale / drop_key / move_mask); ``denom_keys`` = n: the denominator summed over the first n keys only (a lost merge)."""
    mut = mutation or A.Mutation("none", set())
    x = qkv_bf16.detach().cpu().to(torch.bfloat16).double()
    kb = key_bias.detach().cpu().double().reshape(-1)
    ns, ld = len(lens), max(lens)
    probs = torch.zeros(ns, heads, ld, dtype=torch.float64)
    scores = torch.full((ns, heads, ld), -math.inf, dtype=torch.float64)
    for i, (s0, S) in enumerate(zip(A._starts(lens), lens)):
        if S == 0:
            continue
        xs = x[s0:s0 + S].view(S, 3, heads, 64)
        q = xs[min(q_pos, S - 1), 0]                                           # [heads, 64]
        k = xs[:, 1].permute(1, 0, 2)                                          # [heads, S, 64]
        bias = kb[s0:s0 + S][None, :].expand(heads, S).clone()
        for h in range(heads):
            if (i, h) in mut.bias:
                bias[h] = mut.bias[(i, h)](bias[h])
        s = torch.einsum("hd,hkd->hk", q, k) * (A.SCALE * mut.scale) + bias
        e = torch.exp(s - s.amax(-1, keepdim=True))
        den = e.sum(-1, keepdim=True) if denom_keys is None else e[:, :denom_keys].sum(-1, keepdim=True)
        probs[i, :, :S] = e / den
        scores[i, :, :S] = s
    return probs, scores


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernel
_L2E = A._LOG2E32
_NINF = -math.inf


def _merge(ma, la, mb, lb):
    M = torch.maximum(ma, mb)
    wa = torch.where(ma == _NINF, torch.zeros_like(ma), torch.exp2((ma - M) * _L2E))
    wb = torch.where(mb == _NINF, torch.zeros_like(mb), torch.exp2((mb - M) * _L2E))
    return M, la * wa + lb * wb


def emulate_probs(qkv_bf16, key_bias, lens, heads, q_pos=0):
    """fp32 [sequences, heads, max(lens)]: the kernel's arithmetic in its order (see the module docstring)."""
    x = qkv_bf16.detach().cpu().to(torch.bfloat16).float()
    kb = key_bias.detach().cpu().float().reshape(-1)
    ns, ld = len(lens), max(lens)
    out = torch.zeros(ns, heads, ld, dtype=torch.float32)
    for i, (s0, S) in enumerate(zip(A._starts(lens), lens)):
        if S == 0:
            continue
        xs = x[s0:s0 + S].view(S, 3, heads, 64)
        q = (xs[min(q_pos, S - 1), 0] * 0.125).view(heads, 8, 8)               # [heads, lane, dim]; the 1/8 is exact
        k = xs[:, 1].reshape(S, heads, 8, 8)
        d = torch.zeros(S, heads, 8, dtype=torch.float32)
        for j in range(8):                                                     # the per-lane fma chain
            d = d + q[None, :, :, j] * k[:, :, :, j]
        d = d[..., 0::2] + d[..., 1::2]                                        # lane ^ 1
        d = d[..., 0::2] + d[..., 1::2]                                        # lane ^ 2
        d = d[..., 0] + d[..., 1]                                              # lane ^ 4
        s = d + kb[s0:s0 + S][:, None]                                         # [S, heads]
        rounds = (S + 255) // 256
        sp = torch.full((rounds * 256, heads), _NINF, dtype=torch.float32)
        sp[:S] = s
        sp = sp.view(rounds, 8, 32, heads)                                     # key = 256 t + 32 u + g
        m = torch.full((32, heads), _NINF, dtype=torch.float32)
        l = torch.zeros(32, heads, dtype=torch.float32)
        for t in range(rounds):
            active = (256 * t + torch.arange(32) < S)[:, None]                 # the group's first key of the round exists
            blk = sp[t]
            mnew = torch.maximum(blk.amax(0), m)
            ln = l * torch.exp2((m - mnew) * _L2E)
            for u in range(8):
                ln = ln + torch.exp2((blk[u] - mnew) * _L2E)
            m, l = torch.where(active, mnew, m), torch.where(active, ln, l)
        m, l = m.view(4, 8, heads), l.view(4, 8, heads)
        for _ in range(3):                                                     # groups ^ 1, ^ 2, ^ 4 of a wave
            m, l = _merge(m[:, 0::2], l[:, 0::2], m[:, 1::2], l[:, 1::2])
        M, Lt = m[0, 0], l[0, 0]
        for w in range(1, 4):                                                  # the 4 waves in order
            M, Lt = _merge(M, Lt, m[w, 0], l[w, 0])
        inv = 1.0 / Lt
        out[i, :, :S] = (torch.exp2((s - M[None, :]) * _L2E) * inv[None, :]).t()
    return out


# ------------------------------------------------------------------------------------------------ the check
def ratios_probs(got, ref_p, ref_s):
    """{"l1", "elem": [sequences, heads] error / bound (<= 1 passes; inf: non-finite output or a non-zero where the reference is an
    exact zero), "l1_u", "elem_u": the same errors in units of u resp. u * max p_ref (what PHI is calibrated on)}."""
    g = got.detach().double().cpu()
    assert g.shape == ref_p.shape, (g.shape, ref_p.shape)
    nz = ref_p > 0
    smax = torch.where(nz, ref_s.abs(), torch.zeros_like(ref_p)).amax(-1)
    u = U32 * smax.clamp_min(1.0)
    diff = (g - ref_p).abs()
    l1_u = diff.sum(-1) / u
    el_u = diff.amax(-1) / (u * ref_p.amax(-1).clamp_min(1e-300))
    empty = ~nz.any(-1)                                                        # a block without keys: all zeros expected
    el_u = torch.where(empty, torch.zeros_like(el_u), el_u)
    bad = (~torch.isfinite(g)).any(-1) | ((g != 0) & ~nz).any(-1)
    inf = torch.full_like(l1_u, math.inf)
    l1_u, el_u = torch.where(bad, inf, torch.nan_to_num(l1_u, nan=math.inf)), torch.where(bad, inf, torch.nan_to_num(el_u, nan=math.inf))
    return {"l1": l1_u / PHI, "elem": el_u / PHI, "l1_u": l1_u, "elem_u": el_u}


def check_probs(got, ref_p, ref_s, what=""):
    """Assert every (sequence, head) block within its bounds (module docstring).  Returns (largest L1, largest elementwise) error in
    units of u resp. u * max p_ref."""
    r = ratios_probs(got, ref_p, ref_s)
    worst = torch.maximum(r["l1"], r["elem"])
    bad = (~(worst <= 1.0)).nonzero()
    if bad.numel():
        lines = [f"seq {int(s)} head {int(h)}: L1 {float(r['l1_u'][s, h]):.3g} u, elementwise {float(r['elem_u'][s, h]):.3g} u max p (PHI = {PHI})"
                 for s, h in bad[:8]]
        raise AssertionError(f"{what}: {bad.shape[0]} of {worst.numel()} blocks out of bound\n  " + "\n  ".join(lines))
    return float(r["l1_u"].max()), float(r["elem_u"].max())
