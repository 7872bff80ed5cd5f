"""Shared by the CPU and GPU tests of ``attn_fwd_first`` (one query row per sequence): the case list and an fp32 emulation of the
kernel's documented arithmetic.  Not a test module (pytest does not collect it).

The kernel (csrc/attention.hip, ``attn_fwd_first_kernel``): the query row times 1/8 in fp32 (exact), fp32 scores q.k + key_bias, fp32
softmax, fp32 P.V, ONE bf16 rounding at the store.  ``emulate_first`` is that in fp32 torch on the CPU; it is compared with the float64
``attention_ref.reference`` through ``attention_ref.check(..., rows=first_rows(lens))`` at the module's own ``TAU["ctx"]`` /
``KAPPA["ctx"]`` -- no new tolerance."""
import torch

from tests import attention_ref as A

HEADLINE_LENS = [50] * 16 + [550] * 32


def cases():
    """(name, lens, heads, patterns, qk_scale): EDGE_LENS x PATTERNS rotated as in test_edge_lengths_packed_together, heads 1 / 3 / 12 /
    16, qk_scale 1 and 2.83; the headline set 16 x 50 + 32 x 550 at 12 heads."""
    for heads in (1, 3, 12, 16):
        for qs in (1.0, 2.83):
            pats = [A.PATTERNS[(i + heads) % len(A.PATTERNS)] for i in range(len(A.EDGE_LENS))]
            yield f"edge-h{heads}-s{qs}", list(A.EDGE_LENS), heads, pats, qs
    pats = [("none", "tail_inside", "random", "tail_boundary")[i % 4] for i in range(len(HEADLINE_LENS))]
    yield "headline-h12", list(HEADLINE_LENS), 12, pats, 1.0


CASES = list(cases())


def inputs(name, lens, heads, pats, qs):
    qkv, bias, _ = A.make_inputs(lens, heads, pats, seed=len(name) * 11 + heads, qk_scale=qs)
    return qkv, bias


def first_rows(lens):
    """bool [M]: row 0 of every sequence."""
    sel = torch.zeros(sum(lens), dtype=torch.bool)
    sel[torch.tensor(A._starts(lens))] = True
    return sel


def emulate_first(qkv_bf16, key_bias, lens, heads, q_pos=0):
    """{"ctx": [M, H] float64}: zero but at row 0 of every sequence, which holds the kernel's arithmetic for the query at position
    ``q_pos`` of the sequence (0 = the kernel; 1 = the "wrong query row" mutation; clamped to the sequence)."""
    H = heads * 64
    x = qkv_bf16.to(torch.bfloat16).float()
    kb = key_bias.float().reshape(-1)
    out = torch.zeros(sum(lens), H, dtype=torch.float64)
    for s0, S in zip(A._starts(lens), lens):
        xs = x[s0:s0 + S].view(S, 3, heads, 64)
        q = xs[min(q_pos, S - 1), 0] * 0.125                                     # [heads, 64] fp32, exact
        k, v = xs[:, 1].permute(1, 0, 2), xs[:, 2].permute(1, 0, 2)             # [heads, S, 64]
        s = torch.einsum("hd,hkd->hk", q, k) + kb[s0:s0 + S][None, :]           # fp32 scores
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.einsum("hk,hkd->hd", p, v) / p.sum(-1, keepdim=True)
        out[s0] = o.to(torch.bfloat16).double().reshape(H)
    return {"ctx": out}


def expand_first(ctx_compact, lens):
    """The kernel's compact [sequences, H] context as the {"ctx": [M, H]} dict ``check`` reads (row 0 of every sequence)."""
    out = torch.zeros(sum(lens), ctx_compact.shape[1], dtype=torch.float64)
    out[torch.tensor(A._starts(lens))] = ctx_compact.detach().double().cpu()
    return {"ctx": out}
