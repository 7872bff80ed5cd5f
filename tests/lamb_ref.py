"""float64 reference of the LAMB step that mmbert_lamb / msa_amd.optim.LAMB take (no GPU, numpy only): the rule over a list of
tensors of flat buffers, and the scales the kernel's bounds are stated in.

    g' = gscale g        m = b1 m + (1 - b1) g'        v = b2 v + (1 - b2) g'^2
    u  = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd p
    r  = ||p|| / ||u|| over the tensor when both are > 0, else 1; 1 as well when the tensor's wd is 0 and not always_adapt;
         min(r, max_trust) when max_trust is given
    p  = p - lr r u
"""
import numpy as np


def coefs(h, step, f32=False):
    """(b1, b2, 1 - b1, 1 - b2, eps, 1 / (1 - b1^t), 1 / (1 - b2^t), lr, wd) of one (lr, b1, b2, eps, wd): exact Python floats, or with
    ``f32`` each formed in double and rounded to fp32 once -- the values the kernel multiplies by, as float64."""
    lr, b1, b2, eps, wd = (float(x) for x in h)
    c = (b1, b2, 1.0 - b1, 1.0 - b2, eps, 1.0 / (1.0 - b1 ** step), 1.0 / (1.0 - b2 ** step), lr, wd)
    return tuple(float(np.float32(x)) for x in c) if f32 else c


def lamb_step(P, G, M, V, tensors, hyper, step, *, gscale=1.0, decay=None, always_adapt=False, max_trust=None, f32_coefs=False):
    """One step over float64 copies of the flat buffers.  ``tensors``: (offset, length, group) per tensor, disjoint; ``hyper``: (lr, b1,
    b2, eps, wd) per group; ``decay[k]``: whether tensor k applies its group's wd -- the kernel's "decay" flag of the tensor's blocks, one
    bool or one per element (default: it does; a tensor no element of which has wd > 0 counts as wd = 0).  Elements in no tensor keep
    their values.  Returns a dict: P, M, V (new buffers); U (the update direction per element) and A = |mhat / (sqrt(vhat) + eps)| + |wd p| (the scale of U's rounding error), 0 outside the tensors; per tensor R (the
    ratio applied), NP = ||p||, NU = ||u||, CANCEL = ||a|| / ||u|| (1 unless U's two terms cancel; 1 where ||u|| = 0)."""
    P, G, M, V = (np.array(x, dtype=np.float64).reshape(-1).copy() for x in (P, G, M, V))
    U, A = np.zeros_like(P), np.zeros_like(P)
    nt = len(tensors)
    R, NP, NU, CANCEL = np.ones(nt), np.zeros(nt), np.zeros(nt), np.ones(nt)
    for k, (off, length, grp) in enumerate(tensors):
        s = slice(off, off + length)
        b1, b2, omb1, omb2, eps, rbc1, rbc2, lr, wd = coefs(hyper[grp], step, f32_coefs)
        if decay is not None:
            wd = wd * np.asarray(decay[k], dtype=np.float64)               # (per tensor, or per element: the blocks' "decay" flags)
        g = G[s] * gscale
        M[s] = b1 * M[s] + omb1 * g
        V[s] = b2 * V[s] + omb2 * g * g
        adam = (M[s] * rbc1) / (np.sqrt(V[s] * rbc2) + eps)
        U[s] = adam + wd * P[s]
        A[s] = np.abs(adam) + np.abs(wd * P[s])
        NP[k], NU[k] = np.sqrt(np.sum(P[s] ** 2)), np.sqrt(np.sum(U[s] ** 2))
        if (always_adapt or np.any(wd > 0.0)) and NP[k] > 0.0 and NU[k] > 0.0:
            R[k] = NP[k] / NU[k]
        if max_trust is not None:
            R[k] = min(R[k], float(max_trust))
        if NU[k] > 0.0:
            CANCEL[k] = np.sqrt(np.sum(A[s] ** 2)) / NU[k]
        P[s] = P[s] - lr * R[k] * U[s]
    return dict(P=P, M=M, V=V, U=U, A=A, R=R, NP=NP, NU=NU, CANCEL=CANCEL)


def ratio_bound(R, CANCEL):
    """|r - R| allowed of the fp32 kernel: 2e-6 R ||a|| / ||u||.  An element of u carries a handful of fp32 roundings and two 1-ulp
    hardware approximations (sqrt, rcp), about 4e-7 of a; the partial sums are fp32 sums of 256 squares, folded in double."""
    return 2e-6 * np.asarray(R) * np.asarray(CANCEL)


def p_bound(P0, lr, R, U):
    """|p - P| allowed per element: 2e-6 (|P0| + lr R |U|), the grouped AdamW kernel's bound with the LAMB step as the update term."""
    return 2e-6 * (np.abs(P0) + lr * R * np.abs(U))
