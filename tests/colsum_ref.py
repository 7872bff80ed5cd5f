"""The float64 column sum ``ops.colsum_grouped`` is held to, and its bound.

Not a test module (pytest does not collect it): ``from tests import colsum_ref``.  Used by tests/test_colsum_grouped_gpu.py (the kernel
alone) and tests/step_stages.py (the calls a frozen step makes).

Bound per output: ``scale * M * 2^-24 * sum_m |x| + 2^-23 * |ref|`` -- the worst case of ANY fp32 summation order of M terms (each of the at
most M - 1 additions rounds by at most 2^-24 of a partial sum that |x|'s sum bounds, the scaling rounds once more) plus the rounding of the
output (where the call accumulates: of the final addition; ``ref`` then includes the prior value)."""
import torch


def reference(x, prior, acc, scale=1.0):
    """(ref, bound) float64 [N] of out (+)= scale * x.sum(0); ``x`` [M, N] bf16, ``prior`` [N] fp32 (read only where ``acc``)."""
    M = x.shape[0]
    x64 = x.double()
    ref = scale * x64.sum(0) + (prior.double() if acc else 0.0)
    bound = abs(scale) * M * 2.0 ** -24 * x64.abs().sum(0) + 2.0 ** -23 * ref.abs()
    return ref, bound


def errors(out, x, prior, acc, scale=1.0):
    """(|out - ref|, bound) float64 [N]."""
    ref, bound = reference(x, prior, acc, scale)
    return (out.double() - ref).abs(), bound


def ratio(out, x, prior, acc, scale=1.0) -> float:
    """The largest error / bound (<= 1 passes; an error where the bound is 0, or a NaN, is inf)."""
    err, bound = errors(out, x, prior, acc, scale)
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.nan_to_num(q, nan=float("inf"), posinf=float("inf"))
    return float(q.max()) if q.numel() else 0.0
