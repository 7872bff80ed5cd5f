"""mmbert_colsum_grouped (ops.colsum_grouped) against float64 column sums.

Bound per output: ``M * 2^-24 * sum_m |x| + 2^-23 * |ref|`` -- the worst case of ANY fp32 summation order of M terms (each of the at most
M - 1 additions rounds by at most 2^-24 of a partial sum that |x|'s sum bounds, the scaling by alpha rounds once more) plus the rounding of
the output (where the call accumulates: of the final addition; ``ref`` then includes the prior value).  Reference and bound live in
tests/colsum_ref.py, which tests/step_stages.py shares."""
import pytest
import torch

from tests import colsum_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS = (1, 3, 33, 1000)
NS = (8, 136, 520)
ALPHA, ALPHA_DEV = 0.5, 3.0


def _problems(seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    probs, acc = [], []
    for i, M in enumerate(MS):
        for j, N in enumerate(NS):
            x = torch.randn((M, N), generator=g).to(torch.bfloat16)
            if M == 1000 and N == 136:
                x[:, 5] = torch.rand(M, generator=g).to(torch.bfloat16) + 0.5          # a column of all-positive values: no cancellation
            probs.append(x.to(DEV))
            acc.append((i + j) % 2 == 0)
    # a column window [8, 8 + 136) of a wider matrix (ldx = 160 > N): everything outside the window is 1e30
    wide = torch.full((33, 160), 1e30, dtype=torch.bfloat16)
    wide[:, 8:144] = torch.randn((33, 136), generator=g).to(torch.bfloat16)
    probs.append(wide.to(DEV)[:, 8:144])
    acc.append(True)
    probs.append(torch.empty((0, 136), dtype=torch.bfloat16, device=DEV))              # M == 0: skipped, its output untouched
    acc.append(False)
    return probs, acc


def _run(probs, acc, prior_seed=1):
    from msa_amd import ops
    g = torch.Generator(device="cpu").manual_seed(prior_seed)
    prior = [torch.randn(x.shape[1], generator=g).to(DEV) for x in probs]
    out = [p.clone() for p in prior]
    ops.colsum_grouped(list(zip(probs, out)), accumulate=acc, alpha=ALPHA, alpha_dev=torch.tensor([ALPHA_DEV], device=DEV))
    return prior, out


def _check(x, prior, out, acc, scale):
    M = x.shape[0]
    if M == 0:
        assert torch.equal(out, prior)
        return
    err, bound = colsum_ref.errors(out, x, prior, acc, scale)
    print(f"M={M} N={x.shape[1]} acc={acc} max err {float(err.max()):.3e} max bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), (M, x.shape[1], float((err - bound).max()))


def test_mixed_call_against_float64():
    probs, acc = _problems()
    prior, out = _run(probs, acc)
    for x, p, o, a in zip(probs, prior, out, acc):
        _check(x, p, o, a, ALPHA * ALPHA_DEV)


def test_one_and_fifty_two_problems():
    from msa_amd import ops
    g = torch.Generator(device="cpu").manual_seed(7)
    xs = [torch.randn((3 + 5 * i, 8 * (1 + i % 5)), generator=g).to(torch.bfloat16).to(DEV) for i in range(52)]
    for n in (1, 52):
        prior, out = _run(xs[:n], [False] * n)
        for x, p, o in zip(xs[:n], prior, out):
            _check(x, p, o, False, ALPHA * ALPHA_DEV)
    ops.colsum_grouped([])                                           # an empty call: nothing happens


def test_bits_are_reproducible_and_independent_of_deterministic_mode():
    from msa_amd import ops
    probs, acc = _problems()
    was = ops.deterministic()
    try:
        ops.set_deterministic(False)
        _, a = _run(probs, acc)
        _, b = _run(probs, acc)
        ops.set_deterministic(True)
        _, c = _run(probs, acc)
    finally:
        ops.set_deterministic(was)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_bad_width_is_refused():
    from msa_amd import ops
    x = torch.zeros((4, 12), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="mmbert_colsum_grouped failed with code -1"):
        ops.colsum_grouped([(x, torch.zeros(12, device=DEV))])
