"""The float64 attention reference and its check (tests/attention_ref.py), without a GPU.

1. ``emulate`` -- the reference with the roundings the kernels document -- passes ``check`` on every calibration case: the
   bounds are loose enough for a correct bf16 kernel.
2. Every mutation of ``attention_ref`` (a lost key at a 64-key tile edge and at the end of a partial tail tile, a key mask moved
   to its neighbour, a neighbouring head's dropout mask, the softmax scale x (1 + 2^-5), delta left out for one 16-row block, dV
   without the dropout scale) fails ``check`` against the reference with margin: some output of every mutated (sequence,
   head) block sits at >= 2x its bound, and every other block stays within bound.  A kernel carrying one of these bugs is
   the mutation plus at most the emulation's rounding (<= 1/2 of every bound), so it would still fail.

Measured with the bounds of attention_ref: smallest mutation margin 4.2x (the softmax scale, edge lengths at 16 heads, over
the blocks with S >= 3; at S <= 2 the scale shows only through one or two scores and those blocks reach 1.96x), next 6.3x (delta
left out for rows 1040 ... 1049 at S = 1050); every lost key, moved mask, neighbouring head's mask and unscaled dV >= 12x.
About 16 s of wall time on 8 cores.
"""
import pytest
import torch

from tests import attention_ref as A


def _cases():
    for heads in (1, 3, 12, 16):
        for p in (0.0, 0.1):
            for rot in range(2):
                pats = [A.PATTERNS[(i + rot * 3 + heads) % len(A.PATTERNS)] for i in range(len(A.EDGE_LENS))]
                yield f"edge-h{heads}-p{p}-r{rot}", A.EDGE_LENS, heads, pats, p, 1.0, None
    yield "long-h12-p0.1", [550, 1050], 12, ["random", "tail_inside"], 0.1, 1.0, None
    yield "long-h12-p0", [550, 1050], 12, ["none", "random"], 0.0, 1.0, None
    plan = [(0, 3, [0, 2, 5]), (0, 100, [17, 20]), (0, 195, [40, 41, 45]), (1, 128, [1, 7])]
    yield "rescale-h12-p0.1", [200, 129], 12, ["none", "none"], 0.1, 2 ** 1.5, plan
    yield "rescale-h12-p0", [200, 129], 12, ["none", "random"], 0.0, 2 ** 1.5, plan


CALIBRATION_CASES = list(_cases())


def _inputs(name, lens, heads, pats, p, qs, plan):
    qkv, bias, dctx = A.make_inputs(lens, heads, pats, seed=len(name) * 7 + heads, qk_scale=qs)
    if plan:
        qkv = A.spike_rescale(qkv, lens, heads, plan)
    keep = A.random_keep(lens, heads, p, torch.Generator().manual_seed(3)) if p > 0 else None
    return qkv, bias, dctx, keep, 1.0 / (1.0 - p)


@pytest.mark.parametrize("case", CALIBRATION_CASES, ids=[c[0] for c in CALIBRATION_CASES])
def test_emulated_kernel_rounding_passes_the_check(case):
    name, lens, heads = case[:3]
    qkv, bias, dctx, keep, ds = _inputs(*case)
    ref = A.reference(qkv, bias, lens, heads, keep, ds, dctx)
    emu = A.emulate(qkv, bias, lens, heads, keep, ds, dctx)
    worst = A.check(emu, ref, lens, heads, name)
    assert set(worst) == set(A.KINDS)
    assert max(worst.values()) <= 0.6, worst                 # the bounds sit at about 2x the emulation


def _margins(mut, ref, qkv, bias, lens, heads, keep, ds, dctx):
    got = A.reference(qkv, bias, lens, heads, keep, ds, dctx, mutation=mut)
    res = A.ratios(got, ref, lens, heads)
    blocks = mut.blocks if mut.blocks is not None else {(s, h) for s in range(len(lens)) for h in range(heads)}
    hit, rest = {}, 0.0
    for (s, h, kind), w in res.items():
        if (s, h) in blocks:
            hit[(s, h)] = max(hit.get((s, h), 0.0), w.ratio)
        else:
            rest = max(rest, w.ratio)
    assert set(hit) == blocks, mut.name
    # a global mutation (the softmax scale) shows in a sequence of one or two keys only through those one or two scores: there
    # the block has to fail (ratio > 1), not by 2x
    short = [r for (s, h), r in hit.items() if lens[s] <= 2]
    assert mut.blocks is not None or all(r > 1.0 for r in short), (mut.name, short)
    long_ = [r for (s, h), r in hit.items() if lens[s] > 2 or mut.blocks is not None]
    return min(long_), rest


def _mutation_case(name, lens, heads, pats, p, unmask):
    qkv, bias, dctx, keep, ds = _inputs(name, lens, heads, pats, p, 1.0, None)
    starts = A._starts(lens)
    for s, k in unmask:                                        # the keys the mutations drop must be unmasked
        bias[starts[s] + k] = 0.0
    ref = A.reference(qkv, bias, lens, heads, keep, ds, dctx)
    return qkv, bias, dctx, keep, ds, ref


def _first_masked_then_unmasked(bias, s0, n):
    b = bias[s0:s0 + n]
    for j in range(n - 1):
        if float(b[j]) <= A.MASKED and float(b[j + 1]) > A.MASKED:
            return j
    raise AssertionError("no masked key followed by an unmasked one")


def test_every_mutation_fails_the_check_with_margin():
    # the model's lengths: S = 550 (pair passes) and 1050 (the fused leg) at 12 heads, p = 0.1, and a partial tail tile at S = 129
    lens, heads = [550, 1050, 129], 12
    qkv, bias, dctx, keep, ds, ref = _mutation_case("long", lens, heads, ["random", "random", "none"], 0.1,
                                                    [(0, 63), (0, 64), (0, 549), (1, 64), (1, 1049)])
    starts = A._starts(lens)
    muts = [
        A.drop_key(0, 5, 63), A.drop_key(0, 5, 64), A.drop_key(0, 0, 549),       # tile edge; last key of the partial tail tile
        A.drop_key(1, 11, 64), A.drop_key(1, 2, 1049),
        A.drop_key(2, 7, 128),
        A.move_mask(1, _first_masked_then_unmasked(bias, starts[1], lens[1]), heads),
        A.move_mask(0, _first_masked_then_unmasked(bias, starts[0], lens[0]), heads),
        A.neighbour_dropout(0, 4, heads), A.neighbour_dropout(1, 11, heads),
        A.softmax_scale(),
        A.drop_delta(0, 3, 32), A.drop_delta(1, 7, 1040), A.drop_delta(2, 0, 112),
        A.dv_without_dropout_scale(2, 0), A.dv_without_dropout_scale(1, 9),
    ]
    worst = []
    for mut in muts:
        hit, rest = _margins(mut, ref, qkv, bias, lens, heads, keep, ds, dctx)
        worst.append((hit, mut.name))
        assert rest == 0.0, (mut.name, rest)                                      # other blocks: untouched
    low = [w for w in worst if not w[0] >= 2.0]
    assert not low, f"mutations without a 2x margin: {low}"


@pytest.mark.parametrize("heads", [3, 16])
def test_mutations_on_the_packed_edge_lengths(heads):
    """The same at the edge lengths: a lost last key of the partial tail tile of S = 65 / 129 / 257, the softmax scale on every
    block (S = 1 included: its LSE), a neighbouring head's dropout mask and the delta of one 16-row block at S = 17 / 255."""
    lens = A.EDGE_LENS
    pats = ["none"] * len(lens)
    pats[9], pats[13] = "random", "random"                    # S = 127, 256
    qkv, bias, dctx, keep, ds, ref = _mutation_case(f"edge{heads}", lens, heads, pats, 0.1, [])
    i = {n: lens.index(n) for n in lens}
    muts = [A.drop_key(i[65], heads - 1, 64), A.drop_key(i[129], 1, 128), A.drop_key(i[257], 0, 256), A.drop_key(i[64], 2, 63),
            A.softmax_scale(), A.neighbour_dropout(i[17], heads - 1, heads), A.neighbour_dropout(i[256], 0, heads),
            A.drop_delta(i[17], 0, 16), A.drop_delta(i[255], 1, 240),
            A.move_mask(i[127], _first_masked_then_unmasked(bias, A._starts(lens)[i[127]], 127), heads)]
    low = []
    for mut in muts:
        hit, rest = _margins(mut, ref, qkv, bias, lens, heads, keep, ds, dctx)
        assert rest == 0.0, (mut.name, rest)
        if not hit >= 2.0:
            low.append((hit, mut.name))
    assert not low, f"mutations without a 2x margin: {low}"
