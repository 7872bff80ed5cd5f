"""tests/heads_ref.py on the CPU: the restatement of the heads' forward and hand-derived backward equals float64 autograd through the
oracle, every term of every multi-term output counts on the generated inputs, the emulation of the kernels' fp32 roundings passes
``check`` with about a factor 2 to spare, and every value-only mutation of the emulation fails it.

Largest emulation ratio over every case: 0.32 (elementwise, a parameter gradient).

Smallest margin of a mutation (error / bound of the mutated emulation; > 1 fails): 4.1e3, the last sample's row lost from the
pooler's bias sum at B = 17.  Next: pooler tanh' x (1 + 2^-6) 1.0e4, beta x (1 + 2^-6) in dS only 1.4e4, softmax over the columns
2.6e4, then 1.6e5 ... 9.4e8 (the CPC -XPn o csum / -Xn o rsum terms, gate dP through W1 only, a gradient overwritten or ignoring
d, ap2 ignored, drel shifted by a sample, the diagonal from a neighbour, tanh' missing in the 1-label loss, dmlm = d alpha / 3, the
last K granule of the pooler dropped at H = 80, E = dg Apre).
"""
import pytest
import torch

from tests import heads_ref as HR

torch.set_num_threads(min(16, torch.get_num_threads()))

EMU_LIMIT = 0.6            # the emulation's ratios stay below this (about half the bound)
MIN_MARGIN = 8.0
CASES = [dict(B=1, H=16, num_labels=7, nmlm=0, d=1.0), dict(B=3, H=80, num_labels=1, nmlm=3, d=-0.37),
         dict(B=17, H=80, num_labels=7, nmlm=256, d=2.0 ** 10, ap="zeros"), dict(B=16, H=64, num_labels=1, nmlm=3, d=-0.37, ap="ones"),
         dict(B=33, H=256, num_labels=7, nmlm=3, d=-0.37), dict(B=65, H=64, num_labels=7, nmlm=0, d=1.0, beta=0.0)]


def _case(i, kw):
    kw = dict(kw)
    B, H = kw.pop("B"), kw.pop("H")
    return HR.make_case(B, H, 40 + i, **kw)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_equals_float64_autograd_and_emulation_passes(i):
    c = _case(i, CASES[i])
    ref = HR.reference(c)
    terms = {}
    rs = HR.restate(c, terms=terms)
    for k in HR.OUTPUTS:
        if ref.get(k) is None:
            assert rs[k] is None, k
            continue
        a, b = ref[k].reshape(-1), rs[k].v.reshape(-1)
        assert float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1e-300), k
    if c.beta != 0 and c.B > 1:
        # every term of every multi-term sum counts (>= 1e-3 of the largest term; one sample has no in-batch negatives: dS = 0)
        for k, ts in terms.items():
            flat = [float(x) for t in ts for x in (t if isinstance(t, tuple) else (t,))]
            assert min(flat) >= 1e-3 * max(flat), (k, flat)
    exp = HR.expected(c, ref, rs)
    em = HR.restate(c, emu=True)
    worst = 0.0
    for k, r in exp.items():
        q = HR.ratios(em[k].v.reshape(r.val.shape), r)
        assert q.worst <= EMU_LIMIT, (k, q)
        worst = max(worst, q.worst)
    assert HR.kink_ratio(c) >= HR.KINK
    print(f"\n{CASES[i]}: emulation ratio {worst:.3f}")


MUTATIONS = [
    (HR.cpc_csum_dropped(1), dict(B=17, H=64)),
    (HR.cpc_rsum_dropped(2), dict(B=17, H=64)),
    (HR.softmax_over_columns(0), dict(B=16, H=64)),
    (HR.positive_from_neighbour(), dict(B=16, H=64)),
    (HR.beta_in_dS(), dict(B=16, H=64)),
    (HR.speech_labels_from_visual(), dict(B=16, H=64)),
    (HR.drel_rows_shifted(), dict(B=16, H=64)),
    (HR.gate_dP_w1_only(), dict(B=16, H=64)),
    (HR.e_without_relu(), dict(B=16, H=64)),
    (HR.pooler_tanh_grad(), dict(B=16, H=64)),
    (HR.label_tanh_grad_missing(), dict(B=16, H=64, num_labels=1)),
    (HR.grad_ignores_d("cpc_zv.net.bias"), dict(B=16, H=64, d=-0.37)),
    (HR.grad_overwritten("attn.bias"), dict(B=16, H=64)),
    (HR.gbp_last_row_lost(), dict(B=17, H=64)),
    (HR.dmlm_over_three(), dict(B=16, H=64, nmlm=256)),
    (HR.last_granule_dropped(), dict(B=16, H=80)),
]


@pytest.mark.parametrize("j", range(len(MUTATIONS)), ids=[m.name for m, _ in MUTATIONS])
def test_mutation_fails_the_check(j):
    mut, kw = MUTATIONS[j]
    kw = dict(kw)
    B, H = kw.pop("B"), kw.pop("H")
    c = HR.make_case(B, H, 7, **kw)
    exp = HR.expected(c)
    em = HR.restate(c, emu=True, mutation=mut)
    margin = max(HR.ratios(em[k].v.reshape(r.val.shape), r).worst for k, r in exp.items())
    print(f"\n{mut.name}: margin {margin:.3g}")
    assert margin >= MIN_MARGIN, (mut.name, margin)
