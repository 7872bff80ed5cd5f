"""GPU tests of the flat LAMB step (mmbert_lamb) through ops.lamb: the moments bit for bit against the grouped AdamW
kernel, the trust ratios and the parameters against float64 (tests/lamb_ref.py) over three unit layouts -- one unit, a unit per block, a
packed layout with mixed blocks --, frozen blocks, the fused zero_grad and its lazy flag, the bf16 copy, the EMA, run-to-run bits, padding,
the refusals."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ema_ref as E
from tests import lamb_ref as L
from tests.test_adamw_groups_gpu import HYPER7, _random_state

DEV = "cuda"
STEP, GSCALE = 3, 0.37
CASES = [(lay, nblk) for lay in ("one", "each", "packed") for nblk in (1, 5, 4099)]


def _packs(nblk, rng):
    """The packed layout: (tensor lengths packed from a block's first element | None for frozen blocks, number of blocks, what is special)
    in buffer order, cut to nblk blocks.  The fixed head holds every shape the kernel treats differently; a random tail fills the rest."""
    head = [([64, 64], 1, None),                     # 64 | 64 | padding 128
            ([64, 64, 64], 1, None),                 # 64 | 64 | 64 | padding 64
            ([36, 92], 1, None),                     # quad boundaries that are no multiple of 64
            (None, 1, None),                         # frozen between units
            ([256], 1, "zero"),                      # an all-zero tensor
            ([128, 128 + 512 + 10], 4, None),        # a tensor that starts mid-block, two pure blocks, 10 elements of a fourth
            (None, 2, None),
            ([200], 1, "still")]                     # g = m = 0 and wd = 0: a zero update
    out, used = [], 0
    for p in head:
        if used + p[1] <= nblk:
            out.append(p)
            used += p[1]
    while used < nblk:
        kind = int(rng.integers(0, 5))
        if kind == 0:
            p = (None, int(rng.integers(1, 3)), None)
        elif kind == 1:
            p = ([64, 64] if rng.integers(0, 2) else [128, 128], 1, None)
        else:
            k = int(rng.integers(1, 7))
            p = ([256 * k - 4 * int(rng.integers(0, 40))], k, None)
        if used + p[1] > nblk:
            p = ([256 * (nblk - used)], nblk - used, None)
        out.append(p)
        used += p[1]
    return out


@functools.lru_cache(maxsize=None)
def _case(layout, nblk):
    """The inputs of one (layout, size), built once and never written: device buffers, flags and maps, and the float64 reference."""
    from msa_amd.optim import lamb_unit_maps
    p, g, m, v, flags, rng = _random_state(nblk, 4000 + nblk + {"one": 0, "each": 1, "packed": 2}[layout])
    fl = flags.cpu().numpy().copy()
    if (fl & 3 == 2).all():
        fl[0] = 1 | (fl[0] & 4)                      # (one block, drawn frozen: nothing would be tested)
    gmap = np.zeros(nblk, dtype=np.uint8)
    spans, groups, pad = [], [], np.zeros(nblk * 256, dtype=bool)
    if layout == "one":
        gmap[:] = 2
        spans, groups = [(0, nblk * 256)], [2]
    elif layout == "each":
        gmap[:] = rng.integers(0, len(HYPER7), nblk)
        live = np.nonzero(fl & 3 != 2)[0]
        spans, groups = [(256 * int(b), 256) for b in live], [int(gmap[b]) for b in live]
    else:
        b = 0
        p, g, m, v = (x.clone() for x in (p, g, m, v))
        for lens, k, special in _packs(nblk, rng):
            sl = slice(256 * b, 256 * (b + k))
            if lens is None:
                fl[b:b + k] = 2 | (fl[b:b + k] & 4)
            else:
                grp = 1 if special == "still" else int(rng.integers(0, len(HYPER7)))
                dec = 0 if special == "still" else int(rng.integers(0, 2))
                fl[b:b + k] = dec | (fl[b:b + k] & 4)
                gmap[b:b + k] = grp
                off = 256 * b
                for n in lens:
                    spans.append((off, n))
                    groups.append(grp)
                    off += n
                pad[off:256 * (b + k)] = True
                if special == "zero":
                    for x in (p, g, m, v):
                        x[sl] = 0.0
                if special == "still":
                    g[sl] = 0.0
                    m[sl] = 0.0
            b += k
        padt = torch.from_numpy(pad).to(DEV)
        for x in (p, g, m, v):
            x[padt] = 0.0                            # padding is zero in the flat storage
    unit, mixed, ranges = lamb_unit_maps(spans, nblk)
    live_el = np.repeat(fl & 3 != 2, 256)
    dec_el = np.repeat(fl & 3 == 1, 256)
    elems = [np.arange(o, o + n)[live_el[o:o + n]] for o, n in spans]        # (the one-unit layout runs over frozen blocks: not its elements)
    adapt = [bool(HYPER7[grp][4] > 0 and dec_el[e].any()) for grp, e in zip(groups, elems)]
    units = np.zeros((len(spans), 4), dtype=np.int32)
    units[:, :2] = ranges
    units[:, 2] = adapt
    # float64: every unit's live elements gathered into one contiguous tensor, stepped, scattered back
    P0, G0, M0, V0 = (x.double().cpu().numpy() for x in (p, g, m, v))
    idx = np.concatenate(elems) if elems else np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum([len(e) for e in elems])])
    tensors = [(int(starts[k]), len(e), groups[k]) for k, e in enumerate(elems)]
    ref = L.lamb_step(P0[idx], G0[idx], M0[idx], V0[idx], tensors, HYPER7, STEP, gscale=float(np.float32(GSCALE)),
                      decay=[dec_el[e] for e in elems], f32_coefs=True)
    lr_el = np.concatenate([np.full(len(e), float(np.float32(HYPER7[groups[k]][0]))) for k, e in enumerate(elems)]) if elems else idx
    r_el = np.concatenate([np.full(len(e), ref["R"][k]) for k, e in enumerate(elems)]) if elems else idx
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(nblk=nblk, p=p, g=g, m=m, v=v, fl=fl, flags=dev(fl), gmap=dev(gmap), unit=dev(unit), mixed=dev(mixed), units=dev(units),
                spans=spans, elems=elems, adapt=adapt, idx=idx, ref=ref, pad=pad, P0=P0,
                pbound=L.p_bound(P0[idx], lr_el, r_el, ref["U"]))


def _run(c, dev_scale=False, zero_grad=True, bf16=True, ema=None, ema_decay=0.0, step=STEP, state=None, max_trust=None):
    from msa_amd import ops
    p, g, m, v = (x.clone() for x in (state or (c["p"], c["g"], c["m"], c["v"])))
    pb = torch.zeros_like(p, dtype=torch.bfloat16) if bf16 else None
    coef = torch.tensor([GSCALE], device=DEV) if dev_scale else None
    ratios = ops.lamb(p, g, m, v, pb, c["flags"], c["gmap"], HYPER7, c["unit"], c["mixed"], c["units"], step=step,
                      gscale=1.0 if dev_scale else GSCALE, coef=coef, zero_grad=zero_grad, ema=ema, ema_decay=ema_decay, max_trust=max_trust)
    return p, g, m, v, pb, ratios


def test_the_inputs_keep_the_cancellation_factor_small():
    """The ratio bound scales with ||a|| / ||u||: the chosen inputs keep it <= 2 for every tensor (CPU arithmetic on the cached cases)."""
    for lay, nblk in CASES:
        c = _case(lay, nblk)
        assert float(c["ref"]["CANCEL"].max(initial=1.0)) <= 2.0, (lay, nblk, float(c["ref"]["CANCEL"].max()))
    c = _case("packed", 4099)
    fl, unit = c["fl"], c["unit"].cpu().numpy()
    live = fl & 3 != 2
    assert (unit[live] < -1).sum() > 100 and (unit[live] >= 0).sum() > 1000 and (~live).sum() > 100          # mixed, pure, frozen
    assert c["mixed"].cpu().numpy()[1:4].tolist() == [[0, 0, 16, 1, 64, -1, 64, -1], [0, 2, 16, 3, 32, 4, 64, -1], [0, 5, 9, 6, 64, -1, 64, -1]]
    assert any(not a for a in c["adapt"]) and any(c["adapt"])


@pytest.mark.parametrize("dev_scale", [False, True])
@pytest.mark.parametrize("layout,nblk", CASES)
def test_step_against_adamw_moments_and_float64(layout, nblk, dev_scale):
    from msa_amd import ops
    c = _case(layout, nblk)
    p, g, m, v, pb, ratios = _run(c, dev_scale)
    # m, v: the bits of the grouped AdamW kernel from the same inputs
    pa, ga, ma, va = (x.clone() for x in (c["p"], c["g"], c["m"], c["v"]))
    ops.adamw_grouped(pa, ga, ma, va, None, c["flags"], c["gmap"], HYPER7, step=STEP, gscale=1.0 if dev_scale else GSCALE,
                      coef=torch.tensor([GSCALE], device=DEV) if dev_scale else None, mode=0)
    assert torch.equal(m, ma) and torch.equal(v, va)
    # ratios
    ref, r = c["ref"], ratios.double().cpu().numpy()
    if len(c["spans"]):
        err, bound = np.abs(r[:, 0] - ref["R"]), L.ratio_bound(ref["R"], ref["CANCEL"])
        print(f"ratio: worst |r - R| / bound = {float((err / bound).max()):.3f} over {len(err)} units")
        assert bool((err <= bound).all()), (int(np.argmax(err / bound)), float((err / bound).max()))
        one = np.array([not a for a in c["adapt"]]) | (ref["NP"] == 0) | (ref["NU"] == 0)
        assert bool((ratios[:, 0].cpu().numpy()[one] == 1.0).all()) and bool((ref["R"][one] == 1.0).all())
        assert np.allclose(r[:, 1], ref["NP"], rtol=2e-6, atol=0) and np.allclose(r[:, 2], ref["NU"], rtol=4e-6, atol=0)
    # p
    idx = c["idx"]
    got = p.double().cpu().numpy()
    perr = np.abs(got[idx] - ref["P"])
    if len(idx):
        print(f"p: worst |p - P| / bound = {float((perr / np.maximum(c['pbound'], 1e-300)).max()):.3f}")
    assert bool((perr <= c["pbound"]).all())
    # frozen blocks bit-unchanged; the fused zero_grad and its lazy flag; the bf16 copy
    fl = torch.from_numpy(np.repeat(c["fl"], 256)).to(DEV)
    frozen, lazy = (fl & 3) == 2, (fl & 4) != 0
    for new, old in ((p, c["p"]), (m, c["m"]), (v, c["v"])):
        assert torch.equal(new[frozen], old[frozen])
    assert torch.equal(g[lazy], c["g"][lazy]) and int(torch.count_nonzero(g[~lazy])) == 0
    assert torch.equal(pb, p.bfloat16())
    # elements of live blocks that belong to no tensor (padding): +0 in, +0 out
    pad = torch.from_numpy(c["pad"]).to(DEV)
    for x in (p, m, v):
        assert int(torch.count_nonzero(x[pad])) == 0 and not bool(torch.signbit(x[pad]).any())
    # a second run: the same bits, ratios included
    for a, b in zip((p, g, m, v, pb, ratios), _run(c, dev_scale)):
        assert torch.equal(a, b)
    # zero_grad off and no bf16 copy: g is read only, nothing else changes
    p2, g2, m2, v2, _, r2 = _run(c, dev_scale, zero_grad=False, bf16=False)
    assert torch.equal(g2, c["g"]) and torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v) and torch.equal(r2, ratios)


@pytest.mark.parametrize("layout,nblk", [("packed", 4099), ("each", 5)])
def test_ema_leaves_the_step_alone_and_follows_the_new_weights(layout, nblk):
    c = _case(layout, nblk)
    base = _run(c, True)
    e0 = torch.randn(nblk * 256, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    ema = e0.clone()
    with_ema = _run(c, True, ema=ema, ema_decay=0.99)
    for a, b in zip(base, with_ema):
        assert torch.equal(a, b)
    frozen = torch.from_numpy(np.repeat(c["fl"] & 3 == 2, 256)).to(DEV)
    assert torch.equal(ema[frozen], e0[frozen])
    omd = E.omd_f32(0.99)
    want, bound = E.ema_step(e0, base[0], omd), E.ema_bound(e0, base[0], omd)
    assert bool(((ema.double() - want).abs() <= bound)[~frozen].all())
    assert not torch.equal(ema[~frozen], e0[~frozen])


def test_padding_stays_plus_zero_over_three_steps_and_max_trust_caps():
    c = _case("packed", 5)
    state = (c["p"], c["g"], c["m"], c["v"])
    for step in (1, 2, 3):
        p, g, m, v, _, ratios = _run(c, step=step, state=state, zero_grad=False)
        state = (p, g, m, v)
    pad = torch.from_numpy(c["pad"]).to(DEV)
    live_dec = torch.from_numpy(np.repeat(c["fl"] & 3 == 1, 256)).to(DEV)
    assert int(pad.sum()) >= 128 + 64 + 128
    for x in (p, m, v):
        assert int(torch.count_nonzero(x[pad])) == 0 and not bool(torch.signbit(x[pad]).any())
    assert not torch.equal(p[~pad & live_dec], c["p"][~pad & live_dec]) or not bool(live_dec.any())
    # max_trust: min(r, cap) of the uncapped run, bit for bit
    free = _run(c)[5][:, 0]
    cap = float(free.max()) * 0.5
    capped = _run(c, max_trust=cap)[5][:, 0]
    assert torch.equal(capped, torch.clamp(free, max=torch.tensor(cap, device=DEV).float().item())) and float(capped.max()) < float(free.max())


def test_refusals_return_minus_one_and_write_nothing():
    from msa_amd import ops
    c = _case("packed", 5)
    bufs = [x.clone() for x in (c["p"], c["g"], c["m"], c["v"])]
    ratios = torch.full((len(c["spans"]), 3), -7.0, device=DEV)
    args = (None, c["flags"], c["gmap"], HYPER7, c["unit"], c["mixed"], c["units"])

    def refused(*a, **k):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.lamb(*a, ratios=ratios, **k)

    refused(*bufs, *args, step=0)
    refused(*bufs, *args, max_trust=-1.0)
    refused(*bufs, *args, max_trust=float("nan"))
    refused(*bufs, *args, workspace=torch.empty(2 * 5 + 8 * c["mixed"].shape[0] - 2, device=DEV))       # one slot short
    refused(*bufs, *args, ema=torch.zeros_like(bufs[0]), ema_decay=1.0)
    refused(*bufs, *args[:6], c["units"][:0])                                                             # no unit
    refused(*bufs, None, c["flags"], c["gmap"], HYPER7 + [(9.0, 0.9, 0.999, 1e-6, 0.0)] * 249, *args[4:])  # 256 groups
    refused(*bufs, None, c["flags"], c["gmap"], [(1e-3 * (k + 1), 0.9, 0.999, 1e-6, 0.0) for k in range(65)], *args[4:])
    refused(*[x[:300].clone() for x in bufs], *args)                                                      # n % 256 != 0
    torch.cuda.synchronize()
    for x, y in zip(bufs, (c["p"], c["g"], c["m"], c["v"])):
        assert torch.equal(x, y)
    assert bool((ratios == -7.0).all())
    ops.lamb(*bufs, *args, ratios=ratios)                                                                 # (the same call, allowed)
    assert not bool((ratios == -7.0).any())
