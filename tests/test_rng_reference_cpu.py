"""CPU: the integer reference of tests/rng_ref.py against the library's host functions, against wrong generators that the GPU
file's exact comparison (tests/test_rng_gpu.py) must reject at its own cases, against an emulation of the attention kernels for
the mask read-back, and the survey of the correlation between the masks of pairs of streams."""
import ast
import os
import types

import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests import rng_cases as C
from tests import rng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_hash_and_threshold_fixed_points():
    """Values worked out by hand from the definition: hash32(0) = 0 (every step maps 0 to 0); the thresholds of the C comment
    (0.1 -> 6554, 0.5 -> 32768) and its edges; the signed keep rule against the unsigned form it stands for."""
    assert int(R.hash32(0)) == 0 and int(R.pair_bits(0, 0)) == 0
    x = 1
    x ^= x >> 16; x = x * 0x85EBCA6B % 2 ** 32; x ^= x >> 13; x = x * 0xC2B2AE35 % 2 ** 32; x ^= x >> 16
    assert int(R.hash32(1)) == x and int(R.hash32(2 ** 32 + 1)) == x
    assert [R.thr16(p) for p in (0.0, -1.0, 1e-9, 1 / 65536, 0.1, 0.5, 1.0)] == [0, 0, 0, 1, 6554, 32768, 65535]
    # the signed compare is the unsigned "half >= thr16" on halves shifted by 32768: drop probability thr16 / 65536 exactly
    halves = np.arange(65536, dtype=np.uint64)
    for t in C.DROPOUT_THR + [0]:
        kept = R._signed16(halves) >= R._signed16((t - 32768) & 0xFFFF)
        assert int(kept.sum()) == 65536 - t and np.array_equal(kept, ((halves + U64(32768)) % U64(65536)) >= t)


def test_fast_survey_form_equals_pair_bits():
    streams = [0, 0xFFFFFFFF, R.rng_stream(1000004, 8), 123456789]
    for pair0 in (0, 5, 2 ** 21 - 3):
        got = R.stream_halves(streams, pair0, 64).view(np.uint16).astype(np.uint64)
        for k, s in enumerate(streams):
            w = R.pair_bits(s, np.arange(pair0, pair0 + 64))
            want = np.stack([w & U64(0xFFFF), w >> U64(16)], axis=1).reshape(-1)
            assert np.array_equal(got[k], want)
            keep = R.stream_halves([s], pair0, 64)[0] >= np.int16(6554 - 32768)
            assert np.array_equal(keep.astype(np.uint8), R.keep(s, 2 * pair0, 128, 6554))


def test_rho_is_pearson():
    g = np.random.default_rng(5)
    a, b = g.random(4096) < 0.9, g.random(4096) < 0.5
    assert abs(R.rho(a, b) - np.corrcoef(a, b)[0, 1]) < 1e-12
    assert abs(R.rho(a, a) - 1.0) < 1e-12 and abs(R.rho(a, ~a) + 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ the library's host functions
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1] + [7 * 1000003 + k for k in (1, 2, 3, 40)]
SITES = [0, 1, 2, 8, 95, 1000, 1004, 4242, 2 ** 32 - 1]
PROBS = [0.0, 1e-9, 1 / 65536, 0.1, 0.5 - 2.0 ** -17, 0.5, 0.5 + 2.0 ** -16, 0.99999, 1.0]


def _host_lib():
    from msa_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        if not os.path.exists(build.HIPCC):
            pytest.skip("no prebuilt library and no hipcc on this machine")
        build.build(verbose=False)
    return _lib.load()


def test_host_stream_and_threshold_equal_the_reference():
    lib = _host_lib()
    from msa_amd import ops
    for seed in SEEDS:
        for site in SITES:
            want = R.rng_stream(seed, site)
            assert lib.mmbert_rng_stream(seed, site) == want, (seed, site)
            assert ops.rng_stream(seed, site) == want, (seed, site)
    for p in PROBS:
        assert lib.mmbert_dropout_thr16(p) == R.thr16(p), p
    assert [R.thr16(p) for p in PROBS] == [0, 0, 1, 6554, 32768, 32768, 32769, 65535, 65535]


def test_make_drop_scale_is_the_inverse_keep_probability():
    _host_lib()
    from msa_amd import ops
    for p in PROBS:
        stream, t, scale = ops.make_drop(p, 7000022, 8)
        assert t == R.thr16(p), p
        assert scale == 1.0 / (1.0 - t / 65536.0) == R.drop_scale(t), p
        if t:
            assert stream == R.rng_stream(7000022, 8)


# ------------------------------------------------------------------------------------------------ wrong generators
MUTANT_THR = [32767, 32768, 32769, 6554]


def _wrong_keep(kind, stream, idx, t16):
    """``R.keep_at`` with one defect."""
    idx = np.asarray(idx, dtype=np.uint64)
    s16 = R._signed16
    pair = idx >> U64(1)
    if kind == "index truncated to 32 bits before the shift":
        pair = (idx & U64(R.M32)) >> U64(1)
    if kind == "pair index = idx":
        pair = idx
    if kind == "stream xor'ed":
        x = ((pair & U64(R.M32)) * U64(R.WEYL) & U64(R.M32)) ^ U64(stream)
        x = x ^ (x >> U64(16))
        x = (x * U64(R.PAIR_MUL)) & U64(R.M32)
        h = x ^ (x >> U64(16))
    else:
        h = R.pair_bits(stream, pair)
    odd = (idx & U64(1)) == 1
    if kind == "halves swapped":
        odd = ~odd
    half = np.where(odd, h >> U64(16), h & U64(0xFFFF))
    t = (int(t16) - 32768) & 0xFFFF
    if kind == "unsigned compare":
        return (half.astype(np.int64) >= t).astype(np.uint8)
    if kind == "> for >=":
        return (s16(half) > s16(t)).astype(np.uint8)
    return (s16(half) >= s16(t)).astype(np.uint8)


KEEP_MUTANTS = ["halves swapped", "unsigned compare", "> for >=", "index truncated to 32 bits before the shift", "stream xor'ed", "pair index = idx"]


def _rejected(got, want):
    try:
        R.check_equal(got, want, "mutant")
    except AssertionError:
        return True
    return False


def test_unmutated_emulation_passes_the_comparison():
    """The emulation with no defect IS the reference: the comparison accepts it at the cases below (so a rejection is the defect's)."""
    for t in MUTANT_THR:
        for s in C.dropout_streams():
            for n in C.DROPOUT_N[:-1]:
                assert not _rejected(_wrong_keep("", s, np.arange(n), t), R.keep(s, 0, n, t))


@pytest.mark.parametrize("kind", KEEP_MUTANTS)
def test_flat_mask_cases_reject_every_wrong_generator(kind):
    """Each defect at the flat-mask cases of the GPU file, thr16 in {32767, 32768, 32769, 6554}, every stream of the GPU file.  Swapped
    halves, the unsigned compare, the pair index and the XOR'ed stream are rejected at n = 255, 256 and 257 alike (the one, two or
    three flags of the smaller cases can agree by chance), except that a stream XOR'ed in cannot show at stream 0 (x ^ 0 = x + 0) and
    must pass there.  '>' parts from '>=' at one half in 65536: the case n = 2^20 + 1 rejects it (e^-16 that none of its elements
    holds that half), the cases up to 257 cannot.  The truncated index is the same function below 2^32: only the window across
    index 2^32 rejects it."""
    for t in MUTANT_THR:
        for s in C.dropout_streams():
            if kind == "index truncated to 32 bits before the shift":
                idx0, n = C.WINDOW
                assert _rejected(_wrong_keep(kind, s, np.arange(n, dtype=np.uint64) + U64(idx0), t), R.keep(s, idx0, n, t)), (t, s)
                for m in C.DROPOUT_N[:-1]:                                       # ... and nowhere else
                    assert not _rejected(_wrong_keep(kind, s, np.arange(m), t), R.keep(s, 0, m, t))
                continue
            sizes = [2 ** 20 + 1] if kind == "> for >=" else [255, 256, 257]
            for n in sizes:
                assert n in C.DROPOUT_N
                bad = _rejected(_wrong_keep(kind, s, np.arange(n), t), R.keep(s, 0, n, t))
                assert bad == (not (kind == "stream xor'ed" and s == 0)), (kind, t, s, n)


@pytest.mark.parametrize("kind", [k for k in KEEP_MUTANTS if not k.startswith("index truncated")])
def test_attention_mask_cases_reject_every_wrong_generator(kind):
    """The same defects through the attention index scheme at the GPU file's smallest lengths: at S = 5 with 3 heads (75 flags) every
    one of the five bases rejects them; '>' needs the case list's largest masks (S = 130, 12 heads: 2e5 flags per base, the five
    bases together 1e6).  (The truncated index is left out: every index of a layout is below 2^32, where it is the same function --
    the flat window across 2^32 is what rejects it.)"""
    stream = C.dropout_streams()[2]
    for t in MUTANT_THR:
        S, heads = (130, 12) if kind == "> for >=" else (5, 3)
        assert S in C.ATTN_S and heads in C.ATTN_HEADS
        hits = []
        for base in C.attn_bases(S, heads):
            want = R.attn_keep(stream, base, S, heads, t)
            Spad = R.ceil4(S)
            h, i, j = np.meshgrid(np.arange(heads), np.arange(S), np.arange(S), indexing="ij")
            got = _wrong_keep(kind, stream, U64(base) + (h * S * Spad + i * Spad + j).astype(np.uint64), t)
            hits.append(_rejected(got, want))
        assert any(hits) if kind == "> for >=" else all(hits), (kind, t, hits)


def _wrong_mlm(kind, ids, ps, pr, seed, site, special, mask_id):
    ids = np.asarray(ids, dtype=np.int64)
    h = R.pair_bits(R.rng_stream(seed, site), np.arange(ids.size, dtype=np.uint64))
    lo, hi = (h & U64(0xFFFF)).astype(np.int64), (h >> U64(16)).astype(np.int64)
    if kind == "select and replace halves swapped":
        lo, hi = hi, lo
    sp = np.isin(ids, np.asarray(list(special), dtype=np.int64)) if len(special) else np.zeros(ids.size, dtype=bool)
    sel = ~sp & ((lo <= R.mlm_thr(ps)) if kind == "<= for < (select)" else (lo < R.mlm_thr(ps)))
    rep = (hi <= R.mlm_thr(pr)) if kind == "<= for < (replace)" else (hi < R.mlm_thr(pr))
    return np.where(sel & rep, np.int64(mask_id), ids), np.where(sel, ids, -100)


@pytest.mark.parametrize("kind", ["select and replace halves swapped", "<= for < (select)", "<= for < (replace)"])
def test_mlm_cases_reject_every_wrong_generator(kind):
    """Swapped halves show at the GPU file's n = 255 (p_select 0.15, p_replace 0.8).  '<=' parts from '<' at the one half equal to the
    threshold: the GPU file's two boundary cases are built to contain it (a seed searched with the reference), and each rejects
    the defect on its side."""
    rejected = []
    for case in C.mlm_cases():
        ids, kw = case["ids"], case["kw"]
        want = R.mlm_mask(ids, **kw)
        assert not _rejected(np.stack(_wrong_mlm("", ids, **_mlm_args(kw))), np.stack(want))
        if _rejected(np.stack(_wrong_mlm(kind, ids, **_mlm_args(kw))), np.stack(want)):
            rejected.append(case["name"])
    assert rejected, kind
    if kind == "select and replace halves swapped":
        assert any(name.startswith("n255-") for name in rejected)
    else:
        assert rejected == ["boundary-select" if "select" in kind else "boundary-replace"], rejected


def _mlm_args(kw):
    return dict(ps=kw["p_select"], pr=kw["p_replace"], seed=kw["seed"], site=kw["site"], special=kw["special_ids"], mask_id=kw["mask_id"])


def test_mlm_reference_semantics():
    """What the kernel comment promises, on the reference: labels = the original id exactly at the selected elements, special ids never
    selected, ids rewritten only where selected and replaced, p_replace = 1.0 (threshold 65536) replaces every selected element."""
    g = np.random.default_rng(3)
    ids = g.integers(95, 110, size=3200)
    out, lab = R.mlm_mask(ids, 0.15, 1.0, 9, 4242, (101, 102), 103)
    sel = lab != -100
    assert 0.10 < sel.mean() < 0.20 and np.array_equal(lab[sel], ids[sel]) and not np.isin(ids[sel], (101, 102)).any()
    assert (out[sel] == 103).all() and np.array_equal(out[~sel], ids[~sel])
    out0, lab0 = R.mlm_mask(ids, 1.0, 0.0, 9, 4242, (), 103)
    assert np.array_equal(lab0, ids) and np.array_equal(out0, ids)


# ------------------------------------------------------------------------------------------------ the mask read-back, emulated
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_readback_decodes_the_emulated_kernels_exactly(p):
    """tests/attention_ref.emulate (the kernels' documented roundings: bf16 P, bf16 dropped P, bf16 outputs) on the read-back inputs at
    the GPU file's lengths with a masked tail: the decoded flags ARE the masks fed in, along keys (ctx), along queries (dV) and, on the second
    set of inputs, from dQ; one flipped flag is seen in all three."""
    lens, heads = [5, 65, 257, 130], 3
    t16 = R.thr16(p)
    stream = R.rng_stream(7000022, 8)
    bases, _ = R.seq_elem_bases(lens, heads)
    masks = [R.attn_keep(stream, b, S, heads, t16) for b, S in zip(bases, lens)]
    live = [np.ones(S, dtype=bool) for S in lens]
    live[2][200:] = False
    live[3][129:] = False
    qkv, dctx = C.readback_inputs(lens, heads)
    bias = torch.from_numpy(np.concatenate([np.where(l, 0.0, A.MASKED) for l in live])).float()
    for flip in (False, True):
        fed = [m.copy() for m in masks]
        if flip:
            fed[2][1, 100, 131] ^= 1
        out = A.emulate(torch.from_numpy(qkv).to(torch.bfloat16), bias, lens, heads, [torch.from_numpy(m) for m in fed], R.drop_scale(t16),
                        torch.from_numpy(dctx).to(torch.bfloat16))
        qkv2, dctx2 = C.readback_inputs_dq(lens, heads)
        out2 = A.emulate(torch.from_numpy(qkv2).to(torch.bfloat16), bias, lens, heads, [torch.from_numpy(m) for m in fed], R.drop_scale(t16),
                         torch.from_numpy(dctx2).to(torch.bfloat16))
        s0 = 0
        same = True
        for s, S in enumerate(lens):
            for h in range(heads):
                want = masks[s][h] * live[s][None, :]
                cols = slice(64 * h, 64 * h + 64)
                got_f = C.decode_ctx(out["ctx"][s0:s0 + S, cols].numpy(), live[s], R.drop_scale(t16), f"ctx {s} {h}")
                got_b = C.decode_dv(out["dv"][s0:s0 + S, cols].numpy(), live[s], R.drop_scale(t16), f"dv {s} {h}")
                got_q = C.decode_dq(out2["dq"][s0:s0 + S, cols].numpy(), out2["ctx"][s0:s0 + S, 64 * h].numpy(), live[s], R.drop_scale(t16), f"dq {s} {h}")
                bad = _rejected(got_f, want), _rejected(got_b, want), _rejected(got_q, want)
                assert bad[0] == bad[1] == bad[2] == (flip and (s, h) == (2, 1)), (s, h, bad)
                same = same and not any(bad)
            s0 += S
        assert same == (not flip)


# ------------------------------------------------------------------------------------------------ the stream-pair survey
BOUND = 2e-3                          # test_kernels_gpu.test_dropout_hash_pairwise_keep_correlations: "Independent bits give |rho| ~ 1 / sqrt(n) ...; bound 2e-3"
N_ELEMS = 1 << 22
SURVEY_P = (0.1, 0.5)
JOINT_SEGMENTS = 3                    # the pretraining step's passes (text, text + pair, text + pair): sites 1001 + k
SEED_BASES = (1, 2, 3, 4, 5, 6)
CONSECUTIVE = 40


def model_sites():
    """The site numbers of the model's own make_drop calls: every ``make_drop(p, seed, <site>)`` in msa_amd/model.py, its site expression
    evaluated over the configured layer count (``i``) and the joint segments (``k``)."""
    from msa_amd.model import MMBertConfig
    layers = MMBertConfig().num_hidden_layers
    tree = ast.parse(open(os.path.join(ROOT, "msa_amd", "model.py")).read())
    exprs = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "make_drop":
            assert len(node.args) == 3
            exprs.add(ast.unparse(node.args[2]))
    sites = set()
    for e in sorted(exprs):
        names = {n.id for n in ast.walk(ast.parse(e, mode="eval")) if isinstance(n, ast.Name)}
        assert names <= {"i", "k"}, e
        for i in (range(layers) if "i" in names else [0]):
            for k in (range(JOINT_SEGMENTS) if "k" in names else [0]):
                sites.add(int(eval(e, {"__builtins__": {}}, {"i": i, "k": k})))
    return sorted(sites)


def model_seed(base, call):
    """The seed of forward call ``call`` (1, 2, ...) after manual_seed(base), as the model's own _next_seed forms it."""
    from msa_amd.model import _GpuModelBase
    st = types.SimpleNamespace(_seed=base, _calls=call - 1)
    return _GpuModelBase._next_seed(st)


def test_model_sites_are_the_ones_the_issue_lists():
    sites = model_sites()
    assert sites == sorted([8 * i + j for i in range(12) for j in range(3)] + [1000, 1001, 1002, 1003])
    assert model_seed(3, 1) == 3 * 1000003 + 1 and model_seed(3, 2) == 3 * 1000003 + 2


def _packed_keeps(halves_of_chunk, nstreams):
    """Per p: packed keep bits [nstreams, N_ELEMS / 8] from a function chunk -> int16 halves [nstreams, elements of the chunk]."""
    chunk_pairs = 1 << 14
    out = [np.empty((nstreams, N_ELEMS // 8), dtype=np.uint8) for _ in SURVEY_P]
    for c in range(N_ELEMS // 2 // chunk_pairs):
        hv = halves_of_chunk(c * chunk_pairs, chunk_pairs)
        lo = c * chunk_pairs * 2 // 8
        for o, p in zip(out, SURVEY_P):
            o[:, lo:lo + chunk_pairs * 2 // 8] = np.packbits(hv >= np.int16(R.thr16(p) - 32768), axis=1)
    return out


def _pair_rhos(bits, adjacent):
    """|rho| of every pair of rows (``adjacent``: of rows k, k + 1 only) of packed 0/1 rows: {(a, b): rho}."""
    w = bits.view(np.uint64)
    ones = np.bitwise_count(w).sum(1, dtype=np.int64)
    res = {}
    for a in range(w.shape[0] - 1):
        others = w[a + 1:a + 2] if adjacent else w[a + 1:]
        both = np.bitwise_count(others & w[a]).sum(1, dtype=np.int64)
        r = R.rho_counts(N_ELEMS, ones[a], ones[a + 1:a + 1 + len(both)], both)
        for k, v in enumerate(r):
            res[(a, a + 1 + k)] = float(v)
    return res


def _survey(make_rows):
    """``make_rows(group, labels)`` -> a halves-of-chunk function for the group's streams.  Returns {(what, p, a, b): rho} over (1) every
    pair of the model's sites under each of six seeds, (2) every site under 40 consecutive seeds, neighbours in that order."""
    sites = model_sites()
    res = {}
    groups = [("sites of seed %d" % model_seed(b, 1), [(model_seed(b, 1), s) for s in sites], False) for b in SEED_BASES]
    groups += [("site %d, consecutive seeds" % s, [(model_seed(0x5EED, c), s) for c in range(1, CONSECUTIVE + 1)], True) for s in sites]
    for what, members, adjacent in groups:
        packed = _packed_keeps(make_rows(members), len(members))
        for p, bits in zip(SURVEY_P, packed):
            for (a, b), r in _pair_rhos(bits, adjacent).items():
                res[(what, p, members[a], members[b])] = r
    return res


class SurveyExceeds(AssertionError):
    pass


@pytest.mark.xfail(strict=True, raises=SurveyExceeds, reason="stream pairs above the project's |rho| bound: see the docstring and DESIGN.md")
def test_stream_pair_survey_meets_the_projects_bound():
    """Pearson correlation of the keep flags of two streams at the same index, 2^22 elements, p in {0.1, 0.5}, on the reference alone
    (tests/test_rng_gpu.py proves the device bit-equal to it), bound |rho| <= 2e-3 -- the independence bound the project wrote down in
    test_kernels_gpu.test_dropout_hash_pairwise_keep_correlations, which looks at ONE pair (seed 12345, sites 77 / 78).  Here:

      (1) every pair of the model's 40 sites (model_sites(): 8 i + 0..2 for 12 layers, 1000, 1001 + k) under each of six seeds
          (_next_seed's first call after manual_seed(1 .. 6)): 6 x 780 pairs per p;
      (2) every site against itself under the 40 consecutive seeds of calls 1 .. 40 (default model seed), each call against the NEXT
          one: 40 x 39 pairs per p.  (All 780 pairs of the 40 calls would be 31 200 per p: at sigma = 2^-11 the bound is 4.1 sigma and
          an IDEAL generator exceeds it about 1.3 times in 31 200 draws, so the count is kept where the statistic can meet the bound.)

    Control, asserted first and not covered by the expected failure: the same counts of pairs and elements from numpy's default_rng:
    12 480 pairs, largest |rho| 0.00183.

    MEASURED, the generator as it is (one xorshift-multiply-xorshift round on counter + stream, so rho depends on the stream
    difference alone and a fixed fraction of differences is bad):

      part (1)   p 0.1:  45 of 4680 above 2e-3, worst 0.0075 (seed 6000019, sites 41 / 72);   p 0.5: 188 of 4680, worst 0.0189
                 (seed 3000010, sites 0 / 42)
      part (2)   p 0.1:  17 of 1560, worst 0.0090 (site 9, seeds 24301072913 / ...914);          p 0.5:  67 of 1560, worst 0.0086

    317 of 12 480 in all.

    WHAT THE SURVEY DOES NOT MEASURE: the same site 2 .. 39 calls apart (part (2) takes neighbouring calls only), and different
    sites under different seeds.  A derivation tuned to pass it can be bad exactly there (it was, below).

    TRIED ON THE HOST (tools/rng_lattice_search.py, nothing shipped): streams on a lattice over call and site,
    hash32(high word of seed + ...) + ((low word of seed) * 40 + index(site)) * C, so that every pair measured here differs by
    k * C, k = 1 .. 40.  Of 240 random odd C, 49 keep all 40 multiples at or below 2e-3 against one base stream (13 below 1.5e-3).
    The full survey under the three best: 3, 12 and 6 of 12 480 pairs above the bound, worst 0.0023, 0.0027, 0.0024 -- at the noise
    level of the statistic (control 0.0018), none passes.  The same three at what the survey does not measure: 4, 3 and 5 of the 38
    differences of the same site 2 .. 39 calls apart above the bound (worst 0.0077), and 5, 8, 4 of 120 sampled multiples up to 1600
    (worst 0.011): the rate of arbitrary differences.  So a wider search might turn this test green while leaving calls 2 .. 39
    apart as they are; widen the survey's part (2) (with more elements, for the statistic's sake) before shipping one.
    Until something meets the bound this is a strict expected failure: it turns into an error the day the survey passes, and the
    bound is not to be loosened."""
    def generator_rows(members):
        streams = [R.rng_stream(seed, site) for seed, site in members]
        return lambda pair0, npairs: R.stream_halves(streams, pair0, npairs)

    g = np.random.default_rng(2024)

    def control_rows(members):
        return lambda pair0, npairs: g.integers(-32768, 32768, size=(len(members), 2 * npairs), dtype=np.int16)

    control = _survey(control_rows)
    worst_c = max(control.items(), key=lambda kv: abs(kv[1]))
    print(f"control: {len(control)} pairs, largest |rho| {abs(worst_c[1]):.5f}")
    assert abs(worst_c[1]) <= BOUND, ("the control itself exceeds the bound", worst_c)
    got = _survey(generator_rows)
    assert len(got) == len(control) == 2 * (len(SEED_BASES) * 780 + 40 * (CONSECUTIVE - 1))
    over = {k: v for k, v in got.items() if not abs(v) <= BOUND}
    for part in ("sites of seed", "consecutive"):
        for p in SURVEY_P:
            sub = {k: v for k, v in got.items() if part in k[0] and k[1] == p}
            sub_over = sorted(((abs(v), k) for k, v in sub.items() if not abs(v) <= BOUND), reverse=True)
            print(f"{part}, p {p}: {len(sub_over)} of {len(sub)} pairs above {BOUND}; worst {sub_over[:2]}")
    if over:
        worst = max(over.items(), key=lambda kv: abs(kv[1]))
        raise SurveyExceeds(f"{len(over)} of {len(got)} stream pairs above |rho| = {BOUND}; worst {worst}")
