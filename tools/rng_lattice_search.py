"""CPU: search for a host-side derivation of the dropout streams that meets the stream-pair survey of
tests/test_rng_reference_cpu.py (|rho| <= 2e-3 at 2^22 elements, p in {0.1, 0.5}).  Runs on the integer reference alone.

The correlation between the masks of two streams depends on their difference only, so the candidate puts the streams a model can
draw close together on a lattice:

    stream(seed, site) = hash32(high word of seed + 0x7F4A7C15) + ((low word of seed) * 40 + index(site)) * C        (mod 2^32)

(index = position among the model's 40 sites; _next_seed's consecutive calls differ by 1 in the low word).  Every pair the survey
measures then differs by k * C with k = 1 .. 40.  For random odd C this prints

  1. how many candidates keep all of k = 1 .. 40 at or below the bound against one base stream, and the best of them;
  2. for the best ones: the full survey (_survey of the test file) under the candidate derivation;
  3. what the survey does NOT measure: the same site 2 .. 39 calls apart (k = 40 a) and a sample of k up to 1600 (any site pair up
     to 39 calls apart).

    python tools/rng_lattice_search.py [candidates = 240] [full surveys = 3]

Results of the run recorded in DESIGN.md (seed 77, 240 candidates): 49 candidates pass step 1 (13 stay below 1.5e-3); the three best
give 3, 12 and 6 of 12480 survey pairs above the bound (worst 0.0023, 0.0027, 0.0024) against 317 (worst 0.0189) for the hashed
derivation; step 3: 4, 3, 5 of the 38 call distances and 5, 8, 4 of 120 sampled multiples above the bound (worst 0.011)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import rng_ref as R                          # noqa: E402
from tests import test_rng_reference_cpu as T           # noqa: E402

BASE = 0x12345678


def abs_rho_of_multiples(C, ks, base=BASE):
    """[p, k]: |rho| between the masks of stream ``base`` and of base + k * C."""
    streams = [base] + [(base + k * C) & R.M32 for k in ks]
    packed = T._packed_keeps(lambda pair0, npairs: R.stream_halves(streams, pair0, npairs), len(streams))
    out = []
    for bits in packed:
        w = bits.view(np.uint64)
        ones = np.bitwise_count(w).sum(1, dtype=np.int64)
        both = np.bitwise_count(w[1:] & w[0]).sum(1, dtype=np.int64)
        out.append(np.abs(R.rho_counts(T.N_ELEMS, ones[0], ones[1:], both)))
    return np.stack(out)


def lattice_rows(C):
    index = {s: i for i, s in enumerate(T.model_sites())}

    def stream(seed, site):
        base = int(R.hash32(((seed >> 32) + 0x7F4A7C15) & R.M32))
        return (base + ((seed & R.M32) * len(index) + index[site]) * C) & R.M32

    def rows(members):
        streams = [stream(seed, site) for seed, site in members]
        return lambda pair0, npairs: R.stream_halves(streams, pair0, npairs)
    return rows


def main():
    ncand = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    nfull = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    g = np.random.default_rng(77)
    res = []
    for _ in range(ncand):
        C = int(g.integers(0, 2 ** 32)) | 1
        res.append((float(abs_rho_of_multiples(C, range(1, 41)).max()), C))
    res.sort()
    print(f"{ncand} candidates; k = 1..40 all <= {T.BOUND}: {sum(m <= T.BOUND for m, _ in res)}; <= 1.5e-3: {sum(m <= 1.5e-3 for m, _ in res)}")
    for m, C in res[:8]:
        print(f"  {C:#010x}  max |rho| {m:.5f}")
    for _, C in res[:nfull]:
        got = T._survey(lattice_rows(C))
        over = sorted(((abs(v), k) for k, v in got.items() if abs(v) > T.BOUND), reverse=True)
        print(f"{C:#010x}: survey {len(over)} of {len(got)} pairs above {T.BOUND}; worst {over[:2]}")
        r = abs_rho_of_multiples(C, [40 * a for a in range(2, 40)])
        print(f"  same site 2..39 calls apart: {int((r > T.BOUND).any(0).sum())} of 38 above; worst {float(r.max()):.5f}")
        ks = list(range(41, 1600, 13))
        r = abs_rho_of_multiples(C, ks)
        print(f"  sampled k in 41..1599: {int((r > T.BOUND).any(0).sum())} of {len(ks)} above; worst {float(r.max()):.5f}")


if __name__ == "__main__":
    main()
