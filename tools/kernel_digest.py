"""Per-kernel digests of a HIP source's device code, for "this refactor moved no instruction" (no GPU needed).

    python tools/kernel_digest.py msa_amd/csrc/layernorm.hip [more.hip ...]  >  after.txt
    python tools/kernel_digest.py --compare before.txt after.txt

Compiles each source to assembly with the product's flags (as tools/scan_serialized_loads.py does) and prints one line per kernel
symbol: a digest of its instructions, a digest of its .amdhsa_kernel descriptor block (registers, LDS, scratch), the instruction
count and the demangled name.  Assembler comments are stripped and the per-file function number in .LBB<n>_ labels is normalised, so a
kernel keeps its digests when it moves inside a file or to another file.  --compare matches two such tables by demangled name and lists
what differs and what is on one side only; it exits 1 unless every kernel of the first table is equal in the second."""
import hashlib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msa_amd.build import HIPCC, FLAGS  # noqa: E402


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def digest_source(path):
    """{kernel symbol: (instruction digest, descriptor digest, instruction count)} of one source."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC, *[f for f in FLAGS if f != "-fPIC"], "-S", "--cuda-device-only", path, "-o", out], check=True)
        text = open(out).read()
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    lines = [re.sub(r"\s+", " ", l.split(";")[0]).strip() for l in text.split("\n")]
    body, desc, cur, where = {}, {}, None, None
    for l in lines:
        m = re.match(r"^(\w+):$", l)
        if m and not l.startswith(".L"):
            cur, where = m.group(1), "body"
            body[cur] = []
        elif l.startswith(".amdhsa_kernel "):
            cur, where = l.split()[1], "desc"
            desc[cur] = []
        elif l.startswith((".Lfunc_end", ".end_amdhsa_kernel")):
            where = None
        elif l and where == "body" and not l.startswith((".p2align", ".cfi")):
            body[cur].append(l)
        elif l and where == "desc":
            desc[cur].append(l)
    return {k: (_sha(body[k]), _sha(d), sum(1 for l in body[k] if not l.endswith(":"))) for k, d in desc.items()}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def read_table(path):
    rows = [l.rstrip("\n").split(None, 4) for l in open(path) if l.strip() and not l.startswith("#")]
    return {r[4]: (r[1], r[2]) for r in rows}


if __name__ == "__main__":
    if len(sys.argv) < 2 or (sys.argv[1] == "--compare" and len(sys.argv) != 4):
        sys.exit(__doc__)
    if sys.argv[1] == "--compare":
        a, b = read_table(sys.argv[2]), read_table(sys.argv[3])
        differ = [k for k in a if k in b and a[k] != b[k]]
        print(f"# {len(a)} kernels before, {len(b)} after, {sum(1 for k in a if b.get(k) == a[k])} equal in both digests")
        for tag, ks in (("DIFFERS", differ), ("ONLY BEFORE", [k for k in a if k not in b]), ("ONLY AFTER", [k for k in b if k not in a])):
            for k in sorted(ks):
                print(f"# {tag}: {k}")
        sys.exit(0 if all(b.get(k) == a[k] for k in a) else 1)
    for path in sys.argv[1:]:
        table = digest_source(path)
        names = demangle(list(table))
        for k in sorted(table, key=lambda k: names[k]):
            print(f"{os.path.basename(path):14s} {table[k][0]} {table[k][1]} {table[k][2]:5d} {names[k]}")
