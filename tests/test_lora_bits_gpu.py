"""The stored bits of the adapter kernels (csrc/lora.hip), pinned: SHA-256 of the raw bytes of every output of one call through
ops.lora_qkv_fwd / _bwd and ops.lora_dense_fwd / _bwd, against digests recorded with the library of the commit BEFORE the two seam families
came to share one token-sum kernel, one fold, one set of staging helpers and one eight-column update (its 22 instantiations, the Q | K | V
token sums walking the column axis inside the workgroup).  No tolerance: the shared kernels keep each caller's work partition, row-lane
count and order of every fp32 addition, and a digest that moves means they no longer do -- mend the kernel, never the table.

Per case and input dropout (off, and p = 0.5 through the _drop entry points) the digests are, in order: forward (qkv or y, h, aux where
there is one); backward reading forward's h (dres or dx, every gA, every gB, accumulated onto seeded non-zero gradients); backward with h
recomputed; and, for the dense seams under dropout, backward with h recomputed on a permuted int32 row list.  The shapes are the smallest
at which each shared path can go wrong (the table beside each case); inputs from tests/lora_ref.inputs and tests/lora_dense_ref.inputs, the
dropout triples fixed here, so that no library call shapes an input.

``python -m tests.test_lora_bits_gpu`` prints the table below from whatever library the package loads (MMBERT_LIB_PATH names another
build): RECORDED was printed that way from a build of the parent commit's checkout and pasted here.
"""
import hashlib

import pytest
import torch

from tests import lora_dense_ref as DR
from tests import lora_ref as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"
IN_DROP = (0x2545F491, 32768, 2.0)                               # (stream, thr16, 1 / (1 - thr16 / 65536)): p = 0.5 on the adapters' input
OUT_DROP = (0x9E3779B9, 6554, 65536.0 / (65536 - 6554))          # the GEMM's own output mask (p = 0.1) on an ADD seam
Q, K, V = LR.TARGETS
QKV_CASES = {
    "q 65x128 r4": ((Q,), 65, 128, 4),                           # one row past a workgroup; one slab
    "qv 257x768 r8": ((Q, V), 257, 768, 8),                      # three slabs, ragged last; the model's width; two row lanes
    "qkv 257x768 r16": ((Q, K, V), 257, 768, 16),                # staged operands past 64 KiB (the LDS opt-in); six streams
    "qv 257x1088 r8": ((Q, V), 257, 1088, 8),                    # 136 column lanes: above the dense cap, below QKV's; one row lane
    "q 130x2112 r4": ((Q,), 130, 2112, 4),                       # 264 column groups: two column blocks at col_lanes = 256
}
DENSE_CASES = {                                                  # M, K, N, r, mode, the GEMM's dropout, gelu_u in backward
    "add+drop 65x128->832 r4": (65, 128, 832, 4, DR.ADD, OUT_DROP, False),      # N crosses one staging chunk; unequal stream widths
    "gelu 257x768->3072 r8": (257, 768, 3072, 8, DR.GELU, None, False),         # with aux; three column blocks at col_lanes = 128
    "add+gelu_u 257x3072->768 r16": (257, 3072, 768, 16, DR.ADD, None, True),   # four K chunks; the widest stream is dA
    "add 257x1088->64 r8": (257, 1088, 64, 8, DR.ADD, None, False),             # K = one chunk + 320; the narrower stream returns early in block 1
}
CASES = [(name, p) for name in (*QKV_CASES, *DENSE_CASES) for p in (0.0, 0.5)]


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _dev(t):
    return t.to(DEV)


def _qkv_digests(names, M, H, r, ind):
    from msa_amd import ops
    inp = LR.inputs(M, H, r, names, "real", seed=M + H + r)
    x, dqkv, dres = _dev(inp["x"]), _dev(inp["dqkv"]), _dev(inp["dres"])
    A = {t: _dev(inp["A"][t]) for t in names}
    B = {t: _dev(inp["B"][t]) for t in names}
    s, kw = 16.0 / r, ({} if ind is None else {"in_drop": ind})
    qkv = _dev(inp["qkv"])
    h = torch.empty((M, len(names) * r), dtype=torch.bfloat16, device=DEV)
    ops.lora_qkv_fwd(x, qkv, A, B, names, s, h_out=h, **kw)
    out = [_sha(qkv, h)]
    for saved in (h, None):
        gA = {t: _dev(inp["gA0"][t]) for t in names}
        gB = {t: _dev(inp["gB0"][t]) for t in names}
        d = ops.lora_qkv_bwd(dqkv, x, saved, A, B, gA, gB, names, s, dres=dres, **kw)
        out.append(_sha(d, *[gA[t] for t in names], *[gB[t] for t in names]))
    return tuple(out)


def _dense_digests(M, K, N, r, mode, out_drop, with_u, ind):
    from msa_amd import ops
    inp = DR.inputs(M, K, N, r, "real", seed=M + K + N + r)
    x, dy, A, B = _dev(inp["x"]), _dev(inp["dy"]), _dev(inp["A"]), _dev(inp["B"])
    u = _dev(inp["u"]) if with_u else None
    s, kw = 16.0 / r, ({} if ind is None else {"in_drop": ind})
    y = _dev(inp["y"])
    aux = torch.empty_like(y) if mode == DR.GELU else None
    h = torch.empty((M, r), dtype=torch.bfloat16, device=DEV)
    ops.lora_dense_fwd(x, y, A, B, s, mode=mode, drop=out_drop, aux=aux, h_out=h, **kw)
    out = [_sha(y, h, *([] if aux is None else [aux]))]
    forms = [(h, None), (None, None)]
    if ind is not None:                                          # gathered operands: local row i draws the mask of site row rows[i]
        forms.append((None, torch.randperm(M, generator=torch.Generator().manual_seed(M)).to(torch.int32).to(DEV)))
    for saved, rows in forms:
        dx, gA, gB = _dev(inp["dx"]), _dev(inp["gA0"]), _dev(inp["gB0"])
        ops.lora_dense_bwd(dy, x, saved, A, B, gA, gB, s, dx=dx, gelu_u=u, rows=rows, **kw)
        out.append(_sha(dx, gA, gB))
    return tuple(out)


def _digests(name, p):
    ind = IN_DROP if p else None
    got = _qkv_digests(*QKV_CASES[name], ind) if name in QKV_CASES else _dense_digests(*DENSE_CASES[name], ind)
    torch.cuda.synchronize()
    return got


# Recorded with the parent commit's library (the two copied kernel families), built in a checkout of that commit, by this file's print mode.
RECORDED = {
    ('q 65x128 r4', 0.0): ("fb5359a917daf6c92df2b657bdaa4ed71e8ede0aa4bba5ec25359b50a0cc5938",
        "c3d357848320c80026ba612f46a2477599a8c0eea2b428150bf0b2081bf806c3",
        "c3d357848320c80026ba612f46a2477599a8c0eea2b428150bf0b2081bf806c3"),
    ('q 65x128 r4', 0.5): ("d042f61ec14b4def197d9f98d57e38810c1841f2e2b53d62d3cafc9b65bc07f8",
        "da939820baaccf73219fb70dd2872101d64b45eaf19f384b1c6baa30ed8a0ed1",
        "da939820baaccf73219fb70dd2872101d64b45eaf19f384b1c6baa30ed8a0ed1"),
    ('qv 257x768 r8', 0.0): ("21447bfb7ef7fdb7a981c8724495612de8ecf6a264f50652398d26671ef136b2",
        "ae8f99b532d84d0e789bc548f1ed83de7f480be6472efae5f4cefc3ace91bef7",
        "ae8f99b532d84d0e789bc548f1ed83de7f480be6472efae5f4cefc3ace91bef7"),
    ('qv 257x768 r8', 0.5): ("900d1de1f4153750c96892dc43712dca2d83a5780280d4f4ac207b08e9d812b9",
        "98bfa2d457ee3da00684e73f2156c87b510d29d24a9b8c099ee03fa36e5de208",
        "98bfa2d457ee3da00684e73f2156c87b510d29d24a9b8c099ee03fa36e5de208"),
    ('qkv 257x768 r16', 0.0): ("5cf48f590e35814468c1e6cdf7eeb12b77c949a838bc956a8f54474821bb7674",
        "2db4f96086c964d6d49799b94d9db8217d15a18eeb77a04bb3d8aaed3d3d0c54",
        "2db4f96086c964d6d49799b94d9db8217d15a18eeb77a04bb3d8aaed3d3d0c54"),
    ('qkv 257x768 r16', 0.5): ("47c6b122b9c2a6a2e9e398143336d471a516b79994dfe46b771215ffa2a7d51e",
        "8ef0e8f14e66dd98f5b67726eda7bc25ad499262fceab19d82e6976b813676fd",
        "8ef0e8f14e66dd98f5b67726eda7bc25ad499262fceab19d82e6976b813676fd"),
    ('qv 257x1088 r8', 0.0): ("d86dcd17af4d9afd52bb63d12c625da62eca2fb8b6664ff62ac9fb52ed95bd85",
        "656fcacec96b343fcb2b29172516ff1cddb3cb65af1ca24e2589a6845bf30946",
        "656fcacec96b343fcb2b29172516ff1cddb3cb65af1ca24e2589a6845bf30946"),
    ('qv 257x1088 r8', 0.5): ("5fab78162f2f05bab73b125387860a4dda4e973c99b73976d79ab287c3eb831a",
        "2bd7a2fa27cee6967917fd929427aa0ca64b9cf6bc0f693363b9f537800edb31",
        "2bd7a2fa27cee6967917fd929427aa0ca64b9cf6bc0f693363b9f537800edb31"),
    ('q 130x2112 r4', 0.0): ("376d748b002ae20611c827b05bcea3acb6a6803151f7e795ee372c590b708909",
        "d0eb5a49ce60224de0e345f870286c734c61f1e666d6f39d60a0abf67aa8aa5a",
        "d0eb5a49ce60224de0e345f870286c734c61f1e666d6f39d60a0abf67aa8aa5a"),
    ('q 130x2112 r4', 0.5): ("2b50c84561464e0847a956a95832d8250254f21050209049e7af14554ae6ae64",
        "7391496a60957c6c853dabe545357fa74e0f646734878ad2a0a871ce65bd3b98",
        "7391496a60957c6c853dabe545357fa74e0f646734878ad2a0a871ce65bd3b98"),
    ('add+drop 65x128->832 r4', 0.0): ("9485e32ce250e10604a2f3ec3efbdf43e007f9ecd0060ee76727bafe317bd705",
        "dd68cdd1a72dbd6bc329c63fd4c5405a3cb4b83046b16e944621f4b45e51d4cc",
        "dd68cdd1a72dbd6bc329c63fd4c5405a3cb4b83046b16e944621f4b45e51d4cc"),
    ('add+drop 65x128->832 r4', 0.5): ("615e4b07b27f90546df879e316f6c6bf1f9e6c19700fb2adc126a2057266068f",
        "284567f1feaa854d318045a0cb9f527b51c520f23c5c64597e414a50df41eb6b",
        "284567f1feaa854d318045a0cb9f527b51c520f23c5c64597e414a50df41eb6b",
        "0bc181e42b1c0f19afc2bde00769fd22d9e6221e7516433ede85eeebac368890"),
    ('gelu 257x768->3072 r8', 0.0): ("69a5a4c13eb0a944c11e39aa4e247b90a273f152c4efd8faf04789290645845a",
        "f4ed1f94c1fe272c9b2a315ed902533f33373748acf1665917199831b616cd07",
        "f4ed1f94c1fe272c9b2a315ed902533f33373748acf1665917199831b616cd07"),
    ('gelu 257x768->3072 r8', 0.5): ("581a04e3141974c388fdd929d5f2041bc6546c43befc0a18878442e2b2370c1a",
        "eed6a666bffe1b82d3699dee6b1eb8559c671570b70fa49e0d3221bc8659feb8",
        "eed6a666bffe1b82d3699dee6b1eb8559c671570b70fa49e0d3221bc8659feb8",
        "ecdbee1c73fabc894fccb89d229efded9c124ee3317074ee43cd5548611d0688"),
    ('add+gelu_u 257x3072->768 r16', 0.0): ("a48ca5ccec9d6318ae450f56136a7eb1e9603ebdfe050602246ebc50f893bfe3",
        "7145587d5db5f30497eab9321aa1014d1ecac0825c8c63f80cdc552a3a850991",
        "7145587d5db5f30497eab9321aa1014d1ecac0825c8c63f80cdc552a3a850991"),
    ('add+gelu_u 257x3072->768 r16', 0.5): ("97da33343e8d9bd5b92d665db273f63070dccf1dded8ffa92819cbc2923d7217",
        "fc12608da0c8bd70e74a75a3fa177fa19eb18682ea4a50a887c228b2e96b8eac",
        "fc12608da0c8bd70e74a75a3fa177fa19eb18682ea4a50a887c228b2e96b8eac",
        "ee339aa6133d93b0c2c98e21ae25377397cc754da6c0149970b2264e88167406"),
    ('add 257x1088->64 r8', 0.0): ("54eb0303a10f6992070536c4da644319a5932ba2e54c7f907bbb718ca877fba5",
        "83483ac17385d34d5909fce0916a6b4bff39d1ecb0aab42fe043dda4092caba2",
        "83483ac17385d34d5909fce0916a6b4bff39d1ecb0aab42fe043dda4092caba2"),
    ('add 257x1088->64 r8', 0.5): ("de4aecc47bf2cced493525f4ae2430d0d9c37326f0f465f9e77e2a7dbedf4600",
        "a1ab80d3de8aad6c150dea0eb24bb57ca2b41648f79717714816bd645b46d7f5",
        "a1ab80d3de8aad6c150dea0eb24bb57ca2b41648f79717714816bd645b46d7f5",
        "88bc8e7925a4f5f4fbca82c45d223fc61b708ed6aa86fc28fdfa1a7b20e64634"),
}


@pytest.mark.parametrize("name,p", CASES)
def test_stored_bits_are_the_recorded_ones(name, p):
    got = _digests(name, p)
    for d in got:
        print(name, p, d)
    assert got == RECORDED[name, p], [i for i, (a, b) in enumerate(zip(got, RECORDED[name, p])) if a != b]


if __name__ == "__main__":
    for case in CASES:
        print(f"    {case!r}: (" + ",\n        ".join(f'"{d}"' for d in _digests(*case)) + "),")
