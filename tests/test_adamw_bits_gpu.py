"""The stored bits of every AdamW route, pinned: SHA-256 of the raw bytes of p, g, m, v, the bf16 copy and (where there is one) the weight
average after one call, against digests recorded with the library of the commit BEFORE the four kernels came to share one update body
(its four copies of the update, compiled under -ffast-math).  No tolerance: the shared body names every FMA, the hardware square root and
the reciprocal so that it computes that commit's dataflow, and a digest that moves means the arithmetic is no longer pinned to it -- mend
the body, never the digests.  (The cross-kernel tests of test_adamw_groups_gpu / test_adamw_ema_gpu hold the routes to each other on the
ragged 4099-block grid; this file holds them to the recorded past on the smallest launches: 1 block = one wave, 5 blocks = two workgroups,
the second ragged.)

``python -m tests.test_adamw_bits_gpu`` prints the table below from whatever library the package loads: that is how it was recorded.
"""
import hashlib
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_adamw_groups_gpu import HYPER7, _random_state

DEV = "cuda"
SEED = {1: 5009, 5: 5006}                 # _random_state's flags: [1] and [0, 2, 1, 5, 0] (checked below)
GSCALE, DECAY = 0.37, 0.999
ROUTES = ("adamw", "adamw_devscale", "grouped host scale", "grouped device scale", "ema no map host scale", "ema map device scale")
CASES = list(itertools.product((1, 5), (0, 1), (1, 7), (True, False)))      # blocks, mode, step, zero_grad


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _digests(nblk, mode, step, zero_grad):
    """{route: digest of (p, g, m, v, bf16 copy[, ema]) after one call on the same seeded state}"""
    from msa_amd import ops
    p0, g0, m0, v0, flags, rng = _random_state(nblk, SEED[nblk])
    gmap = torch.from_numpy(rng.integers(0, len(HYPER7), nblk).astype(np.uint8)).to(DEV)
    coef = torch.tensor([GSCALE], device=DEV)
    lr, b1, b2, eps, wd = HYPER7[0]
    one = dict(lr=lr, beta1=b1, beta2=b2, eps=eps, wd=wd)
    kw = dict(step=step, mode=mode, zero_grad=zero_grad)
    out = {}
    for route in ROUTES:
        p, g, m, v = p0.clone(), g0.clone(), m0.clone(), v0.clone()
        pb = torch.zeros_like(p, dtype=torch.bfloat16)
        ema = (p0 * 0.5).contiguous() if route.startswith("ema") else None
        if route == "adamw":
            ops.adamw(p, g, m, v, pb, flags, gscale=GSCALE, **one, **kw)
        elif route == "adamw_devscale":
            ops.adamw_devscale(p, g, m, v, pb, flags, coef, **one, **kw)
        elif route == "grouped host scale":
            ops.adamw_grouped(p, g, m, v, pb, flags, gmap, HYPER7, gscale=GSCALE, **kw)
        elif route == "grouped device scale":
            ops.adamw_grouped(p, g, m, v, pb, flags, gmap, HYPER7, coef=coef, **kw)
        elif route == "ema no map host scale":
            ops.adamw_ema(p, g, m, v, pb, flags, None, [HYPER7[0]], ema, ema_decay=DECAY, gscale=GSCALE, **kw)
        else:
            ops.adamw_ema(p, g, m, v, pb, flags, gmap, HYPER7, ema, ema_decay=DECAY, coef=coef, **kw)
        torch.cuda.synchronize()
        out[route] = _sha(p, g, m, v, pb, *([] if ema is None else [ema]))
    return out


# Recorded with the parent commit's library (the four copied kernels), built in a worktree of that commit, by this file's print mode.
RECORDED = {
    (1, 0, 1, True): ("74613b3ac399f5d48b6cd2b5ccf22fe260f3721d1ba055edfa79f02c54df3174",
        "74613b3ac399f5d48b6cd2b5ccf22fe260f3721d1ba055edfa79f02c54df3174",
        "74f3730d61ac4b3c675c28807f8202d9c714d0bcce147d4040c8eeaf4c3a64bb",
        "74f3730d61ac4b3c675c28807f8202d9c714d0bcce147d4040c8eeaf4c3a64bb",
        "3bf2a3bc838b8fad513326b3c365ded98bda88c7290684dc33af8aa88e2a9f77",
        "99453b2d5fe09b7d835ba5647dc11da6602bf13ea57802301f0c24f2e5b70c00"),
    (1, 0, 1, False): ("076601748556a97020fa8528a603368513ff815bbf541455f77e3cc5bf159e83",
        "076601748556a97020fa8528a603368513ff815bbf541455f77e3cc5bf159e83",
        "f2b48896bd6b959a79a870006d6bb18c928530ae64a0396bc46f4c7ac88e264b",
        "f2b48896bd6b959a79a870006d6bb18c928530ae64a0396bc46f4c7ac88e264b",
        "b02180e621bedf38c1a6a7443b6196950eff0b9469d1435c453c23bb2d1f7067",
        "10d5f4e481fdc9e0d9b27d767f4a98ebb1f410c0bd30b852c16a8d646249655e"),
    (1, 0, 7, True): ("ef1bf44dee3745ab91c49c425f1ef7d2e92c942677c1a59e59a24b36444e19df",
        "ef1bf44dee3745ab91c49c425f1ef7d2e92c942677c1a59e59a24b36444e19df",
        "667ffd06bd1d837ee543c94b8729c3ba8841686f225d2073c574a7b23372250d",
        "667ffd06bd1d837ee543c94b8729c3ba8841686f225d2073c574a7b23372250d",
        "00a9fd437e265bbd9cc163c0bfe9b2a065cff65d9fa5dbacf018a30978970dd3",
        "55fec8a910546d7f77c6ccf696ef5a31e8355efa4ecd69a8e53deb8caa12542d"),
    (1, 0, 7, False): ("48815851ea373c1b3423eb5a92a7f823082eee7d88502b143ddb939bdc5d0bad",
        "48815851ea373c1b3423eb5a92a7f823082eee7d88502b143ddb939bdc5d0bad",
        "f679261019a1dabcd879937036e0ca40cf4879d15c1a4b2aaad8f213e9743f8f",
        "f679261019a1dabcd879937036e0ca40cf4879d15c1a4b2aaad8f213e9743f8f",
        "59542ca9e44aa84b996cbd298430f83cdfc49c6fec63e68acf6af76e2f2dbe1b",
        "3e4e042092ad339d61b57b018358163712cf50e7a5eb78b010399506d503d886"),
    (1, 1, 1, True): ("0e84f016a9aa09dc2f582e3fc6e65964f2b9d699bd2ce62c076f3f18e91f137d",
        "0e84f016a9aa09dc2f582e3fc6e65964f2b9d699bd2ce62c076f3f18e91f137d",
        "7e02a0263109732074a7b231ba972042cc96e52ce20220ae77201a8c5a4994d3",
        "7e02a0263109732074a7b231ba972042cc96e52ce20220ae77201a8c5a4994d3",
        "c77ffd63b1fb5aaacd09a8ad1f3e0641d2c170b7696d2fc975f02324f7841f97",
        "321b1152bf87709684d523839d215ea2c4ab70c659e7a069a6448cae1b6ad21e"),
    (1, 1, 1, False): ("9d43103757cfe956715372ee88689b95fb8741f540f4ee3bc06cd32a0f1c10a4",
        "9d43103757cfe956715372ee88689b95fb8741f540f4ee3bc06cd32a0f1c10a4",
        "514f47a2fbbbd2071abf165db45745ab47f059e7383aa158e16d3acbfdbc1a0b",
        "514f47a2fbbbd2071abf165db45745ab47f059e7383aa158e16d3acbfdbc1a0b",
        "d5ef4b2badaf556564c6363735fd7cc9caa4a0c97d50550f2d1e782d2244e57d",
        "66dd88f51818a79db3d0df015c89b4316ba8f214636129e4f4cc8aa0ebaaad6a"),
    (1, 1, 7, True): ("baca5720701b2358c30f5850a7294dd829e6d4f8a35e67c7c869fa4a0f577f59",
        "baca5720701b2358c30f5850a7294dd829e6d4f8a35e67c7c869fa4a0f577f59",
        "9b21b995eb50161a9f7c8e95974175cdd37bf70975d9b0ded3df3d9feb5989ef",
        "9b21b995eb50161a9f7c8e95974175cdd37bf70975d9b0ded3df3d9feb5989ef",
        "3601d9ac6fcc075a0a407e9b0ab8cea8f1f58e65822ab66111882a8935b3ed93",
        "cd038f398f8998edc0cf4f185bde9b236be7c41f76308ebbdbd67125bdfcb78b"),
    (1, 1, 7, False): ("0c355ce24c3e3e0fd17fe2dd31e3471495c593a067448df9330868ba0816768d",
        "0c355ce24c3e3e0fd17fe2dd31e3471495c593a067448df9330868ba0816768d",
        "29b7660a1132d302547fcc60d0b2986f131b49fd5b670ec2e253c534e98f34f3",
        "29b7660a1132d302547fcc60d0b2986f131b49fd5b670ec2e253c534e98f34f3",
        "9eb4257c43c548524928c48d8ec687c11b0c2d2471f32130d88a48e24e446add",
        "0102b9c409ea240bfb6cbaca7f214d8cccd8a9d302de7305024e2d784df93f76"),
    (5, 0, 1, True): ("6846efa4de4ba064a96d8eed71c15eea691fbd1bcc6575d4dff2e1a421ff20ee",
        "6846efa4de4ba064a96d8eed71c15eea691fbd1bcc6575d4dff2e1a421ff20ee",
        "e6adbb77119d8ef67961352ff2bb7717417cabf74d332464375a4e1b547eba89",
        "e6adbb77119d8ef67961352ff2bb7717417cabf74d332464375a4e1b547eba89",
        "b793ccb329314897da3276a3685ec95a0d8640b9171cf413c8959d2189fbc832",
        "660463a7de71e71d963d6c66e46acb2223473f79e0001a2a0f50be7526e58023"),
    (5, 0, 1, False): ("a70f4c87a779a9107903c4152c19504d5fccd47b37c1c90ac9c38daf4f38b4ab",
        "a70f4c87a779a9107903c4152c19504d5fccd47b37c1c90ac9c38daf4f38b4ab",
        "b2b086633dae70b408cc5f05b114d2b56fed0bbb63e8a55b29349b43482b35a0",
        "b2b086633dae70b408cc5f05b114d2b56fed0bbb63e8a55b29349b43482b35a0",
        "d7e1e0c9c5ce75b9a18161e32d9aef4f1a12bdd176926ea8f45699ab49250bd7",
        "eb267c9c08c1f725391c30bbff30d3a7f852b7ff8ba0f18dbc10cbe0f273d427"),
    (5, 0, 7, True): ("e66c386060b47684fa2abe1e88fa9906bee365f7b1ebe7a814372486c458c882",
        "e66c386060b47684fa2abe1e88fa9906bee365f7b1ebe7a814372486c458c882",
        "e8b242ec44396407505b50b7aeed7770cfb5f995afe46038f61b1817bcf36cf5",
        "e8b242ec44396407505b50b7aeed7770cfb5f995afe46038f61b1817bcf36cf5",
        "bd749511ef55f57681d5b62544d92e5ee892c9b316dcfb94611019afb1d76994",
        "130dee854120d0d47180f20934f055f3e68799c91bda97161fcb130b767ebc06"),
    (5, 0, 7, False): ("356473cc3a47f65401995ed243be7b4fbe1753b377d3f49086c1e4daf051300a",
        "356473cc3a47f65401995ed243be7b4fbe1753b377d3f49086c1e4daf051300a",
        "9cc2d137df107d7023e10b0dbfa64cb7cf0683e85628c2fa7c0f7209484b6955",
        "9cc2d137df107d7023e10b0dbfa64cb7cf0683e85628c2fa7c0f7209484b6955",
        "bb2c6de321f471c91a77217352da0c29eb5efff9b5e9a41210d4372c244d0653",
        "a5cba9b4c0e74aa838da037aa9725d8d4d981b73604dbe529f20a6fe2f710a5f"),
    (5, 1, 1, True): ("004d9b1c043e4cef2e6db93a1396d21f1f29284e4b395c6d6263c244ec947e0e",
        "004d9b1c043e4cef2e6db93a1396d21f1f29284e4b395c6d6263c244ec947e0e",
        "b654787bbddf92b3433069c24fb1836fbc9e943e0bd1c5fe3b3168408be87228",
        "b654787bbddf92b3433069c24fb1836fbc9e943e0bd1c5fe3b3168408be87228",
        "2da819365b8a091090f7ed98e3e76f3c3a1093667f7b9af6c8423b960005aac8",
        "c073e0e74e51aca0048cd60898cf3edadcbe55507d5caaa22623cb273a92c455"),
    (5, 1, 1, False): ("c57baa64b3c735de4badfadae6f591a8bebdf5f6a506abe4311bec35c75e9980",
        "c57baa64b3c735de4badfadae6f591a8bebdf5f6a506abe4311bec35c75e9980",
        "41821053fe8c48273e3651dbc4daa0ad11b7f5414975f61bd1d7fd12e899975c",
        "41821053fe8c48273e3651dbc4daa0ad11b7f5414975f61bd1d7fd12e899975c",
        "88c299c7c24cdb115f50af42730f92b69862cdef1a4545378bc6e533677c8a0c",
        "f8c86824ccefc9a091ebfda4982572095656057c11189e07c7dd259fadb3a9ae"),
    (5, 1, 7, True): ("11100f16f7682b5b78ec4f8f69ec58d1bd0307ec0e67a161bc8c8fd3b4d9c28a",
        "11100f16f7682b5b78ec4f8f69ec58d1bd0307ec0e67a161bc8c8fd3b4d9c28a",
        "6ef9f6adf46b361d33bf372d5fbee21d1a67325dd602110f08daa81bd80452c6",
        "6ef9f6adf46b361d33bf372d5fbee21d1a67325dd602110f08daa81bd80452c6",
        "d958ebe09fad23d83d4800220f97588f025034a28721b8b373438d79db4a0384",
        "600167f5bcf7e42ab92bef63b3f08072a23a81daf18132cb74d41606d587ef74"),
    (5, 1, 7, False): ("efe44306e2dfa75366faaa740d97e7a0a5601d414ebe7f77303b78597735bcc7",
        "efe44306e2dfa75366faaa740d97e7a0a5601d414ebe7f77303b78597735bcc7",
        "e89f7fff4c5f0dfc1481534f35acc47caf51e7ac2e80f2e2d542bff5484126c0",
        "e89f7fff4c5f0dfc1481534f35acc47caf51e7ac2e80f2e2d542bff5484126c0",
        "8a9c53f4619747f1f3a10b6d0808ff67d4dc078cc69555fae0697ca00be648aa",
        "79e79caa93f5c3a71b376b3c37118880ff23e37954d82a4bcf3b63190fdc4c92"),
}


def test_the_states_cover_every_flag():
    assert [int(x) for x in _random_state(1, SEED[1])[4].cpu()] == [1]
    assert [int(x) for x in _random_state(5, SEED[5])[4].cpu()] == [0, 2, 1, 5, 0]           # 0, 1, 2 and a lazy (+4) block


@pytest.mark.parametrize("nblk,mode,step,zero_grad", CASES)
def test_stored_bits_are_the_recorded_ones(nblk, mode, step, zero_grad):
    got = _digests(nblk, mode, step, zero_grad)
    for route in ROUTES:
        print(nblk, mode, step, zero_grad, route, got[route])
    want = dict(zip(ROUTES, RECORDED[nblk, mode, step, zero_grad]))
    assert got == want, [r for r in ROUTES if got[r] != want[r]]


if __name__ == "__main__":
    for case in CASES:
        d = _digests(*case)
        print(f"    {case}: (" + ",\n        ".join(f'"{d[r]}"' for r in ROUTES) + "),")
