"""GPU tests of global gradient-norm clipping: the norm kernel (mmbert_grad_norm) against float64 at odd segment edges, the
torch-semantics drop-in (optim.clip_grad_norm_) and the fused form (AdamW.clip_grad_norm_ + step) against
torch.nn.utils.clip_grad_norm_, lazily zeroed and accumulated gradients, no host sync, data parallelism, and the trainer."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import mmbert_oracle as O
from msa_amd.data import synthetic_batch, batch_to

DEV = "cuda"
CFG = dict(hidden=128, layers=2, heads=2, intermediate=512, vocab=4096, dataset="mosei", alpha=1.0, beta=1.0)


def build(cfg=CFG, dropout=0.0):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                     intermediate_size=cfg["intermediate"], hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings(cfg["dataset"])
    m.bert.jointEmbeddings.dropout_prob = dropout if dropout == 0.0 else 0.5
    m.load_state_dict(O.seeded_params(cfg), strict=False)
    return m.to(DEV)


def _batch(seed, cfg=CFG):
    return batch_to(synthetic_batch(2, 16, 40, 24, vocab=cfg["vocab"], seed=seed), DEV)


def _fb(m, b):
    out, _ = m(**b)
    out[0].mean().backward()


def _optimizer(m, lr=1e-3):
    from msa_amd import trainer as T
    opt, sched = T.build_optimizer(m, T.default_args(learning_rate=lr), 10)
    for g in opt.param_groups:
        g["lr"] = lr
    return opt, sched


def _seg_norm64(g, segs, gscale=1.0):
    """float64 L2 norm of gscale * g over the (offset, length) segments (g on any device)."""
    x = g.detach().double().cpu().numpy()
    return float(np.sqrt(sum(float(np.dot(x[o:o + k], x[o:o + k])) for o, k in segs))) * abs(gscale)


def _torch_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient from an fp32 norm tensor"""
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)


@pytest.fixture
def deterministic():
    from msa_amd import ops
    lib = ops._lib.load()
    was = lib.mmbert_get_deterministic()
    yield lambda on: lib.mmbert_set_deterministic(1 if on else 0)
    lib.mmbert_set_deterministic(was)


def _random_segments(n, rng):
    """every other interval between random cut points of [0, n): unaligned offsets and lengths, the first segment from 0"""
    if n <= 4:
        return [(0, n)]
    k = min(int(rng.integers(3, 24)), n - 1)
    b = [0, *sorted(int(c) for c in rng.choice(np.arange(1, n), size=k, replace=False)), n]
    return [(b[i], b[i + 1] - b[i]) for i in range(0, len(b) - 1, 2)]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 10 ** 6, 119 * 10 ** 6])
def test_grad_norm_kernel_against_float64(n, deterministic):
    from msa_amd import ops
    rng = np.random.default_rng(n % 9973)
    g = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(n % 1009)) * 0.01
    segs = _random_segments(n, rng)
    assert any(o % 4 or k % 4 for o, k in segs) or n < 4
    st = torch.tensor(segs, dtype=torch.int64, device=DEV)
    base = _seg_norm64(g, segs)
    x = g.cpu().numpy()
    amax = max(float(np.abs(x[o:o + k]).max()) for o, k in segs if k > 0)
    del x
    for gscale in (1.0, 0.5, 0.37):
        ref2 = base * gscale
        for max_norm in (ref2 * 0.25, ref2 * 4.0):
            out = ops.grad_norm(g, st, len(segs), max_norm=max_norm, norm_type=2.0, gscale=gscale)
            assert abs(float(out[0]) - ref2) <= 1e-6 * ref2, (n, gscale, float(out[0]), ref2)
            c = float(_torch_coef(out[0:1], max_norm))                      # (on the device, as torch's clip forms it)
            assert abs(float(out[1]) - c) <= 2.0 ** -23 * c, (float(out[1]), c)    # (torch's device reciprocal: within one ulp of IEEE)
            assert float(out[2]) == np.float32(float(out[1]) * gscale)
            assert (float(out[1]) < 1.0) == (max_norm < ref2)
        outi = ops.grad_norm(g, st, len(segs), max_norm=1.0, norm_type=math.inf, gscale=gscale)
        assert float(outi[0]) == np.float32(amax * gscale), (n, gscale, float(outi[0]), amax * gscale)
    # bit-identical run to run, deterministic mode on and off (there is no float atomic to order)
    outs = []
    for det in (False, True, False):
        deterministic(det)
        outs += [ops.grad_norm(g, st, len(segs), max_norm=1.0).clone() for _ in range(2)]
    assert all(torch.equal(o, outs[0]) for o in outs)


def test_grad_norm_kernel_zero_inf_nan_match_torch():
    from msa_amd import ops
    n = 1031
    segs = [(1, 500), (503, 527)]
    st = torch.tensor(segs, dtype=torch.int64, device=DEV)
    z = torch.zeros(n, device=DEV)
    z[0] = z[501] = z[502] = 7.0                                        # outside the segments: never read into the norm
    out = ops.grad_norm(z, st, 2, max_norm=1.0).cpu()
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0 and float(out[2]) == 1.0
    base = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    for bad in (math.inf, -math.inf, math.nan):
        g = base.clone()
        g[700] = bad
        g[502] = math.nan                                               # a NaN between the segments changes nothing
        for norm_type in (2.0, math.inf):
            out = ops.grad_norm(g, st, 2, max_norm=1.0, norm_type=norm_type)
            p = torch.nn.Parameter(torch.zeros(n - 3, device=DEV))
            p.grad = torch.cat([g[1:501], g[503:]]).clone()
            tn = torch.nn.utils.clip_grad_norm_([p], 1.0, norm_type=norm_type)
            assert torch.equal(out[0:1], tn.reshape(1)) or (math.isnan(float(out[0])) and math.isnan(float(tn)))
            c = _torch_coef(tn.reshape(1), 1.0)
            assert torch.equal(out[1:2], c) or (math.isnan(float(out[1])) and math.isnan(float(c)))
    # torch.ops.mmbert.grad_norm: the same kernel behind the operator namespace
    import msa_amd.torch_ops  # noqa: F401
    r = torch.ops.mmbert.grad_norm(base, st, 1.0, 2.0, 0.5).cpu()
    assert torch.equal(r, ops.grad_norm(base, st, 2, max_norm=1.0, gscale=0.5).cpu())
    with pytest.raises(RuntimeError):
        ops.grad_norm(base, st, 2, max_norm=1.0, norm_type=1.0)        # the C entry point rejects other norms


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the drop-in against torch on the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_clip_on_clones(named, max_norm):
    clones = []
    for _, p in named:
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = p.grad.detach().clone()
        clones.append(q)
    n = torch.nn.utils.clip_grad_norm_(clones, max_norm)
    return n, [q.grad for q in clones]


@pytest.mark.parametrize("subset", [False, True])
def test_drop_in_equals_torch_clip_on_the_model(subset):
    from msa_amd import optim
    m = build(dropout=0.1)
    m.train()
    m.manual_seed(3)
    _fb(m, _batch(41))
    named = [(n, p) for n, p in m.named_parameters() if p.grad is not None and (not subset or n.startswith("bert.encoder."))]
    full = torch.cat([p.grad.reshape(-1) for _, p in named]).double().norm()
    saved = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    for frac in (0.3, 3.0):
        for n, p in m.named_parameters():
            if n in saved:
                p.grad.copy_(saved[n])
        max_norm = float(full) * frac
        tn, tgrads = _torch_clip_on_clones(named, max_norm)
        got = optim.clip_grad_norm_([p for _, p in named], max_norm)
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
        assert abs(float(got) - float(tn)) <= 1e-5 * float(tn), (float(got), float(tn))
        for (n, p), tg in zip(named, tgrads):
            assert torch.allclose(p.grad, tg, rtol=1e-5, atol=1e-9), n
        if frac > 1.0:
            assert all(torch.equal(p.grad, saved[n]) for n, p in named)          # coefficient 1: untouched
        if subset:                                                               # parameters outside the subset are not written
            inside = {n for n, _ in named}
            assert all(torch.equal(p.grad, saved[n]) for n, p in m.named_parameters() if n in saved and n not in inside)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the fused path against torch's clip + a plain step
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_models_with_the_same_gradients():
    ms = [build() for _ in range(3)]
    for m in ms:
        m.eval()
        m._ensure_ready(torch.device(DEV, 0))
    _fb(ms[0], _batch(51))
    for m in ms[1:]:
        _fb(m, _batch(51))
        m._flat.grads.copy_(ms[0]._flat.grads)                                  # (the same bits: fp32 atomics aside)
    return ms


@pytest.mark.parametrize("frac", [0.2, 5.0])
def test_fused_clip_equals_torch_clip_then_plain_step(frac):
    from msa_amd.flat import FROZEN
    m1, m2, m3 = _three_models_with_the_same_gradients()
    o1, o2, o3 = (_optimizer(m)[0] for m in (m1, m2, m3))
    named = [(n, p) for n, p in m2.named_parameters() if p.grad is not None and not n.startswith(FROZEN)]
    norm = float(torch.cat([p.grad.reshape(-1) for _, p in named]).double().norm())
    max_norm = norm * frac
    g_before = m1._flat.grads.clone()
    n1 = o1.clip_grad_norm_(max_norm)
    assert torch.equal(m1._flat.grads, g_before)                                  # .grad is not modified by the fused form
    assert abs(float(n1) - norm) <= 1e-5 * norm
    o1.step()
    torch.nn.utils.clip_grad_norm_([p for _, p in named], max_norm)
    o2.step()
    o3.step()                                                                     # no clipping at all
    for a, b in ((m1._flat.params, m2._flat.params), (o1._m, o2._m), (o1._v, o2._v), (m1._flat.half.float(), m2._flat.half.float())):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-12)
    if frac > 1.0:                                                                # coefficient 1: bit-identical to the unclipped step
        for a, b in ((m1._flat.params, m3._flat.params), (o1._m, o3._m), (o1._v, o3._v), (m1._flat.half, m3._flat.half)):
            assert torch.equal(a, b)
    else:
        assert not torch.equal(o1._m, o3._m)


def test_fused_clip_is_consumed_by_step_and_dropped_by_zero_grad():
    m1, m2, _ = _three_models_with_the_same_gradients()
    o1, o2 = _optimizer(m1)[0], _optimizer(m2)[0]
    o1.clip_grad_norm_(1e-6)                                                      # a clip no step applies ...
    o1.zero_grad()                                                                # ... is dropped with the gradients
    assert o1._clip is None
    for m in (m1, m2):
        _fb(m, _batch(52))
    m1._flat.grads.copy_(m2._flat.grads)
    o1.clip_grad_norm_(1e-6)
    o1.clip_grad_norm_(1e30)                                                      # a second clip replaces the first
    o1.step()
    o2.step()
    assert torch.equal(m1._flat.params, m2._flat.params) and torch.equal(o1._m, o2._m) and o1._clip is None


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. lazily zeroed and accumulated gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def test_clip_reads_dropped_gradients_as_zero_and_accumulated_ones_as_their_sum():
    from msa_amd import model as MM
    from msa_amd.flat import FROZEN
    m = build()
    m.eval()
    opt, _ = _optimizer(m, lr=0.0)                                                # parameters never move: references stay valid
    m._ensure_ready(torch.device(DEV, 0))
    flat = m._flat
    b0, b1, b2 = _batch(60), _batch(61), _batch(62)
    nolabel = dict(b2)
    nolabel["masked_labels"] = tuple(torch.full_like(x, -100) for x in nolabel["masked_labels"])
    first = torch.randn(6, CFG["hidden"], device=DEV, generator=torch.Generator(DEV).manual_seed(7)).requires_grad_(True)

    def heads_only():
        hl, *_ = MM._HeadsFn.apply(first, m, torch.tensor([0, 1, 1, 0], device=DEV), torch.tensor([0.5, -1.0], device=DEV))
        hl.backward()
    ref = {}
    for k, fn in (("b0", lambda: _fb(m, b0)), ("b1", lambda: _fb(m, b1)), ("nolabel", lambda: _fb(m, nolabel)), ("heads", heads_only)):
        flat.grads.zero_()
        fn()
        ref[k] = flat.grads.clone()
    opt._bind()
    st, ns = flat.segments(opt._names, FROZEN)
    segs = [tuple(s) for s in st[:ns].tolist()]
    close = lambda got, want: abs(float(got) - want) <= 1e-5 * want

    opt.step(); opt.zero_grad()
    _fb(m, nolabel)
    assert close(opt.clip_grad_norm_(1.0), _seg_norm64(ref["nolabel"], segs))
    opt.step(); opt.zero_grad()
    heads_only()                                                                  # the encoder's dropped gradients are never written
    assert flat.stale
    assert close(opt.clip_grad_norm_(1.0), _seg_norm64(ref["heads"], segs))
    opt.step(); opt.zero_grad()
    _fb(m, b0); _fb(m, b1)
    assert close(opt.clip_grad_norm_(1.0), _seg_norm64(ref["b0"] + ref["b1"], segs))
    opt.step(); opt.zero_grad()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. no host sync
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fused_clip_and_step_do_not_sync_with_the_host():
    from msa_amd import optim
    m = build()
    m.eval()
    opt, _ = _optimizer(m)
    _fb(m, _batch(70))
    optim.clip_grad_norm_(m.parameters(), 1e30)                                   # (first use: bind, segment lists, workspace)
    opt.clip_grad_norm_(1.0); opt.step(); opt.zero_grad()
    _fb(m, _batch(71))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n = opt.clip_grad_norm_(0.5)
        opt.step()
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert math.isfinite(float(n)) and float(n) > 0.0
    _fb(m, _batch(72))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        optim.clip_grad_norm_(m.parameters(), 0.5)
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. data parallelism
# ---------------------------------------------------------------------------------------------------------------------------------
def _dp_clip_worker(rank, world, port, q, max_norm):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)         # 1-GPU box: both ranks share cuda:0, gloo moves the bytes
    try:
        from msa_amd import optim, parallel
        torch.cuda.set_device(0)
        m = build()
        opt, _ = _optimizer(m)
        dp = parallel.DataParallel(m, opt, bucket_mb=0.25)
        m.eval()
        _fb(m, _batch(10 + rank))
        dp.finish_backward()
        drop_in = optim.clip_grad_norm_(m.parameters(), 1e30)            # coefficient 1: .grad unchanged
        fused = opt.clip_grad_norm_(max_norm)
        opt.step()
        torch.cuda.synchronize()
        q.put(dict(rank=rank, drop_in=float(drop_in), fused=float(fused), params=m._flat.params.cpu().numpy(), scale=m._flat.grad_scale))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_data_parallel_clip_measures_the_mean_gradient():
    from msa_amd.flat import FROZEN
    # single-process reference: the two shards' gradients, averaged
    m = build()
    m.eval()
    m._ensure_ready(torch.device(DEV, 0))
    total = None
    for r in range(2):
        m._flat.grads.zero_()
        _fb(m, _batch(10 + r))
        total = m._flat.grads.clone() if total is None else total + m._flat.grads
    opt, _ = _optimizer(m)
    opt._bind()
    st, ns = m._flat.segments(opt._names, FROZEN)
    ref = _seg_norm64(total * 0.5, [tuple(s) for s in st[:ns].tolist()])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_dp_clip_worker, args=(r, 2, port, q, ref * 0.3)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda d: d["rank"])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in res:
        assert r["scale"] == 0.5
        assert abs(r["fused"] - ref) <= 1e-4 * ref and abs(r["drop_in"] - ref) <= 1e-4 * ref, (r["fused"], r["drop_in"], ref)
    assert np.array_equal(res[0]["params"], res[1]["params"])                     # the clipped step leaves the ranks equal


def _rccl_world1_clip_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    from msa_amd import parallel
    try:
        rank, local, world = parallel.init_from_env(force=True)                     # RCCL with world_size 1, before any GPU call
        assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
        norms = []
        for use_dp in (False, True):
            m = build()
            m.eval()
            opt, _ = _optimizer(m)
            dp = parallel.DataParallel(m, opt, bucket_mb=0.25) if use_dp else None
            _fb(m, _batch(80))
            if dp is not None:
                dp.finish_backward()
            norms.append(float(opt.clip_grad_norm_(1.0)))
            opt.step()
        torch.cuda.synchronize()
        q.put(("ok", norms))
    except Exception as e:                                                          # report, do not hang the parent
        q.put(("error", repr(e)))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_data_parallel_over_rccl_world1_clip_equals_plain():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    p = ctx.Process(target=_rccl_world1_clip_worker, args=(port, q))
    p.start()
    status, norms = q.get(timeout=600)
    p.join(120)
    assert status == "ok", norms
    assert p.exitcode == 0
    plain, wrapped = norms
    assert abs(plain - wrapped) <= 1e-4 * plain, norms


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_train_epoch_with_max_grad_norm(deterministic):
    from msa_amd import trainer as T
    deterministic(True)                                                             # two runs of one loop must give the same bits
    batches = [_batch(90 + i) for i in range(2)]

    def run(max_grad_norm="absent", hand=False):
        m = build()
        kw = {} if max_grad_norm == "absent" else dict(max_grad_norm=max_grad_norm)
        args = T.default_args(train_batch_size=2, learning_rate=1e-3, **kw)
        opt, sched = T.build_optimizer(m, args, 2)
        if not hand:
            T.train_epoch(args, m, None, opt, sched, device=DEV, quirk_step=False, batches=batches)
        else:                                                                       # torch's clip on .grad, then the plain step
            m.train()
            for b in batches:
                _fb(m, b)
                torch.nn.utils.clip_grad_norm_(m.parameters(), max_grad_norm)
                opt.step()
                sched.step()
                opt.zero_grad()
        assert opt._steps == 2
        return m._flat.params.clone(), opt._m.clone(), opt._v.clone()

    plain = run()
    for a, b in zip(plain, run(1e9)):
        assert torch.equal(a, b)                                                    # clipping that never bites changes no bit
    m0 = build()
    m0.train()
    _fb(m0, batches[0])
    small = 0.1 * float(torch.nn.utils.clip_grad_norm_([p for p in m0.parameters() if p.grad is not None], 1e30))
    got, want = run(small), run(small, hand=True)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-12)
    assert not torch.equal(got[1], plain[1])
