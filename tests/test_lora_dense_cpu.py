"""CPU tests of the adapters on attention.output.dense / intermediate.dense / output.dense: model.add_lora's new targets and
its bookkeeping, merge, the adapter file, freeze.trainable_plan with the new names, trainer.apply_lora / build_optimizer, the C ABI's
declarations.  tests/test_lora_cpu.py keeps holding the Q / K / V side."""
import math
import os
import re
import types

import pytest
import torch

from msa_amd import freeze as F

L, H, I = 4, 128, 512
BASE = ("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder.")
ALL = ("query", "key", "value", "attention_output", "intermediate", "ffn_output")
PATH = {"query": "attention.self.query", "key": "attention.self.key", "value": "attention.self.value",
        "attention_output": "attention.output.dense", "intermediate": "intermediate.dense", "ffn_output": "output.dense"}
KN = {"query": (H, H), "key": (H, H), "value": (H, H), "attention_output": (H, H), "intermediate": (H, I), "ffn_output": (I, H)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(intermediate=I):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=512, hidden_size=H, num_hidden_layers=L, num_attention_heads=2, intermediate_size=intermediate)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings("mosei")
    return m


def _adapters(m):
    return [n for n, _ in m.named_parameters() if ".lora_" in n]


def _key(i, t, x):
    return f"bert.encoder.layer.{i}.{PATH[t]}.lora_{x}"


def test_new_targets_register_parameters_on_their_own_projections():
    m = _model()
    keys = set(m.state_dict())
    assert m.add_lora(r=8, alpha=16.0, targets=("ffn_output", "query", "intermediate", "attention_output"), seed=3) is m
    names = ("query", "attention_output", "intermediate", "ffn_output")
    ad = _adapters(m)
    assert sorted(ad) == sorted(_key(i, t, x) for i in range(L) for t in names for x in "AB")
    named = dict(m.named_parameters())
    for i in range(L):
        for t in names:
            K, N = KN[t]
            a, b = named[_key(i, t, "A")], named[_key(i, t, "B")]
            assert tuple(a.shape) == (8, K) and tuple(b.shape) == (N, 8) and a.requires_grad and b.requires_grad
            assert not bool(b.any())
            # kaiming_uniform_(a = sqrt 5) on [r, K]: U(+-1 / sqrt K), K the projection's own fan-in (I for ffn_output)
            assert float(a.detach().abs().max()) <= 1.0 / math.sqrt(K) and float(a.detach().std()) > 0.5 / math.sqrt(K), (t, K)
            lin = m.bert.encoder.layer[i]
            for part in PATH[t].split("."):
                lin = getattr(lin, part)
            assert lin.lora_A is a and lin.lora_B is b and tuple(lin.weight.shape) == (N, K)
    for n, p in named.items():
        if ".lora_" not in n:
            assert p.requires_grad == (not n.startswith(BASE)), n
    # exactly the four keys, targets in the canonical order whatever order they were given in; the dict goes back in as keyword arguments
    assert m._lora == dict(r=8, alpha=16.0, targets=names, layers=(0, 1, 2, 3)) and m._flat is None
    assert set(m.state_dict()) == keys | set(ad)
    again = _model().add_lora(**m._lora)
    assert again._lora == m._lora


def test_all_linear_and_the_canonical_order():
    from msa_amd import ops
    m = _model().add_lora(r=4, targets="all-linear", layers=[1])
    assert m._lora["targets"] == ALL and len(_adapters(m)) == 12
    assert ops.LORA_TARGETS == ("query", "key", "value") and ops.LORA_DENSE_TARGETS == ("attention_output", "intermediate", "ffn_output")
    assert ops.lora_mask(("value", "query")) == 5                         # the Q | K | V ABI's mask keeps its meaning
    with pytest.raises(ValueError):
        ops.lora_mask(("attention_output",))
    assert ops.lora_split_targets("all-linear") == (ops.LORA_TARGETS, ops.LORA_DENSE_TARGETS)
    assert ops.lora_split_targets(("ffn_output", "value")) == (("value",), ("ffn_output",))
    assert [ops.lora_dense_dims(t, H, I) for t in ops.LORA_DENSE_TARGETS] == [(H, H), (H, I), (I, H)]


def test_seeding_keeps_the_existing_qkv_draws():
    """One generator, a fixed order: first query / key / value over the layers (what a seed always gave), then the dense targets over the
    layers.  Adding dense targets to a call leaves the Q / K / V matrices of that seed as they were."""
    old = _model().add_lora(r=8, targets=("query", "value"), seed=3).state_dict()
    new = _model().add_lora(r=8, targets=("query", "value", "intermediate", "ffn_output"), seed=3).state_dict()
    for i in range(L):
        for t in ("query", "value"):
            assert torch.equal(old[_key(i, t, "A")], new[_key(i, t, "A")]), (i, t)
    # the QKV draws are what the generator gives first, in layer order
    g = torch.Generator().manual_seed(3)
    b = 1.0 / math.sqrt(H)
    for i in range(L):
        for t in ("query", "value"):
            want = torch.empty((8, H)).uniform_(-b, b, generator=g)
            assert torch.equal(new[_key(i, t, "A")], want), (i, t)
    for i in range(L):                                                      # ... and the dense ones follow, in layer order
        for t in ("intermediate", "ffn_output"):
            K = KN[t][0]
            want = torch.empty((8, K)).uniform_(-1.0 / math.sqrt(K), 1.0 / math.sqrt(K), generator=g)
            assert torch.equal(new[_key(i, t, "A")], want), (i, t)
    other = _model().add_lora(r=8, targets=("intermediate",), seed=4).state_dict()
    same = _model().add_lora(r=8, targets=("intermediate",), seed=4).state_dict()
    k = _key(2, "intermediate", "A")
    assert torch.equal(other[k], same[k]) and not torch.equal(other[k], _model().add_lora(r=8, targets=("intermediate",), seed=5).state_dict()[k])


def test_bad_names_raise_and_leave_the_model_untouched():
    m = _model()
    for kw in (dict(targets=("output",)), dict(targets="output"), dict(targets=("attention_output", "output")), dict(targets=("dense",)),
               dict(targets=("ffn_output", "ffn_output")), dict(targets="all"), dict(targets=("all-linear",)), dict(targets=()),
               dict(targets=("intermediate",), r=3), dict(targets=("intermediate",), layers=[L])):
        with pytest.raises(ValueError):
            m.add_lora(**kw)
        assert not _adapters(m) and m._lora is None and all(p.requires_grad for p in m.parameters()), kw
    odd = _model(intermediate=480)                                          # 480 % 64 != 0: refused for the dense targets only
    with pytest.raises(ValueError, match="intermediate_size"):
        odd.add_lora(targets=("ffn_output",))
    assert not _adapters(odd) and odd._lora is None
    odd.add_lora(targets=("query",))
    assert len(_adapters(odd)) == 2 * L


@pytest.mark.parametrize("t", ["attention_output", "intermediate", "ffn_output"])
def test_merge_folds_each_adapter_into_the_right_master(t):
    m = _model().add_lora(r=4, alpha=8.0, targets=(t,), layers=[2])
    lin = m.bert.encoder.layer[2]
    for part in PATH[t].split("."):
        lin = getattr(lin, part)
    with torch.no_grad():
        lin.lora_B.normal_(0, 0.02)
    want = lin.weight.detach().double() + 2.0 * (lin.lora_B.detach().double() @ lin.lora_A.detach().double())
    others = {n: p.detach().clone() for n, p in m.named_parameters() if ".lora_" not in n and p is not lin.weight}
    keys = set(_model().state_dict())
    m.merge_lora()
    assert set(m.state_dict()) == keys and m._lora is None
    assert torch.allclose(lin.weight.detach().double(), want, rtol=0, atol=1e-7)
    named = dict(m.named_parameters())
    assert all(torch.equal(named[n], v) for n, v in others.items())        # no other master moved


def test_adapter_file_round_trip_with_the_new_keys():
    tg = ("value", "attention_output", "ffn_output")
    m = _model().add_lora(r=8, alpha=12.0, targets=tg, layers=[1, 3], seed=1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B"):
                p.normal_(0, 0.02)
    sd = m.lora_state_dict()
    assert {k: sd[k] for k in ("r", "alpha", "targets", "layers")} == dict(r=8, alpha=12.0, targets=tg, layers=(1, 3))
    tens = {k: v for k, v in sd.items() if torch.is_tensor(v)}
    assert sorted(tens) == sorted(_adapters(m)) == sorted(_key(i, t, x) for i in (1, 3) for t in tg for x in "AB")
    named = dict(m.named_parameters())
    assert all(v.data_ptr() != named[k].data_ptr() and torch.equal(v, named[k]) for k, v in tens.items())     # clones
    fresh = _model()
    fresh.load_lora_state_dict(sd)
    assert fresh._lora == m._lora and all(torch.equal(dict(fresh.named_parameters())[k], v) for k, v in tens.items())
    assert not fresh.bert.embeddings.word_embeddings.weight.requires_grad
    for other_targets in (("value", "attention_output"), ("value", "attention_output", "intermediate"), ("value",), "all-linear"):
        other = _model().add_lora(r=8, alpha=12.0, targets=other_targets, layers=[1, 3])
        with pytest.raises(ValueError, match="differ"):
            other.load_lora_state_dict(sd)
    bad = dict(sd)
    del bad[_key(3, "ffn_output", "B")]
    with pytest.raises(ValueError, match="missing"):
        _model().load_lora_state_dict(bad)
    bad = dict(sd)
    bad[_key(3, "ffn_output", "A")] = torch.zeros(8, H)                     # [r, H] where [r, I] belongs
    with pytest.raises(ValueError, match="shape"):
        _model().load_lora_state_dict(bad)
    m.remove_lora()
    assert not _adapters(m) and m._lora is None


def test_trainable_plan_with_the_new_names():
    """The layer regex of freeze.py sees a dense adapter as a trainable parameter of its layer: no new rule."""
    m = _model().add_lora(r=8, targets=("attention_output", "intermediate", "ffn_output"), layers=[2, 3])
    p = m.trainable_plan()
    assert p.first_layer == 2 and p.stop == 2 and not p.embedding_stage and not p.word_table and sorted(p.layers) == [2, 3]
    assert all(v == "none" for i in p.layers for v in p.layers[i].values())          # frozen base: no weight-gradient problem, no bias sum
    assert "bert.encoder.layer.2.output.dense.weight" in p.frozen and not any(".lora_" in n for n in p.frozen)
    flags = {n: q.requires_grad for n, q in m.named_parameters()}
    for t in ("attention_output", "intermediate", "ffn_output"):           # the pure function on names alone
        flags2 = dict(flags)
        flags2[_key(1, t, "A")] = True
        p2 = F.trainable_plan(flags2, L, {}, {})
        assert p2.first_layer == 1 and p2.stop == 1 and all(v == "none" for v in p2.layers[1].values()), t
    m2 = _model().add_lora(r=8, targets="all-linear", freeze_base=False)
    assert m2.trainable_plan() is None
    m2.freeze(layers=2)
    p3 = m2.trainable_plan()
    assert p3.first_layer == 2 and all(n in p3.frozen for n in _adapters(m2) if ".layer.0." in n or ".layer.1." in n)


def test_apply_lora_and_build_optimizer_wiring():
    from msa_amd import trainer
    from msa_amd.optim import layerwise_param_groups
    args = types.SimpleNamespace(**vars(trainer.default_args()))
    args.lora_rank, args.lora_targets, args.lora_layers = 4, "all-linear", [2, 3]
    m = _model()
    opt, _ = trainer.build_optimizer(m, args, 10)                           # applies the adapters first
    ad = _adapters(m)
    assert len(ad) == 2 * 6 * 2 and m._lora == dict(r=4, alpha=8.0, targets=ALL, layers=(2, 3))
    listed = {id(p) for g in opt.param_groups for p in g["params"]}
    named = dict(m.named_parameters())
    assert all(id(named[n]) in listed for n in ad)
    assert listed == {id(p) for p in m.parameters() if p.requires_grad}
    assert not any(id(p) in listed for n, p in named.items() if n.startswith(BASE) and ".lora_" not in n)
    args.lora_targets = ("query", "ffn_output")
    m = _model()
    assert trainer.apply_lora(m, args) is True and m._lora["targets"] == ("query", "ffn_output")
    groups = layerwise_param_groups(m, 1e-4, layer_decay=0.9)
    assert all(id(p) in {id(q) for g in groups for q in g["params"]} for n, p in m.named_parameters() if ".lora_" in n)


def test_flat_layout_lists_the_new_names_in_their_layer():
    """flat.py's per-layer list names the dense adapters right behind the Q / K / V ones (the order of the source, checked on the text: the
    storage itself needs a device)."""
    src = open(os.path.join(ROOT, "msa_amd", "flat.py")).read()
    qkv = src.index('attention.self.{t}.lora_{m}')
    dense = src.index('("attention.output.dense", "intermediate.dense", "output.dense")')
    assert qkv < dense < src.index('bert.jointEmbeddings.', dense)
    # every adapter is a multiple of 256 elements: it starts a block of its own
    for t in ALL:
        K, N = KN[t]
        assert (4 * K) % 256 == 0 and (N * 4) % 256 == 0


def test_the_abi_is_declared_in_header_and_bindings():
    from msa_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mmbert_hip.h")).read()
    for name, nargs in (("mmbert_lora_dense_fwd", 20), ("mmbert_lora_dense_bwd_workspace", 4), ("mmbert_lora_dense_bwd", 22)):
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "MMBERT_LORA_DENSE_ADD 0" in hdr and "MMBERT_LORA_DENSE_GELU 1" in hdr
    assert (ops.LORA_DENSE_ADD, ops.LORA_DENSE_GELU) == (0, 1)
    # the per-launch wrappers are among those the launch spies can wrap
    assert ops._UNWRAPPED["lora_dense_fwd"] is ops.lora_dense_fwd and ops._UNWRAPPED["lora_dense_bwd"] is ops.lora_dense_bwd
    assert ops.launches_unwrapped()
    orig = ops.lora_dense_fwd
    ops.lora_dense_fwd = lambda *a, **k: orig(*a, **k)
    try:
        assert not ops.launches_unwrapped()
    finally:
        ops.lora_dense_fwd = orig
    assert ops.launches_unwrapped()
