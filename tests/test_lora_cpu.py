"""CPU tests of the low-rank adapters' interface: model.add_lora and its bookkeeping, trainer.apply_lora / build_optimizer,
freeze.trainable_plan with adapter names (a pure function: no GPU), the adapter file's metadata."""
import math
import types

import pytest
import torch

from msa_amd import freeze as F

L, H = 4, 128
BASE = ("bert.embeddings.", "bert.jointEmbeddings.", "bert.encoder.")


def _model():
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=512, hidden_size=H, num_hidden_layers=L, num_attention_heads=2, intermediate_size=512)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings("mosei")
    return m


def _adapters(m):
    return [n for n, _ in m.named_parameters() if ".lora_" in n]


def test_add_lora_registers_parameters_and_freezes_the_base():
    m = _model()
    keys = set(m.state_dict())
    assert m.add_lora(r=8, alpha=16.0, targets=("value", "query"), seed=3) is m
    ad = _adapters(m)
    assert sorted(ad) == sorted(f"bert.encoder.layer.{i}.attention.self.{t}.lora_{x}" for i in range(L) for t in ("query", "value") for x in "AB")
    named = dict(m.named_parameters())
    for n in ad:
        p = named[n]
        assert p.requires_grad and tuple(p.shape) == ((8, H) if n.endswith("A") else (H, 8))
        if n.endswith("B"):
            assert not bool(p.any())
        else:
            assert float(p.detach().abs().max()) <= 1.0 / math.sqrt(H) and float(p.detach().std()) > 0.3 / math.sqrt(H)     # kaiming_uniform_(a = sqrt 5): U(+-1 / sqrt H)
    for n, p in named.items():
        if ".lora_" not in n:
            assert p.requires_grad == (not n.startswith(BASE)), n
    assert m._lora == dict(r=8, alpha=16.0, targets=("query", "value"), layers=(0, 1, 2, 3)) and m._flat is None
    assert set(m.state_dict()) == keys | set(ad)
    # the same seed gives the same A; another seed another
    a, b, c = _model().add_lora(seed=3), _model().add_lora(seed=3), _model().add_lora(seed=4)
    k = "bert.encoder.layer.2.attention.self.value.lora_A"
    assert torch.equal(a.state_dict()[k], b.state_dict()[k]) and not torch.equal(a.state_dict()[k], c.state_dict()[k])
    # freeze_base=False leaves every flag alone
    u = _model().add_lora(freeze_base=False)
    assert all(p.requires_grad for p in u.parameters())


def test_add_lora_refuses_bad_arguments_and_a_second_call():
    m = _model()
    for kw in (dict(r=3), dict(r=0), dict(r=8.0), dict(r=True), dict(targets=()), dict(targets=("output",)), dict(targets=("key", "key")),
               dict(layers=[]), dict(layers=[L]), dict(layers=[0, 0]), dict(layers=[1.0]), dict(alpha=float("inf"))):
        with pytest.raises(ValueError):
            m.add_lora(**kw)
        assert not _adapters(m) and m._lora is None and all(p.requires_grad for p in m.parameters()), kw
    m.add_lora(r=4, targets="key", layers=[1])
    assert _adapters(m) == ["bert.encoder.layer.1.attention.self.key.lora_A", "bert.encoder.layer.1.attention.self.key.lora_B"]
    with pytest.raises(ValueError, match="already has adapters"):
        m.add_lora()
    m.remove_lora()
    assert not _adapters(m) and m._lora is None
    m.add_lora(r=16, layers=[3, 0])
    assert m._lora["layers"] == (0, 3)


def test_merge_folds_the_update_into_the_masters():
    m = _model().add_lora(r=4, alpha=8.0, targets=("query",), layers=[2])
    lin = m.bert.encoder.layer[2].attention.self.query
    with torch.no_grad():
        lin.lora_B.normal_(0, 0.02)
    want = lin.weight.detach().double() + 2.0 * (lin.lora_B.detach().double() @ lin.lora_A.detach().double())
    keys = set(_model().state_dict())
    m.merge_lora()
    assert set(m.state_dict()) == keys and m._lora is None
    assert torch.allclose(lin.weight.detach().double(), want, rtol=0, atol=1e-7)
    with pytest.raises(ValueError, match="no adapters"):
        m.merge_lora()


def test_adapter_file_metadata_and_round_trip():
    m = _model().add_lora(r=8, alpha=12.0, targets=("query", "value"), layers=[1, 3], seed=1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B"):
                p.normal_(0, 0.02)
    sd = m.lora_state_dict()
    assert {k: sd[k] for k in ("r", "alpha", "targets", "layers")} == dict(r=8, alpha=12.0, targets=("query", "value"), layers=(1, 3))
    tens = {k: v for k, v in sd.items() if torch.is_tensor(v)}
    assert sorted(tens) == sorted(_adapters(m)) and len(tens) == 8
    named = dict(m.named_parameters())
    assert all(v.data_ptr() != named[k].data_ptr() and torch.equal(v, named[k]) for k, v in tens.items())     # clones
    fresh = _model()
    fresh.load_lora_state_dict(sd)
    assert fresh._lora == m._lora and all(torch.equal(dict(fresh.named_parameters())[k], v) for k, v in tens.items())
    assert not fresh.bert.embeddings.word_embeddings.weight.requires_grad                                   # created with the frozen base
    other = _model().add_lora(r=8, alpha=12.0, targets=("query", "value"), layers=[1, 2])
    with pytest.raises(ValueError, match="differ"):
        other.load_lora_state_dict(sd)
    bad = dict(sd)
    del bad["bert.encoder.layer.3.attention.self.value.lora_B"]
    with pytest.raises(ValueError, match="missing"):
        _model().load_lora_state_dict(bad)
    with pytest.raises(ValueError, match="no adapters"):
        _model().lora_state_dict()


def test_trainable_plan_with_adapter_names():
    """The layer regex of freeze.py sees an adapter as a trainable parameter of its layer: no new rule."""
    m = _model().add_lora(r=8, layers=[2, 3])
    p = m.trainable_plan()
    assert p.first_layer == 2 and p.stop == 2 and not p.embedding_stage and not p.word_table and sorted(p.layers) == [2, 3]
    assert all(v == "none" for i in p.layers for v in p.layers[i].values())
    assert "bert.encoder.layer.2.attention.self.query.weight" in p.frozen and not any(".lora_" in n for n in p.frozen)
    flags = {n: q.requires_grad for n, q in m.named_parameters()}
    # the pure function on names alone: an adapter on layer 1 moves the start of backward there; q / k / v weights stay "none"
    flags2 = dict(flags)
    flags2["bert.encoder.layer.1.attention.self.query.lora_A"] = True
    p2 = F.trainable_plan(flags2, L, {}, {})
    assert p2.first_layer == 1 and p2.layers[1]["qkv"] == "none"
    # adapters beside trainable projection weights: both run
    m2 = _model().add_lora(r=8, freeze_base=False)
    assert m2.trainable_plan() is None
    m2.freeze(layers=2)                                                    # freezing layers takes their adapters along
    p3 = m2.trainable_plan()
    assert p3.first_layer == 2 and all(n in p3.frozen for n in _adapters(m2) if ".layer.0." in n or ".layer.1." in n)


def test_apply_lora_and_build_optimizer_wiring():
    from msa_amd import trainer
    from msa_amd.optim import layerwise_param_groups
    m = _model()
    assert trainer.apply_lora(m, trainer.default_args()) is False and not _adapters(m)
    opt, _ = trainer.build_optimizer(m, trainer.default_args(), 10)          # no lora_rank: nothing happens
    assert not _adapters(m)
    args = types.SimpleNamespace(**vars(trainer.default_args()))
    args.lora_rank, args.lora_targets, args.lora_layers = 4, ("query", "key", "value"), [2, 3]
    m = _model()
    opt, _ = trainer.build_optimizer(m, args, 10)                           # applies the adapters first
    ad = _adapters(m)
    assert len(ad) == 2 * 3 * 2 and m._lora == dict(r=4, alpha=8.0, targets=("query", "key", "value"), layers=(2, 3))
    listed = {id(p) for g in opt.param_groups for p in g["params"]}
    named = dict(m.named_parameters())
    assert all(id(named[n]) in listed for n in ad)
    assert listed == {id(p) for p in m.parameters() if p.requires_grad}
    assert not any(id(p) in listed for n, p in named.items() if n.startswith(BASE) and ".lora_" not in n)
    trainer.build_optimizer(m, args, 10)                                    # adapters already there: not applied twice
    assert len(_adapters(m)) == len(ad)
    groups = layerwise_param_groups(m, 1e-4, layer_decay=0.9)
    assert all(id(named[n]) in {id(p) for g in groups for p in g["params"]} for n in ad)


def test_ops_mask_helper():
    from msa_amd import ops
    assert ops.lora_mask(("query",)) == 1 and ops.lora_mask(("value", "query")) == 5 and ops.lora_mask("key") == 2
    for bad in ((), ("q",), ("query", "query")):
        with pytest.raises(ValueError):
            ops.lora_mask(bad)
