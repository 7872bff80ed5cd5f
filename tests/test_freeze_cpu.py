"""CPU tests of the frozen-parameter decisions (msa_amd/freeze.py: a pure function of the ``requires_grad`` flags and the flat layout) and of
the interface around them (model.freeze / unfreeze, trainer.apply_freeze, the optimizer groups)."""
import types

import pytest
import torch

from msa_amd import freeze as F

L, H = 4, 128
EMB = "bert.embeddings."
JOINT = "bert.jointEmbeddings."


def _model():
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=512, hidden_size=H, num_hidden_layers=L, num_attention_heads=2, intermediate_size=512)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings("mosei")
    return m


@pytest.fixture(scope="module")
def layout():
    """(names, offset, numel) packed as flat.FlatParams packs: 256-aligned groups; the q / k / v weights, the q / k / v biases and a
    LayerNorm's weight and bias are neighbours inside one group."""
    named = dict(_model().named_parameters())
    groups, used = [], set()

    def add(*ns):
        g = [n for n in ns if n in named and n not in used]
        if g:
            groups.append(g)
            used.update(g)
    for n in named:
        if n.endswith("LayerNorm.weight"):
            add(n, n[:-6] + "bias")
        elif n.endswith("attention.self.query.weight"):
            add(n, n.replace("query", "key"), n.replace("query", "value"))
        elif n.endswith("attention.self.query.bias"):
            add(n, n.replace("query", "key"), n.replace("query", "value"))
    for n in named:
        add(n)
    offset, numel, off = {}, {}, 0
    for g in groups:
        off = (off + 255) // 256 * 256
        for n in g:
            offset[n], numel[n] = off, named[n].numel()
            off += numel[n]
    return list(named), offset, numel


def _plan(layout, frozen):
    names, offset, numel = layout
    frozen = set(frozen)
    assert frozen <= set(names)
    return F.trainable_plan({n: n not in frozen for n in names}, L, offset, numel)


def _sel(layout, **kw):
    return F.resolve_freeze(layout[0], L, **kw)


ALL = {"qkv": "full", "o": "full", "w1": "full", "w2": "full"}
BIAS = {k: "bias" for k in ALL}


def test_nothing_frozen_is_no_plan(layout):
    assert _plan(layout, []) is None
    # the parameters the reference never differentiates decide no work, whatever their flag says
    never = [n for n in layout[0] if F.never_trainable(n)]
    p = _plan(layout, never)
    assert never and p.frozen == frozenset(never) and p.stop == 0 and p.embedding_stage and p.word_table
    assert all(dict(p.layers[i]) == ALL for i in range(L))


@pytest.mark.parametrize("k,first", [(2, 2), (3, 3), (4, 4)])
def test_frozen_prefix_with_embeddings(layout, k, first):                  # sets a, b, c
    p = _plan(layout, _sel(layout, embeddings=True, layers=k))
    assert p.first_layer == first and p.stop == first and not p.embedding_stage and not p.word_table
    assert sorted(p.layers) == list(range(first, L)) and all(dict(p.layers[i]) == ALL for i in p.layers)
    assert "bert.embeddings.word_embeddings.weight" in p.frozen and "cls.predictions.bias" not in p.frozen


def test_frozen_layers_with_trainable_embeddings(layout):                  # set d: every input gradient runs, only weight gradients go
    p = _plan(layout, _sel(layout, layers=2))
    assert p.first_layer == 2 and p.embedding_stage and p.stop == 0 and p.word_table
    assert sorted(p.layers) == [0, 1, 2, 3]
    assert all(m == "none" for i in (0, 1) for m in p.layers[i].values()) and dict(p.layers[2]) == ALL


def test_layer_weights(layout):                                            # sets e and f
    p = _plan(layout, _sel(layout, layer_weights=True))
    assert p.first_layer == 0 and p.stop == 0 and p.embedding_stage and all(dict(p.layers[i]) == BIAS for i in range(L))
    p = _plan(layout, _sel(layout, embeddings=True, layers=2, layer_weights=True))
    assert p.first_layer == 2 and p.stop == 2 and sorted(p.layers) == [2, 3] and all(dict(p.layers[i]) == BIAS for i in (2, 3))


def test_single_problem_and_word_table(layout):                            # sets g and h
    w = "bert.encoder.layer.1.intermediate.dense."
    p = _plan(layout, [w + "weight", w + "bias"])
    assert p.stop == 0 and dict(p.layers[1]) == dict(ALL, w1="none") and dict(p.layers[0]) == ALL and p.word_table
    p = _plan(layout, [w + "weight"])
    assert dict(p.layers[1]) == dict(ALL, w1="bias")
    p = _plan(layout, ["bert.embeddings.word_embeddings.weight"])
    assert p.stop == 0 and p.embedding_stage and not p.word_table and all(dict(p.layers[i]) == ALL for i in range(L))
    # the packed q / k / v weights count as frozen only when all three are
    q = "bert.encoder.layer.2.attention.self."
    assert _plan(layout, [q + "query.weight"]).layers[2]["qkv"] == "full"
    assert _plan(layout, [q + x + ".weight" for x in ("query", "key", "value")]).layers[2]["qkv"] == "bias"


def test_packed_neighbours_raise(layout):
    q = "bert.encoder.layer.0.attention.self.query.bias"
    with pytest.raises(NotImplementedError) as e:
        _plan(layout, [q])
    assert q in str(e.value) and "bert.encoder.layer.0.attention.self.key.bias" in str(e.value)
    ln = "bert.encoder.layer.1.output.LayerNorm.weight"
    with pytest.raises(NotImplementedError) as e:
        _plan(layout, [ln])
    assert ln in str(e.value) and "bert.encoder.layer.1.output.LayerNorm.bias" in str(e.value)
    assert _plan(layout, [ln, ln[:-6] + "bias"]) is not None
    # at H = 256 a bias fills its block: no neighbour shares it
    names, offset, numel = layout
    wide = {n: (o * 2) for n, o in offset.items()}
    wide_n = {n: (k * 2 if k == H else k) for n, k in numel.items()}
    assert F.trainable_plan({n: n != q for n in names}, L, wide, wide_n) is not None


def test_freeze_and_unfreeze_resolve_names():
    m = _model()
    names = m.freeze(embeddings=True, layers=2)
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen == set(names) and all(n.startswith((EMB, JOINT, "bert.encoder.layer.0.", "bert.encoder.layer.1.")) for n in names)
    assert {n for n, _ in m.named_parameters() if n.startswith((EMB, JOINT))} <= frozen
    p = m.trainable_plan()
    assert p.first_layer == 2 and not p.embedding_stage
    m.unfreeze()
    assert all(p.requires_grad for p in m.parameters()) and m.trainable_plan() is None
    got = m.freeze(layers=[3], layer_weights=True)
    assert "bert.encoder.layer.3.output.LayerNorm.weight" in got and "bert.encoder.layer.0.output.dense.weight" in got
    assert "bert.encoder.layer.0.output.dense.bias" not in got and "bert.encoder.layer.0.output.LayerNorm.weight" not in got
    for bad in (dict(layers=L + 1), dict(layers=-1), dict(layers=[L]), dict(layers=[0, -1])):
        with pytest.raises(ValueError):
            m.freeze(**bad)


def test_apply_freeze_and_optimizer_groups():
    from msa_amd import trainer
    from msa_amd.optim import layerwise_param_groups
    m = _model()
    assert trainer.apply_freeze(m, trainer.default_args()) == [] and all(p.requires_grad for p in m.parameters())
    args = types.SimpleNamespace(**vars(trainer.default_args()))
    args.freeze_embeddings, args.freeze_layers = True, 2
    names = trainer.apply_freeze(m, args)
    assert names and all(not dict(m.named_parameters())[n].requires_grad for n in names)
    frozen = {id(p) for p in m.parameters() if not p.requires_grad}
    opt, _ = trainer.build_optimizer(m, args, 10)
    listed = {id(p) for g in opt.param_groups for p in g["params"]}
    assert listed and not (listed & frozen) and listed == {id(p) for p in m.parameters() if p.requires_grad}
    groups = layerwise_param_groups(m, 1e-4, layer_decay=0.9)
    listed = {id(p) for g in groups for p in g["params"]}
    assert listed and not (listed & frozen)
