"""CPU tests of msa_amd.optim.LAMB's host side: the trust-unit maps of mmbert_lamb on a hand-made layout, the
trainer.build_optimizer switch, the state_dict kind check."""
import numpy as np
import pytest
import torch


def test_unit_maps_on_a_hand_made_layout():
    from msa_amd.optim import lamb_unit_maps
    spans = [(0, 64), (64, 64),                      # block 0: 64 | 64 | padding 128
             (256, 64), (320, 64), (384, 64),        # block 1: 64 | 64 | 64 | padding 64
             (512, 36), (548, 92),                   # block 2: 36 | 92 | padding 128
             (896, 650),                             # starts in the middle of block 3, blocks 4 and 5 whole, 10 elements of block 6
             (2304, 256)]                            # block 9 whole; blocks 7 and 8 hold nothing of a unit
    unit, mixed, ranges = lamb_unit_maps(spans, 10, others=[(1792, 256), (2056, 8)])
    assert unit.dtype == np.int32 and mixed.dtype == np.int32 and ranges.dtype == np.int32
    assert unit.tolist() == [-2, -3, -4, -5, 7, 7, 7, -1, -1, 8]
    assert mixed.tolist() == [[0, -1, 64, -1, 64, -1, 64, -1],              # record 0: no unit
                              [0, 0, 16, 1, 64, -1, 64, -1],                # (padding stays with the unit before it)
                              [0, 2, 16, 3, 32, 4, 64, -1],
                              [0, 5, 9, 6, 64, -1, 64, -1],
                              [0, -1, 32, 7, 64, -1, 64, -1]]               # what precedes a unit inside a block is no unit's
    assert ranges.tolist() == [[0, 1], [0, 1], [1, 2], [1, 2], [1, 2], [2, 3], [2, 3], [3, 7], [9, 10]]


def test_unit_maps_keep_a_foreign_neighbour_out_of_the_unit():
    from msa_amd.optim import lamb_unit_maps
    # a stepped tensor, a tensor that is not stepped, a stepped one, in one block: the middle stretch measures nothing and takes ratio 1
    unit, mixed, _ = lamb_unit_maps([(0, 64), (128, 64)], 1, others=[(64, 64)])
    assert unit.tolist() == [-2] and mixed[1].tolist() == [0, 0, 16, -1, 32, 1, 64, -1]
    unit, mixed, _ = lamb_unit_maps([(128, 64)], 1, others=[(0, 64), (64, 64)])
    assert mixed[1].tolist() == [0, -1, 32, 0, 64, -1, 64, -1]              # two foreign neighbours are one stretch


def test_unit_maps_refusals():
    from msa_amd.optim import lamb_unit_maps
    with pytest.raises(ValueError, match="multiple of 4"):
        lamb_unit_maps([(0, 30), (30, 10)], 1)
    with pytest.raises(ValueError, match="overlapping"):
        lamb_unit_maps([(0, 300), (256, 8)], 2)
    with pytest.raises(ValueError, match="outside"):
        lamb_unit_maps([(0, 300)], 1)
    with pytest.raises(NotImplementedError, match="stretches"):
        lamb_unit_maps([(0, 8), (8, 8), (16, 8), (24, 8), (32, 8)], 1)
    unit, mixed, ranges = lamb_unit_maps([(0, 0), (0, 256)], 1)             # an empty tensor: a unit without blocks
    assert unit.tolist() == [1] and ranges.tolist() == [[0, 0], [0, 1]] and len(mixed) == 1


def _model():
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    c = MMBertConfig(vocab_size=512, hidden_size=64, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128)
    m = MMBertForPretraining(c)
    m.bert.set_joint_embeddings("mosei")
    return m


def test_build_optimizer_switch():
    from msa_amd import trainer as T
    from msa_amd.optim import AdamW, LAMB
    m = _model()
    args = T.default_args(learning_rate=1e-3)
    assert not hasattr(args, "optimizer") and not hasattr(args, "lamb_always_adapt") and not hasattr(args, "lamb_max_trust")
    opt, _ = T.build_optimizer(m, args, 10)
    assert type(opt) is AdamW
    args.optimizer = "adamw"
    assert type(T.build_optimizer(m, args, 10)[0]) is AdamW
    args.optimizer = "lamb"
    lamb, sched = T.build_optimizer(m, args, 10)
    assert type(lamb) is LAMB and lamb.always_adapt is False and lamb.max_trust is None and sched.opt is lamb
    assert [len(g["params"]) for g in lamb.param_groups] == [len(g["params"]) for g in opt.param_groups]
    assert [g["weight_decay"] for g in lamb.param_groups] == [0.01, 0.0]
    args.lamb_always_adapt, args.lamb_max_trust, args.ema_decay = True, 10.0, 0.99
    lamb, _ = T.build_optimizer(m, args, 10)
    assert lamb.always_adapt is True and lamb.max_trust == 10.0 and lamb._ema_decay == 0.99
    args.optimizer = "lars"
    with pytest.raises(ValueError, match="lars"):
        T.build_optimizer(m, args, 10)
    with pytest.raises(ValueError, match="max_trust"):
        LAMB(list(m.parameters()), max_trust=0.0)


def test_state_dict_names_its_kind_and_another_kind_is_refused():
    from msa_amd.optim import AdamW, LAMB
    ps = [torch.nn.Parameter(torch.zeros(4))]
    lamb, adamw = LAMB(ps), AdamW(ps)
    assert lamb.state_dict()["optimizer"] == "lamb" and adamw.state_dict()["optimizer"] == "adamw"
    with pytest.raises(ValueError, match="adamw"):
        lamb.load_state_dict(adamw.state_dict())
    with pytest.raises(ValueError, match="lamb"):
        adamw.load_state_dict(lamb.state_dict())
    old = {k: v for k, v in lamb.state_dict().items() if k != "optimizer"}
    for opt in (lamb, adamw):                                               # no key: past the kind check (these parameters have no storage)
        with pytest.raises(RuntimeError, match="flat storage"):
            opt.load_state_dict(old)
    assert LAMB(ps).eps == 1e-6 and LAMB(ps).param_groups[0]["weight_decay"] == 0.01
