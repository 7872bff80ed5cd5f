"""The label-only step's host side (no GPU): ``args.label_only`` through the trainer's packing and epoch loop, the storage's record of
the parameters such a step does not reach, and what the optimizer makes of it."""
import types

import numpy as np
import torch

from msa_amd import trainer as T
from msa_amd import flat as F


def test_default_args_have_the_key_off():
    assert T.default_args().label_only is False
    assert T.default_args(label_only=True).label_only is True


def _examples(n=4, L=6, D=3, seed=0):
    """``n`` items in the dataset's 16-tuple form (tests' sizes: text length L, one pair feature of width D per position)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ids = torch.tensor([101] + rng.integers(1000, 2000, L - 2).tolist() + [102])
        tti = torch.zeros(L, dtype=torch.long)
        vis = rng.normal(size=(L, D))
        sp = rng.integers(1, 9, size=(L, D))
        out.append((ids, 1, tti, 0.5 * i, ids.numpy().copy(), vis, i % 2, torch.ones(L, dtype=torch.long), 0.5 * i,
                    ids.numpy().copy(), sp, (i + 1) % 2, torch.ones(L, dtype=torch.long), 0.5 * i, "seg%d" % i, "raw%d" % i))
    return out


class _Model:
    def __init__(self):
        self.calls = []

    def train(self):
        pass

    def eval(self):
        pass

    def __call__(self, **kw):
        self.calls.append(kw)
        loss = torch.ones((), requires_grad=True) * 2.0
        B = kw["input_ids"][0].shape[0]
        return (loss, None, None, None, torch.zeros(()), torch.zeros(())), torch.zeros(B, 1)


class _Opt:
    def step(self):
        pass

    def zero_grad(self):
        pass


def test_pack_step_inputs_hands_over_the_unmasked_ids_and_no_labels():
    batch = T.collate(_examples())
    gen = torch.Generator().manual_seed(3)
    before = gen.get_state().clone()
    kw = T.pack_step_inputs(batch, T.default_args(label_only=True), "cpu", gen)
    assert kw["masked_labels"] is None
    assert torch.equal(gen.get_state(), before)                      # nothing was drawn from the mask generator
    assert torch.equal(kw["input_ids"][0], batch[0][0]) and torch.equal(kw["input_ids"][3], batch[1][0]) and torch.equal(kw["input_ids"][4], batch[2][0])
    std = T.pack_step_inputs(batch, T.default_args(), "cpu", torch.Generator().manual_seed(3))
    assert set(std) == set(kw)
    for k in ("token_type_ids", "attention_mask", "ap_label"):
        for a, b in zip(std[k], kw[k]):
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert torch.equal(x, y), k
    assert torch.equal(std["sentiment"], kw["sentiment"]) and std["masked_labels"] is not None
    assert std["input_ids"][1] is not None and torch.equal(std["input_ids"][1], kw["input_ids"][1])


def test_train_and_eval_epochs_pass_unmasked_ids_and_none():
    data = _examples()
    gen = torch.Generator().manual_seed(5)
    before = gen.get_state().clone()
    args = T.default_args(label_only=True, train_batch_size=2, val_batch_size=2)
    m = _Model()
    T.train_epoch(args, m, data, _Opt(), _Opt(), device="cpu", generator=gen, shuffle=False)
    assert len(m.calls) == 2
    raw = torch.stack([e[0] for e in data])
    for i, kw in enumerate(m.calls):
        assert kw["masked_labels"] is None
        assert torch.equal(kw["input_ids"][0], raw[2 * i:2 * i + 2])
        assert not bool((kw["input_ids"][0] == T.MASK).any())
    m = _Model()
    T.eval_epoch(args, m, data, device="cpu", generator=gen)
    assert len(m.calls) == 2 and all(kw["masked_labels"] is None for kw in m.calls)
    assert torch.equal(gen.get_state(), before)
    # the standard loop on the same data draws from it and hands labels over
    m = _Model()
    T.train_epoch(T.default_args(train_batch_size=2), m, data, _Opt(), _Opt(), device="cpu", generator=gen, shuffle=False)
    assert all(kw["masked_labels"] is not None for kw in m.calls) and not torch.equal(gen.get_state(), before)


class _P:
    def __init__(self):
        self.grad = "attached"


def _storage(names):
    """A FlatParams with the host-side state set_frozen works on and nothing else (no buffers: nothing leaves the set here but through
    ``_attach``, which is recorded)."""
    f = F.FlatParams.__new__(F.FlatParams)
    f.named = {n: _P() for n in names}
    f.frozen, f.unreached, f.stale, f.lazy = frozenset(), frozenset(), set(), {}
    f.offset = {n: 256 * i for i, n in enumerate(names)}
    f.numel = {n: 4 for n in names}
    f.grads = torch.zeros(256 * len(names))
    f._owner = lambda: None
    f._attach = types.MethodType(lambda self, n: setattr(self.named[n], "grad", "attached"), f)
    return f


def test_unreached_parameters_join_and_leave_the_frozen_set():
    f = _storage(["a", "b", "c"])
    f.set_frozen(frozenset({"a"}), frozenset({"b"}))
    assert f.frozen == {"a", "b"} and f.unreached == {"b"}
    assert f.named["a"].grad is None and f.named["b"].grad is None and f.named["c"].grad == "attached"
    f.set_frozen(frozenset({"a"}))                                   # a standard step: b is reached again
    assert f.frozen == {"a"} and f.unreached == frozenset() and f.named["b"].grad == "attached" and f.named["a"].grad is None
    f.set_frozen(frozenset({"a", "b"}), frozenset({"b"}))            # frozen by the caller AND unreached: frozen is what it is
    assert f.unreached == frozenset() and f.frozen == {"a", "b"}


def test_adamw_lets_unreached_parameters_back_and_still_refuses_unfrozen_ones():
    from msa_amd.optim import AdamW
    import pytest
    opt = AdamW.__new__(AdamW)
    built = []
    opt._build_maps = lambda flat: (built.append(flat.frozen), setattr(opt, "_frozen", flat.frozen), setattr(opt, "_unreached", flat.unreached))
    opt._build_flags = lambda: None
    opt._listed = frozenset({"a", "b", "c"})
    opt._steps = 3
    f = _storage(["a", "b", "c"])
    opt._flat = f
    f.set_frozen(frozenset({"a"}), frozenset({"b"}))
    opt._frozen, opt._unreached = frozenset(), frozenset()
    opt._follow_frozen()
    assert built[-1] == {"a", "b"}
    f.set_frozen(frozenset({"a"}))                                   # b reached again after steps: no error, maps rebuilt
    opt._follow_frozen()
    assert built[-1] == {"a"}
    f.set_frozen(frozenset())                                        # a unfrozen after steps: refused, as before
    with pytest.raises(NotImplementedError, match="became trainable"):
        opt._follow_frozen()
