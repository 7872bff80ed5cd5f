"""CPU: global gradient-norm clipping's host side -- the segment list the norm kernel reads, the argument checks, and where
train_epoch calls the optimizer's clip (stubs, no GPU)."""
import math

import pytest
import torch

from msa_amd import flat as F
from msa_amd import optim
from msa_amd import trainer as T


def _maps(layout):
    """offset / numel maps of a hand-made flat layout: [(name, offset, numel)]"""
    return {n: o for n, o, _ in layout}, {n: k for n, _, k in layout}


# two parameters packed into one 256-element block (odd lengths, the second unaligned), a frozen one, a block-aligned pair
LAYOUT = [("a.bias", 0, 3), ("a.weight", 3, 250), ("bert.jointEmbeddings.W_cv.weight", 256, 300), ("c.weight", 768, 256),
          ("c.bias", 1024, 7), ("d.weight", 1280, 1)]


def test_segments_merge_adjacent_parameters_and_keep_odd_edges():
    off, num = _maps(LAYOUT)
    names = [n for n, _, _ in LAYOUT]
    assert F.grad_segments(off, num, names) == [(0, 253), (256, 300), (768, 263), (1280, 1)]
    # frozen names excluded: the neighbours on either side stay apart (the frozen span is a gap)
    assert F.grad_segments(off, num, names, exclude=F.FROZEN) == [(0, 253), (768, 263), (1280, 1)]


def test_segments_of_a_subset_and_of_repeated_names():
    off, num = _maps(LAYOUT)
    assert F.grad_segments(off, num, ["a.weight"]) == [(3, 250)]                      # unaligned start, odd length
    assert F.grad_segments(off, num, ["c.bias", "a.bias", "a.bias"]) == [(0, 3), (1024, 7)]     # buffer order, each once
    assert F.grad_segments(off, num, ["d.weight", "c.weight"]) == [(768, 256), (1280, 1)]
    assert F.grad_segments(off, num, []) == []


def test_segments_cover_exactly_the_named_elements():
    off, num = _maps(LAYOUT)
    for names in (["a.bias", "c.bias"], ["a.weight", "c.weight", "c.bias"], [n for n, _, _ in LAYOUT]):
        want = sorted(e for n in names for e in range(off[n], off[n] + num[n]))
        got = sorted(e for o, k in F.grad_segments(off, num, names) for e in range(o, o + k))
        assert got == want


def test_clip_argument_checks():
    assert optim._clip_args(1, 2) == (1.0, 2.0)
    assert optim._clip_args(0.5, "inf") == (0.5, math.inf)
    assert optim._clip_args(0.0, math.inf) == (0.0, math.inf)
    for bad in (1.0, 3.0, 0.0, -math.inf):
        with pytest.raises(NotImplementedError):
            optim._clip_args(1.0, bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            optim._clip_args(bad, 2.0)
    # the optimizer's fused clip checks before it touches any storage
    opt = optim.AdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    with pytest.raises(NotImplementedError):
        opt.clip_grad_norm_(1.0, norm_type=1.0)
    with pytest.raises(ValueError):
        opt.clip_grad_norm_(-0.5)


def test_drop_in_falls_back_to_torch_off_flat_storage():
    """Parameters outside msa_amd flat storage: torch's clip, any norm_type (here on the CPU)."""
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    p.grad = torch.tensor([3.0, 0.0, 4.0])
    q.grad = None                                                                          # skipped, as torch skips it
    n = optim.clip_grad_norm_([p, q], 1.0)
    assert abs(float(n) - 5.0) < 1e-6 and torch.allclose(p.grad, torch.tensor([0.6, 0.0, 0.8]), atol=1e-6)
    p.grad = torch.tensor([3.0, 0.0, 4.0])
    n1 = optim.clip_grad_norm_(p, 100.0, norm_type=1.0)
    assert abs(float(n1) - 7.0) < 1e-6 and torch.equal(p.grad, torch.tensor([3.0, 0.0, 4.0]))


def test_default_args_have_no_max_grad_norm():
    assert not hasattr(T.default_args(), "max_grad_norm")
    assert T.default_args(max_grad_norm=1.0).max_grad_norm == 1.0


class _Opt:
    def __init__(self, log):
        self.log = log

    def clip_grad_norm_(self, max_norm, norm_type=2.0):
        self.log.append(("clip", max_norm))
        return torch.zeros(())

    def step(self):
        self.log.append(("step",))

    def zero_grad(self):
        self.log.append(("zero",))


class _Sched:
    def step(self):
        pass


class _Model:
    def __init__(self, log):
        self.log = log

    def train(self):
        pass

    def __call__(self, **kw):
        self.log.append(("fb", kw["i"]))
        loss = torch.ones(1, requires_grad=True)
        return (loss, None, None, None, torch.zeros(()), torch.zeros(())), None


class _DP:
    def __init__(self, log):
        self.log = log

    def no_sync(self):
        log = self.log

        class _Ctx:
            def __enter__(self):
                log.append(("no_sync",))

            def __exit__(self, *a):
                return False
        return _Ctx()

    def finish_backward(self):
        self.log.append(("finish",))


def _run(args, n, quirk, dp=False):
    log = []
    T.train_epoch(args, _Model(log), None, _Opt(log), _Sched(), device="cpu", quirk_step=quirk, dp=_DP(log) if dp else None,
                  batches=[dict(i=i) for i in range(n)])
    return log


@pytest.mark.parametrize("quirk", [True, False])
def test_train_epoch_clips_once_per_optimizer_step(quirk):
    args = T.default_args(gradient_accumulation_step=2, max_grad_norm=0.25)
    log = _run(args, 6, quirk)
    steps = [i for i in range(6) if T.should_step(i, 2, quirk)]
    assert steps == ([0, 3, 4] if quirk else [1, 3, 5])              # the `&` quirk: (step + 1) & 2 == 0
    want = []
    for i in range(6):
        want.append(("fb", i))
        if i in steps:
            want += [("clip", 0.25), ("step",), ("zero",)]
    assert log == want


def test_train_epoch_clips_after_the_gradient_exchange():
    args = T.default_args(gradient_accumulation_step=1, max_grad_norm=1.0)
    log = _run(args, 2, False, dp=True)
    assert log == [e for i in range(2) for e in (("fb", i), ("finish",), ("clip", 1.0), ("step",), ("zero",))]


def test_train_epoch_without_the_key_never_clips():
    for args in (T.default_args(gradient_accumulation_step=2), T.default_args(gradient_accumulation_step=2, max_grad_norm=None)):
        log = _run(args, 4, True)
        assert ("step",) in log and not any(e[0] == "clip" for e in log)
