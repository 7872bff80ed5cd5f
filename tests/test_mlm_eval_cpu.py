"""CPU: the host logic of ``trainer.mlm_eval_epoch`` over a stub model whose ``predict_tokens`` returns known ranks and
log-probabilities -- counts, token-weighted loss, perplexity, top-1, top-k and MRR across uneven batches and an empty pass."""
import math
import types

import pytest
import torch

from msa_amd import trainer as T

NAMES = ("text", "visual", "speech")


class Stub:
    """``predict_tokens`` hands back what the batch carries under "stub": per pass (ranks, log-probabilities)."""

    def __init__(self):
        self.training = True
        self.calls = []

    def predict_tokens(self, input_ids, token_type_ids, attention_mask, masked_labels=None, positions=None, top_k=5):
        assert positions is None and masked_labels is not None
        self.calls.append((input_ids, top_k))
        out = {}
        for n, (rank, lp) in zip(NAMES, masked_labels):
            rank = torch.tensor(rank, dtype=torch.int64)
            out[n] = dict(index=torch.zeros((rank.numel(), 2), dtype=torch.int64), top_ids=torch.zeros((rank.numel(), top_k), dtype=torch.int64),
                          top_logprob=torch.zeros((rank.numel(), top_k)), label=torch.zeros(rank.numel(), dtype=torch.int64),
                          label_logprob=torch.tensor(lp, dtype=torch.float32), label_rank=rank)
        out["loss"] = torch.zeros(3)
        return out


def batch(i, per_pass):
    return dict(input_ids=i, token_type_ids=None, attention_mask=None, masked_labels=per_pass, ap_label=None, sentiment=None)


def test_metrics_over_uneven_batches_and_an_empty_pass():
    # text: 3 + 1 + 0 positions; visual: 2 + 0 + 4; speech: none at all
    b = [batch(0, (([0, 2, 7], [-0.5, -1.5, -4.0]), ([0, 0], [-0.25, -0.125]), ([], []))),
         batch(1, (([1], [-3.0]), ([], []), ([], []))),
         batch(2, (([], []), ([3, 0, 4, 30000], [-3.0, -0.5, -2.5, -11.0]), ([], [])))]
    m = Stub()
    got = T.mlm_eval_epoch(types.SimpleNamespace(mlm=True), m, None, device="cpu", batches=iter(b), top_k=4)
    assert m.training and [c[0] for c in m.calls] == [0, 1, 2] and all(c[1] == 4 for c in m.calls)       # in order, top_k handed on

    def want(ranks, lps, k):
        n = len(ranks)
        loss = -sum(lps) / n
        return dict(count=n, loss=loss, perplexity=math.exp(loss), top1=sum(r == 0 for r in ranks) / n, topk=sum(r < k for r in ranks) / n,
                    mrr=sum(1.0 / (r + 1) for r in ranks) / n)
    exp = {"text": want([0, 2, 7, 1], [-0.5, -1.5, -4.0, -3.0], 4), "visual": want([0, 0, 3, 0, 4, 30000], [-0.25, -0.125, -3.0, -0.5, -2.5, -11.0], 4)}
    for n in ("text", "visual"):
        assert got[n]["count"] == exp[n]["count"] and isinstance(got[n]["count"], int)
        for key in ("loss", "perplexity", "top1", "topk", "mrr"):
            assert got[n][key] == pytest.approx(exp[n][key], rel=1e-12), (n, key)
    # token-weighted: not the mean of the batches' means
    assert got["text"]["loss"] != pytest.approx(((0.5 + 1.5 + 4.0) / 3 + 3.0) / 2)
    assert got["speech"] == dict(count=0, loss=0.0, perplexity=0.0, top1=0.0, topk=0.0, mrr=0.0)
    assert got["text"]["top1"] <= got["text"]["topk"] <= 1.0


def test_top_k_is_the_rank_threshold():
    b = [batch(0, (([0, 1, 2, 3, 4, 5], [-1.0] * 6), ([], []), ([], [])))]
    for k, share in ((1, 1 / 6), (3, 0.5), (5, 5 / 6)):
        got = T.mlm_eval_epoch(types.SimpleNamespace(mlm=False), Stub(), None, device="cpu", batches=b, top_k=k)
        assert got["text"]["topk"] == pytest.approx(share) and got["text"]["top1"] == pytest.approx(1 / 6)
        assert got["text"]["loss"] == pytest.approx(1.0) and got["text"]["perplexity"] == pytest.approx(math.e)


def test_an_empty_dataset_gives_zeros():
    m = Stub()
    m.training = False
    got = T.mlm_eval_epoch(types.SimpleNamespace(mlm=True), m, None, device="cpu", batches=[])
    assert not m.training and not m.calls
    assert got == {n: dict(count=0, loss=0.0, perplexity=0.0, top1=0.0, topk=0.0, mrr=0.0) for n in NAMES}


def test_a_huge_loss_does_not_overflow_the_perplexity():
    got = T.mlm_eval_epoch(types.SimpleNamespace(mlm=True), Stub(), None, device="cpu", batches=[batch(0, (([9], [-1000.0]), ([], []), ([], [])))])
    assert got["text"]["loss"] == pytest.approx(1000.0) and math.isfinite(got["text"]["perplexity"])
