"""copy.deepcopy / torch.save of the whole module without a GPU: the copy carries parameters and settings, none of the runtime state
(flat storage, views, streams, last outputs), and its parts point at the copy, not at the original (the GPU half:
tests/test_flat_semantics_gpu.py)."""
import copy

import pytest
import torch


def _model():
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    m = MMBertForPretraining(MMBertConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128))
    m.bert.set_joint_embeddings("mosei")
    return m


def _runtime_leftovers(m):
    """What a step leaves in the module: stand-ins that can be neither copied nor pickled."""
    m._flat = lambda: None                                               # (a local function: deepcopy shares it, pickle refuses it)
    m._lw, m._w, m._plans = [m._flat], {"x": m._flat}, {"k": m._flat}
    m.__dict__["_input_stream"] = m._flat
    m.__dict__["_pro_marks"] = {0: m._flat}
    m.outputs = (torch.ones(3, requires_grad=True) * 2,)                 # a non-leaf tensor: deepcopy refuses it


def _check_copy(m, c):
    assert c is not m and c._flat is None and c._plans == {}
    for k in ("_lw", "_w", "_input_stream", "_pro_marks", "outputs"):
        assert k not in c.__dict__, k
    assert c.bert._owner() is c and c.cls._owner() is c and c.bert.jointEmbeddings._owner() is c
    assert m.bert._owner() is m and m.cls._owner() is m and m.bert.jointEmbeddings._owner() is m
    assert c.cls.predictions.decoder.weight is c.bert.embeddings.word_embeddings.weight
    assert c.cls.predictions.decoder.bias is c.cls.predictions.bias
    a, b = m.state_dict(), c.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr(), k
    with torch.no_grad():
        c.classifier1_2.weight.add_(1.0)
    assert not torch.equal(m.classifier1_2.weight, c.classifier1_2.weight)
    assert (c.num_labels, c.alpha, c.beta, c._seed, c.coop_heads) == (m.num_labels, m.alpha, m.beta, m._seed, m.coop_heads)


def test_deepcopy_carries_no_runtime_state():
    m = _model()
    m.manual_seed(77)
    _runtime_leftovers(m)
    _check_copy(m, copy.deepcopy(m))
    assert m.outputs and m._w                                             # the original keeps its own


def test_torch_save_carries_no_runtime_state(tmp_path):
    m = _model()
    _runtime_leftovers(m)
    torch.save(m, tmp_path / "m.pt")
    _check_copy(m, torch.load(tmp_path / "m.pt", weights_only=False))


def test_flat_storage_is_never_copied_or_pickled():
    import pickle
    from msa_amd.flat import FlatParams
    f = FlatParams.__new__(FlatParams)
    assert copy.deepcopy(f) is None and pickle.loads(pickle.dumps(f)) is None
    p = torch.nn.Parameter(torch.zeros(3))
    p._mmb_flat = (f, 0)
    q = pickle.loads(pickle.dumps(p))
    assert q._mmb_flat == (None, 0) and getattr(copy.deepcopy(p), "_mmb_flat", None) is None


def test_an_unbacked_parameter_is_refused_by_the_optimizer():
    from msa_amd.optim import AdamW
    p = torch.nn.Parameter(torch.zeros(3))
    p._mmb_flat = (None, 0)                                               # as a pickled parameter arrives
    with pytest.raises(RuntimeError, match="not backed"):
        AdamW([p]).step()
