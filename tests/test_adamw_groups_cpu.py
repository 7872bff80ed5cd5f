"""CPU tests of per-parameter-group AdamW: optim.layerwise_param_groups (coverage, exponents, the reference's two groups at the defaults),
the trainer hook, the slot de-duplication and its limits, the per-group keys that are refused, the warm-up schedule per group, and the
ISA guard of the grouped kernel."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(layers, hidden=32):
    from msa_amd.model import MMBertConfig, MMBertForPretraining
    m = MMBertForPretraining(MMBertConfig(vocab_size=128, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=2,
                                          intermediate_size=2 * hidden))
    m.bert.set_joint_embeddings("mosei")
    return m


def _per_param(groups):
    """{id(param): (lr, weight_decay)}; every parameter exactly once"""
    out = {}
    for g in groups:
        for p in g["params"]:
            assert id(p) not in out
            out[id(p)] = (g.get("initial_lr", g.get("lr")), g["weight_decay"])
    return out


@pytest.mark.parametrize("L", [2, 24])
def test_layerwise_groups_cover_every_parameter_once_with_the_right_exponent(L):
    from msa_amd.optim import layerwise_param_groups
    m = _model(L)
    lr, d, head = 1e-3, 0.9, 7e-3
    groups = layerwise_param_groups(m, lr, weight_decay=0.02, layer_decay=d, head_lr=head)
    pp = _per_param(groups)
    named = list(m.named_parameters())
    assert len(pp) == len(named)
    for n, p in named:
        glr, wd = pp[id(p)]
        assert wd == (0.0 if any(k in n for k in ("bias", "LayerNorm.bias", "LayerNorm.weight")) else 0.02), n
        if n.startswith("bert.encoder.layer."):
            i = int(n.split(".")[3])
            assert glr == lr * d ** (L - i), n
        elif n.startswith("bert.embeddings."):
            assert glr == lr * d ** (L + 1), n
        elif n.startswith("bert.pooler."):
            assert glr == lr, n
        else:
            assert n.startswith(("bert.jointEmbeddings.", "cls.", "classifier1_", "attn.", "vt.", "vv.", "vs.", "cpc_")), n
            assert glr == head, n
    assert len({g["lr"] for g in groups}) == L + 3                     # L layers, embeddings, pooler, head
    assert all(g["params"] for g in groups)


def test_layerwise_defaults_reproduce_the_reference_groups():
    from msa_amd import trainer as T
    from msa_amd.optim import AdamW, layerwise_param_groups
    m = _model(2)
    ref, _ = T.build_optimizer(m, T.default_args(learning_rate=3e-4), 10)
    groups = layerwise_param_groups(m, 3e-4)
    assert len(groups) == 2
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
    assert _per_param(groups) == _per_param(ref.param_groups)
    opt = AdamW(groups, lr=3e-4)
    assert [(g["betas"], g["eps"]) for g in opt.param_groups] == [(g["betas"], g["eps"]) for g in ref.param_groups]


def test_build_optimizer_uses_the_layerwise_groups_only_when_asked():
    from msa_amd import trainer as T
    m = _model(2)
    assert not hasattr(T.default_args(), "layer_lr_decay") and not hasattr(T.default_args(), "head_learning_rate")
    plain, _ = T.build_optimizer(m, T.default_args(learning_rate=1e-3), 10)
    assert len(plain.param_groups) == 2
    opt, sched = T.build_optimizer(m, T.default_args(learning_rate=1e-3, layer_lr_decay=0.5, head_learning_rate=1e-2), 10)
    pp = _per_param(opt.param_groups)
    assert pp[id(m.bert.encoder.layer[0].intermediate.dense.weight)] == (1e-3 * 0.25, 0.01)
    assert pp[id(m.bert.embeddings.word_embeddings.weight)] == (1e-3 * 0.125, 0.01)
    assert pp[id(m.cpc_zt.net.weight)] == (1e-2, 0.01)
    assert pp[id(m.bert.pooler.dense.bias)] == (1e-3, 0.0)
    only_head, _ = T.build_optimizer(m, T.default_args(learning_rate=1e-3, head_learning_rate=1e-2), 10)
    assert {v[0] for v in _per_param(only_head.param_groups).values()} == {1e-3, 1e-2}


def test_warmup_schedule_scales_each_groups_own_initial_lr():
    from msa_amd.optim import AdamW, LinearWarmupSchedule
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = AdamW([{"params": [a], "lr": 1e-3}, {"params": [b], "lr": 4e-5}], lr=1.0)
    sched = LinearWarmupSchedule(opt, 4, 8)
    assert opt.param_groups[0]["lr"] == 0.0 and opt.param_groups[1]["lr"] == 0.0
    for k in range(1, 8):
        sched.step()
        lam = k / 4 if k < 4 else (8 - k) / 4
        assert sched.get_last_lr() == [1e-3 * lam, 4e-5 * lam]


def test_slot_deduplication_and_limits():
    from msa_amd import ops
    from msa_amd.optim import adamw_slots
    a, b, c = (1e-3, 0.9, 0.999, 1e-6, 0.01), (1e-3, 0.9, 0.999, 1e-6, 0.0), (2e-3, 0.8, 0.99, 1e-8, 0.01)
    assert adamw_slots([a, b, a, c, b]) == ([0, 1, 0, 2, 1], [a, b, c])
    assert adamw_slots([a]) == ([0], [a])
    assert ops.ADAMW_MAX_GROUPS == 255 and ops.ADAMW_MAX_SLOTS == 64
    distinct = [(1e-4 * (k + 1), 0.9, 0.999, 1e-6, 0.0) for k in range(64)]
    slots, keys = adamw_slots(distinct + distinct[:10] * 19)                # 64 distinct in 254 groups
    assert len(keys) == 64 and slots[-1] == 9
    assert len(adamw_slots([a] * 255)[0]) == 255
    with pytest.raises(NotImplementedError, match="merge"):
        adamw_slots(distinct + [(5.0, 0.9, 0.999, 1e-6, 0.0)])              # 65 distinct
    with pytest.raises(NotImplementedError, match="merge"):
        adamw_slots([a] * 256)                                               # 256 groups
    # the header's limits are the ones the Python side enforces
    text = open(os.path.join(ROOT, "include", "mmbert_hip.h")).read()
    assert "#define MMBERT_ADAMW_MAX_GROUPS 255" in text and "#define MMBERT_ADAMW_MAX_SLOTS 64" in text


@pytest.mark.parametrize("key,value", [("amsgrad", True), ("maximize", True), ("correct_bias", False)])
def test_unimplemented_per_group_keys_are_refused(key, value):
    from msa_amd.optim import AdamW
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = AdamW([{"params": [a]}, {"params": [b], key: value}])
    with pytest.raises(NotImplementedError, match=key):
        opt.step()                                                           # (refused before the optimizer binds to a storage)
    assert opt._steps == 0 and opt._flat is None
    ok = AdamW([{"params": [a]}, {"params": [b], key: not value}])
    assert ok._hyper() == [(1e-3, 0.9, 0.999, 1e-6, 0.0)] * 2


def test_groups_carry_their_own_betas_and_eps():
    from msa_amd.optim import AdamW
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    opt = AdamW([{"params": [a]}, {"params": [b], "betas": (0.8, 0.99), "eps": 1e-8, "lr": 5e-3, "weight_decay": 0.1}],
                lr=1e-3, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.01)
    assert opt._hyper() == [(1e-3, 0.9, 0.98, 1e-7, 0.01), (5e-3, 0.8, 0.99, 1e-8, 0.1)]
    opt.param_groups[0]["lr"] = 2e-3                                         # read afresh at every step
    assert opt._hyper()[0][0] == 2e-3


def test_grouped_kernel_loads_stay_in_flight():
    """ISA guard (the scan of tests/test_isa_cpu.py): adamw_grouped_kernel, both forms, has no more serialized loads than adamw_kernel,
    no scratch, and no more VGPRs than adamw_kernel."""
    import subprocess
    import tempfile
    if not os.path.exists("/opt/rocm/bin/hipcc") and not os.environ.get("HIPCC"):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("scan_serialized_loads", os.path.join(ROOT, "tools", "scan_serialized_loads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t = mod.scan_source("rowwise.hip")
    (base,) = [v for k, v in t.items() if k.startswith("adamw_kernel") or k.startswith("_Z12adamw_kernel")]
    grouped = [v for k, v in t.items() if "adamw_grouped_kernel" in k]
    assert len(grouped) == 2
    for loads, drains, serialized in grouped:
        assert loads > 0 and serialized <= base[2], (loads, drains, serialized, base)
    # registers: the same budget as adamw_kernel (the coefficients live in SGPRs)
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([mod.HIPCC, *[f for f in mod.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only", "-o", os.path.join(td, "r.s"),
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(mod.SRC_DIR, "rowwise.hip")],
                           capture_output=True, text=True, check=True)
    usage, name = {}, None
    for line in r.stderr.split("\n"):
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split("[")[0].strip()
        elif name and ("VGPRs:" in line or "ScratchSize" in line):
            usage.setdefault(name, {})["vgpr" if "VGPRs:" in line else "scratch"] = int(line.split(":")[-1].split("[")[0])
    base_u = [u for k, u in usage.items() if k.startswith("_Z12adamw_kernel")][0]
    grouped_u = [u for k, u in usage.items() if "adamw_grouped_kernel" in k]
    assert len(grouped_u) == 2
    for u in grouped_u:
        assert u["scratch"] == 0 and u["vgpr"] <= base_u["vgpr"], (u, base_u)
