"""The cascade model, host side (no GPU): the product's class and the float64 restatement the GPU tests use as their oracle
(tests/cascade_cases.py) against the reference's own `EfficientCascade` (loaded from the reference checkout where there is
one), the refused options, the batch field, the argument checks, and the binding of the new entry points."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import cascade_cases as cc
from helpers import deterministic_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"
POOL_ENTRIES = ("sn_pool_max2_fwd_f32", "sn_pool_max2_bwd_f32", "sn_unpool2_add_fwd_f32", "sn_unpool2_bwd_f32")


@pytest.fixture
def ref_normal(monkeypatch):
    """The reference's normal_predict/models.py on the reference's OWN utils_pt (no import swap)."""
    path = os.path.join(REF_SRC, "normal_predict", "models.py")
    if not os.path.exists(path):
        pytest.skip("no reference checkout on this machine")
    monkeypatch.setattr(sys, "dont_write_bytecode", True)        # (the reference mount is read-only)
    monkeypatch.syspath_prepend(REF_SRC)
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        monkeypatch.delitem(sys.modules, k)
    spec = importlib.util.spec_from_file_location("ref_normal_predict_models", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.utils.__file__) == os.path.realpath(os.path.join(REF_SRC, "utils", "utils_pt.py"))
    yield mod
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        monkeypatch.delitem(sys.modules, k, raising=False)


@pytest.mark.parametrize("levels", [4, 2, 1])
def test_state_dict_schema_equals_the_reference(ref_normal, levels):
    from surfacenetworks_amd import cascade

    mine = cascade.LapCascade(3, 3, cascade_levels=levels)
    theirs = ref_normal.EfficientCascade(3, 3, cascade_levels=levels)
    restated = cc.RefCascade(3, 3, levels)
    a, b, c = mine.state_dict(), theirs.state_dict(), restated.state_dict()
    assert list(a) == list(b) == list(c)
    assert all(a[k].shape == b[k].shape == c[k].shape for k in a)
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in theirs.parameters())
    assert a["conv2.fc.weight"].shape == (3, 128) and a["conv1.fc.weight"].shape == (128, 3)


def test_state_dict_keys_without_a_reference_checkout():
    """The key list written out (models.py:535-566: conv1, down_rn3..1, lap0, up_rn1..3, conv2; blocks of bn_fc0 / bn_fc1)."""
    from surfacenetworks_amd import cascade

    blocks = ["down_rn3", "down_rn2", "down_rn1", "lap0", "up_rn1", "up_rn2", "up_rn3"]
    want = ["conv1.fc.weight", "conv1.fc.bias"]
    for blk in blocks:
        for st in ("bn_fc0", "bn_fc1"):
            want += [f"{blk}.{st}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
            want += [f"{blk}.{st}.fc.weight", f"{blk}.{st}.fc.bias"]
    want += [f"conv2.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    want += ["conv2.fc.weight", "conv2.fc.bias"]
    for model in (cascade.LapCascade(), cc.RefCascade()):
        sd = model.state_dict()
        assert list(sd) == want
        assert sd["down_rn3.bn_fc0.fc.weight"].shape == (128, 256) and sd["lap0.bn_fc1.bn.running_var"].shape == (256,)


def _close64(ms, runs, case):
    outs = []
    for m, Laps in zip(ms, runs):
        out = m(Laps, case["mask"].double(), case["inputs"].double())
        (out * case["targets"].double()).sum().backward()
        outs.append(out.detach())
    assert outs[0].shape == (2, case["V"], 3)
    assert float((outs[0] - outs[1]).abs().max()) <= 1e-12 * float(outs[0].abs().max())
    for (k, p), (_, q) in zip(ms[0].named_parameters(), ms[1].named_parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 1e-12 * max(float(p.grad.abs().max()), 1e-30), k


@pytest.mark.parametrize("levels", [4, 2])
def test_float64_restatement_is_the_reference_arithmetic(ref_normal, levels):
    """The oracle of the GPU tests against the reference's class, float64, same weights, dense (B, V_k, V_k) Laps: <= 1e-12
    relative, outputs and every parameter gradient.  (With sparse Laps the reference's own block stops at the transposed view
    its pooling returns — `x.view(-1, feat)`, models.py:470 — so the dense form is the one it can be asked.)"""
    case = cc.cascade_batch(levels, sizes=((5, 4), (6, 5)))
    Laps = cc.host_operators(case, torch.float64, dense=True)
    theirs = deterministic_init(ref_normal.EfficientCascade(3, 3, cascade_levels=levels), 41).double().train()
    restated = cc.RefCascade(3, 3, levels)
    restated.load_state_dict(theirs.state_dict())
    _close64((theirs, restated.double().train()), (Laps, Laps), case)


def test_restatement_on_sparse_operators_equals_the_dense_run():
    """What the GPU tests feed the oracle — block-diagonal sparse Laps — against the dense (B, V_k, V_k) run above.  A check of
    the oracle itself: it runs nothing of the product and passes without it."""
    case = cc.cascade_batch(4, sizes=((5, 4), (6, 5)))
    a = deterministic_init(cc.RefCascade(3, 3, 4), 41).double().train()
    b = deterministic_init(cc.RefCascade(3, 3, 4), 41).double().train()
    _close64((a, b), (cc.host_operators(case, torch.float64, dense=True), cc.host_operators(case, torch.float64)), case)


def test_torch_pooling_forms_are_the_reference_modules(ref_normal):
    x = torch.randn(2, 6, 5, dtype=torch.float64)
    skip = torch.randn(2, 12, 5, dtype=torch.float64)
    P = ref_normal.EfficientCascade._Pooling
    assert torch.equal(cc.torch_pool(skip), P(down=True)(None, skip))
    assert torch.equal(cc.torch_unpool_add(x, skip), P(down=False)(None, x) + skip)


def test_pair_levels_are_a_hierarchy():
    """Empty rows and columns at padded nodes, sizes n_0 2^k, every coarse entry the halved sum over its 2 x 2 block of children,
    zero row sums up to rounding (the cloth Laplacian's rows sum to zero).  A check of the test fixture itself: it runs nothing
    of the product and passes without it."""
    case = cc.cascade_batch(4)
    assert case["V"] % 8 == 0 and case["V"] >= max(case["nv"])
    m = case["mask"][:, :, 0]
    assert all(int(m[b].sum()) == case["nv"][b] and not bool(m[b, :case["nv"][b]].all()) for b in range(2))      # no prefix
    for pm, nv in zip(case["per_mesh"], case["nv"]):
        assert [M.shape[0] for M in pm] == [case["V"] >> (3 - k) for k in range(4)]
        fine = pm[3].toarray().astype(np.float64)
        fake = np.setdiff1d(np.arange(case["V"]), case["position"][case["nv"].index(nv)])
        assert len(fake) == case["V"] - nv and not fine[fake].any() and not fine[:, fake].any()
        for k in (3, 2, 1):
            f = pm[k].toarray().astype(np.float64)
            n = f.shape[0] // 2
            want = 0.5 * f.reshape(n, 2, n, 2).sum(axis=(1, 3))
            got = pm[k - 1].toarray().astype(np.float64)
            assert np.abs(got - want).max() <= 2.0 ** -23 * max(np.abs(want).max(), 1e-30)
            assert np.abs(got.sum(1)).max() <= 1e-4 * np.abs(got).max()
    for k, M in enumerate(case["Laps"]):
        assert M.shape == (2 * (case["V"] >> (3 - k)),) * 2 and M.dtype == np.float32 and M.has_sorted_indices


def test_refused_options_raise():
    from surfacenetworks_amd import cascade
    from surfacenetworks_amd import normal_predict as NP

    for make in (lambda: cascade.LapCascade(bottleneck=True), lambda: cascade.LapCascade(naive_pool=False),
                 lambda: cascade.LapCascade(inner_layers=1), lambda: cascade.LapCascade(inner_layers=3),
                 lambda: cascade.LapCascade(bnmode=None), lambda: cascade.LapCascade(bnmode="group"),
                 lambda: cascade.LapCascade(out_features=4)):
        with pytest.raises(NotImplementedError, match="cascade.LapCascade"):
            make()
    with pytest.raises(ValueError):
        cascade.LapCascade(cascade_levels=0)
    cascade.LapCascade(with_avg=True)                                # accepted and unused, as in the reference
    assert "avg" not in "".join(cascade.LapCascade(with_avg=True).state_dict())
    with pytest.raises(NotImplementedError, match=r"cascade\.LapCascade"):       # the stub names the model that is built
        NP.EfficientCascade()


def test_batch_carries_the_level_operators():
    from surfacenetworks_amd import normal_predict as NP

    t = torch.zeros(1, 2, 3)
    b = NP.Batch(t, t, t[:, :, :1], "L", None, None, [0])
    assert b.Laps is None and b.operator == "L"                       # existing construction is unchanged
    assert NP.Batch(t, t, t[:, :, :1], None, "Di", "DiA", [0]).operator == ("Di", "DiA")
    laps = ["L0", "L1"]
    assert NP.Batch(t, t, t[:, :, :1], None, None, None, [0], Laps=laps).operator is laps


def test_argument_checks_precede_any_launch():
    """The wrong number of operators, a node count that the levels do not divide, an operator of the wrong size: ValueError
    before anything is computed (CPU tensors never reach a kernel)."""
    from surfacenetworks_amd import cascade

    class Op:
        def __init__(self, n):
            self.shape = (n, n)

    model = cascade.LapCascade(cascade_levels=3)
    x = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="3 operators"):
        model([Op(4), Op(8)], None, x)
    with pytest.raises(ValueError, match="multiple of 2\\^2"):
        model([Op(4), Op(8), Op(12)], None, torch.zeros(2, 6, 3))
    with pytest.raises(ValueError, match=r"Laps\[1\]"):
        model([Op(4), Op(9), Op(16)], None, x)


def test_pooling_refuses_cpu_tensors_and_bad_shapes():
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd import kernels

    x = torch.zeros(1, 4, 4)
    for call in (lambda: snF.pool_max2(x), lambda: snF.unpool2_add(x[:, :2], x), lambda: kernels.pool_max2_bwd(x, x[:, :2]),
                 lambda: kernels.unpool2_bwd(x)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
    with pytest.raises(ValueError, match="even"):
        snF.pool_max2(torch.zeros(1, 3, 4))


def test_new_entry_points_are_declared_and_bound():
    from surfacenetworks_amd import _lib

    full = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in POOL_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in doc, name
    assert "Sibling-pair pooling" in full and "Replaces: src/normal_predict/models.py:568-576" in full
    # argument errors come back as status codes, before any launch (no device needed)
    assert lib.sn_pool_max2_fwd_f32(None, 4, -1, 4, None, 4, None) == -2            # SN_E_SHAPE
    assert lib.sn_pool_max2_fwd_f32(None, 3, 1, 4, None, 4, None) == -2             # ld < C
    assert lib.sn_unpool2_bwd_f32(None, 4, 1, 0, None, 4, None) == -2               # C < 1
    assert lib.sn_pool_max2_bwd_f32(None, 4, None, 4, 1, 4, None, 4, None) == -1    # SN_E_NULL
    assert lib.sn_unpool2_add_fwd_f32(None, 4, None, 4, 0, 4, None, 4, None) == 0   # nothing to do
