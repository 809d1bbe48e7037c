"""Normal prediction, host side (no GPU): the product's model classes against the reference's own (loaded from the reference
checkout where there is one), the float64 restatements the GPU tests use as their oracle against those same classes, the
reference statements of the loss and the metric against an independent evaluation, the analytic gradient of the definition
against autograd, the refused options, and the binding of the new entry points."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import normal_cases as nc
from helpers import deterministic_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"


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


def _pairs(ref, layers):
    from surfacenetworks_amd import normal_predict as NP

    return {"lap": (NP.LapDeepModel(3, 3, layers=layers), ref.LapDeepModel(3, 3, layers=layers), nc.RefLapDeep(3, 3, layers)),
            "dir": (NP.DirDeepModel(3, 3, layers=layers), ref.DirDeepModel(3, 3, layers=layers), nc.RefDirDeep(3, 3, layers)),
            "avg": (NP.AvgModel(3, 3, layers), ref.AvgModel(3, 3, layers), nc.RefAvg(3, 3, layers))}


@pytest.mark.parametrize("layers", [15, 3])
def test_state_dict_schema_equals_the_reference(ref_normal, layers):
    for kind, (mine, theirs, restated) in _pairs(ref_normal, layers).items():
        a, b, c = mine.state_dict(), theirs.state_dict(), restated.state_dict()
        assert list(a) == list(b) == list(c), kind
        assert all(a[k].shape == b[k].shape == c[k].shape for k in a), kind
        assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in theirs.parameters()), kind
        assert a["conv2.fc.weight"].shape == (3, 128) and a["conv2.fc.bias"].shape == (3,)


@pytest.mark.parametrize("kind", ["lap", "dir", "avg"])
def test_float64_restatement_is_the_reference_arithmetic(ref_normal, kind):
    """The oracle of the GPU tests (tests/normal_cases.py) against the reference's classes, float64, same weights, two padded
    batches: <= 1e-12 relative, outputs and every parameter gradient."""
    for sizes, seed in ((((5, 4), (6, 5)), 3), (((4, 4), (7, 3)), 5)):
        op, mask, inputs, targets, _, _ = nc.two_mesh_batch(kind, torch.float64, sizes, seed)
        _, theirs, restated = _pairs(ref_normal, 3)[kind]
        theirs = deterministic_init(theirs, 41).double().train()
        restated.load_state_dict(theirs.state_dict())
        restated = restated.double().train()
        outs = []
        for m in (theirs, restated):
            out = m(op, mask, inputs)
            (out * targets).sum().backward()
            outs.append(out.detach())
        scale = float(outs[0].abs().max())
        assert float((outs[0] - outs[1]).abs().max()) <= 1e-12 * scale
        for (k, p), (_, q) in zip(theirs.named_parameters(), restated.named_parameters()):
            assert float((p.grad - q.grad).abs().max()) <= 1e-12 * max(float(p.grad.abs().max()), 1e-30), (kind, k)


def _independent(outputs, mask, targets):
    """loss and mad of train_4_normal.py:113-123 with numpy in float64, row by row."""
    o, t = outputs.double().numpy().reshape(-1, 3), targets.double().numpy().reshape(-1, 3)
    keep = mask.numpy().reshape(-1) != 0
    ls, as_ = [], []
    for r in np.flatnonzero(keep):
        u = o[r] / max(np.sqrt((o[r] ** 2).sum()), 1e-12)
        c = float((u * t[r]).sum())
        ls.append(1 - c * c)
        as_.append(np.arccos(min(abs(c), 1.0)))
    return np.mean(ls), np.mean(as_)


def _cpu_case(seed, dtype):
    y, t, _ = nc.planted_rows(24, seed)
    mask = torch.ones(2, 12, 1)
    mask[0, 9:] = 0
    mask[1, 7:] = 0
    return y.reshape(2, 12, 3).to(dtype), mask, t.reshape(2, 12, 3).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_reference_statements_equal_an_independent_evaluation(dtype):
    from surfacenetworks_amd import normal_predict as NP

    outputs, mask, targets = _cpu_case(7, dtype)
    want_l, want_a = _independent(outputs, mask, targets)
    tol = 1e-13 if dtype == torch.float64 else 2e-6
    assert abs(float(NP.loss_reference(outputs, mask, targets)) - want_l) <= tol
    assert abs(float(NP.mad_reference(outputs, mask, targets)) - want_a) <= tol
    # CPU tensors and other dtypes: the public functions ARE the reference statements
    assert float(NP.cosine_loss(outputs, mask, targets)) == float(NP.loss_reference(outputs, mask, targets))
    assert float(NP.mean_angle_deviation(outputs, mask, targets)) == float(NP.mad_reference(outputs, mask, targets))
    l2, a2 = NP.loss_and_mad(outputs, mask, targets)
    assert float(l2) == float(NP.loss_reference(outputs, mask, targets)) and float(a2) == float(NP.mad_reference(outputs, mask, targets))


def test_the_reference_byte_mask_is_refused_by_this_torch():
    """The finding behind `.bool()`: train_4_normal.py:117 as written."""
    l = torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="(?i)bool"):
        torch.masked_select(l, torch.ones(2, 3).byte())


def test_analytic_gradient_equals_autograd_of_the_reference_statement():
    """Zero row, a row below the 1e-12 norm, rows exactly parallel and anti-parallel to the target, scaled rows, masked rows."""
    from surfacenetworks_amd import normal_predict as NP

    outputs, mask, targets = _cpu_case(9, torch.float64)
    outputs.requires_grad_(True)
    NP.loss_reference(outputs, mask, targets).backward()
    want = nc.analytic_gradient(outputs.detach(), mask, targets)
    got = outputs.grad
    assert torch.equal(got[mask.expand_as(got) == 0], torch.zeros_like(got[mask.expand_as(got) == 0]))
    scale = nc.cos_truth(outputs.detach().reshape(-1, 3), targets.reshape(-1, 3), mask.reshape(-1))["g_scale"].reshape(2, 12, 3)
    assert bool(((got - want).abs() <= 1e-13 * scale + 1e-300).all()), float(((got - want).abs() / (scale + 1e-300)).max())
    assert float(want[0, 0].abs().max()) == 0.0                      # the zero row: c = 0
    assert float(want[0, 2].abs().max()) <= 1e-15 and float(want[0, 3].abs().max()) <= 1e-15      # |c| = 1: t - c u = 0
    assert float(want[0, 1].abs().max()) > 1e9                       # below the clamp: divided by 1e-12, not by the norm


def test_device_functions_refuse_cpu_tensors():
    from surfacenetworks_amd import kernels

    y, t = torch.zeros(4, 3), torch.zeros(4, 3)
    for call in (lambda: kernels.normal_cosine_fwd(y, t), lambda: kernels.normal_cosine_fwdg(y, t),
                 lambda: kernels.normal_cosine_bwd(y, t, None, None, torch.zeros(3), torch.ones(1))):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()


def test_refused_options_raise():
    from surfacenetworks_amd import normal_predict as NP

    for make in (lambda: NP.LapDeepModel(bottleneck=True, layers=16), lambda: NP.LapDeepModel(nofirstId=True),
                 lambda: NP.LapDeepModel(bnmode=None), lambda: NP.LapDeepModel(bnmode="group"), lambda: NP.GatDeepModel(),
                 lambda: NP.EfficientCascade(), lambda: NP.LapMATModel()):
        with pytest.raises(NotImplementedError, match="normal_predict"):
            make()


def test_repeating_expand_and_schedule_and_optimizers():
    from surfacenetworks_amd import normal_predict as NP

    for n in (1, 2, 3, 4, 100):
        x = torch.randn(2, 5, n)
        assert torch.equal(NP.repeating_expand(x, 3), nc.repeating_expand(x, 3))
    m = NP.AvgModel(3, 3, 1)
    opt = NP.make_optimizer(m, lr=0.25, optimizer="sgd")
    assert opt.defaults["momentum"] == 0.9 and opt.defaults["weight_decay"] == 1e-5 and opt.defaults["lr"] == 0.25
    adam = NP.make_optimizer(m, amsgrad=True)
    assert adam.defaults["amsgrad"] and adam.defaults["lr"] == 1e-3 and adam.defaults["weight_decay"] == 0
    assert not NP.halve_lr(opt, 100, 10) and not NP.halve_lr(opt, 105, 10) and not NP.halve_lr(opt, 110, -1)
    assert NP.halve_lr(opt, 110, 10) and opt.param_groups[0]["lr"] == 0.125


def test_fuzzy_load_keeps_what_does_not_fit():
    from surfacenetworks_amd import normal_predict as NP

    m = deterministic_init(NP.LapDeepModel(layers=1), 3)
    before = m.conv2.fc.weight.detach().clone()
    sd = {k: torch.full_like(v, 2.0) for k, v in deterministic_init(NP.LapDeepModel(layers=1), 4).state_dict().items()}
    sd["conv2.fc.weight"] = torch.zeros(120, 128)            # another head: skipped by LapDeepModel.fuzzy_load (models.py:81)
    sd["not.a.key"] = torch.zeros(1)
    m.fuzzy_load(sd)
    assert torch.equal(m.conv2.fc.weight, before) and float(m.conv1.fc.weight.detach().min()) == 2.0


def test_new_entry_points_are_declared_bound_and_plannable():
    from surfacenetworks_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sn_spmm.h")).read(), flags=re.S)
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in ("sn_normal_cosine_fwd_f32", "sn_normal_cosine_fwdg_f32", "sn_normal_cosine_bwd_f32", "sn_normal_cosine_bwdg_f32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
        assert f"SN_PLAN_FN({name})" in table and name in doc
    assert int(lib.sn_normal_cosine_grid_rows()) == 1024 * 256
    assert int(lib.sn_normal_cosine_workspace_bytes(10)) >= 3 * 1024 * 8
    full = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    assert "Normal prediction" in full and "Replaces: src/normal_predict/train_4_normal.py:113-123" in full
