"""arap.FUSED_TAIL on the CPU seam (tests/cpu_kernels.py): the Python plumbing of the fused output tail as far as it reaches without
the device — when the fused forms step aside, that the flag changes no value, and what the models ask of their last block.  The
kernels themselves are tests/test_step_tail_gpu.py's."""
import numpy as np
import pytest
import torch

from helpers import deterministic_init


@pytest.fixture(autouse=True)
def _flag():
    from surfacenetworks_amd import arap

    yield
    arap.FUSED_TAIL = True


def _batch(kind):
    from surfacenetworks_amd import arap

    ds = arap.ClothSequences([(5, 5)] * 2, frames=arap.INPUT_FRAMES + arap.OUTPUT_FRAMES + 3, op_frames=3, seed=11, device="cpu",
                             model=kind)
    return ds.sample_batch(2, np.random.default_rng(1), seq_ids=np.arange(2))


def test_new_entry_points_are_declared_bound_and_plannable():
    import os
    import re

    from surfacenetworks_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sn_spmm.h")).read(), flags=re.S)
    table = open(os.path.join(root, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in ("sn_linear_fwd_frame_f32", "sn_masked_smooth_l1_fwdg_f32", "sn_masked_smooth_l1_bwdg_f32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
        assert f"SN_PLAN_FN({name})" in table and name in doc
    assert "sn_linear_fwd_frame_supported" in _lib.SIGNATURES and hasattr(_lib.load(), "sn_linear_fwd_frame_supported")


def test_the_frame_is_not_fused_off_the_device_or_for_inputs_that_want_a_gradient(cpu_kernels):
    from surfacenetworks_amd import arap, blocks
    from surfacenetworks_amd import utils_pt as U

    conv = deterministic_init(U.GraphConv1x1(128, 120, batch_norm="pre"), 3).train()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, 128, generator=g)
    inputs = torch.randn(2, 9, 6, generator=g)
    assert not blocks.elu_conv_frame_ok(conv, x, inputs[:, :, 3:])                       # CPU tensors
    assert not U.elu_conv1x1_frame_ok(conv, x, inputs.clone().requires_grad_(True)[:, :, 3:])
    with pytest.raises(ValueError):
        U.elu_conv1x1(conv, x, inputs[:, :, 3:])                                         # asked for without asking first
    got = arap._predict(conv, x, inputs)
    want = arap._add_last_frame(U.elu_conv1x1(conv, x), inputs, arap.OUTPUT_FRAMES)
    assert got.shape == (2, 9, 120) and torch.equal(got, want)


@pytest.mark.parametrize("kind", ["dir", "lap"])
def test_the_flag_changes_no_value_on_the_seam(cpu_kernels, kind, monkeypatch):
    """One step of each model with the flag on and off: same loss, output and gradients; the Dirac model asks only its LAST block
    to leave v unwritten, and only with the flag on; the loss stays on the seam's two kernels (no device: no one-pass form)."""
    from surfacenetworks_amd import arap, blocks

    need_v = []
    real_block = blocks.dirac_block

    def block(mod, Di, DiA, v, f, need_f=True, num_faces=None, avg_next=None, need_v_=True):
        need_v.append(need_v_)
        return real_block(mod, Di, DiA, v, f, need_f, num_faces, avg_next, need_v_)

    monkeypatch.setattr(blocks, "dirac_block", block)
    batch = _batch(kind)
    res = {}
    for fused in (True, False):
        arap.FUSED_TAIL = fused
        need_v.clear()
        model = deterministic_init(arap.DirModel() if kind == "dir" else arap.Model(), 7).train()
        loss, out = arap.forward_loss(model, batch, 2)
        loss.backward()
        res[fused] = [loss.detach(), out.detach()] + [p.grad.clone() for p in model.parameters()]
        if kind == "dir":
            assert need_v == ([True] * 7 + [False] if fused else [True] * 8)
    assert bool(torch.isfinite(res[True][1]).all())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_the_unwritten_vertex_output_is_a_nan_placeholder_only_elu_conv_reads(cpu_kernels):
    from surfacenetworks_amd import arap, blocks
    from surfacenetworks_amd import utils_pt as U

    batch = _batch("dir")
    blk = deterministic_init(U.DirResNet2(128), 5).train()
    conv = deterministic_init(U.GraphConv1x1(128, 120, batch_norm="pre"), 3).train()
    v = torch.randn(2, batch.inputs.shape[1], 128, generator=torch.Generator().manual_seed(1))
    nf = arap._num_faces(batch.Di, batch.DiA, 2)
    vo, _ = blk(batch.Di, batch.DiA, v, None, f_out_needed=False, num_faces=nf, avg_next=False, v_out_needed=False)
    assert vo.shape == v.shape and blocks._unwritten(vo) and bool(torch.isnan(vo + 0).all())
    y = U.elu_conv1x1(conv, vo)
    assert bool(torch.isfinite(y).all())
    with pytest.raises(RuntimeError, match="placeholder"):
        U.elu_conv1x1(conv, vo)
    full, _ = blk(batch.Di, batch.DiA, v, None, f_out_needed=False, num_faces=nf, avg_next=False)
    assert not blocks._unwritten(full) and bool(torch.isfinite(full).all())


def test_the_loss_allocates_its_gradient_only_on_the_device(cpu_kernels, monkeypatch):
    from surfacenetworks_amd import arap, kernels

    def never(*a, **k):
        raise AssertionError("the one-pass loss has no host twin: CPU tensors keep the two kernels")

    monkeypatch.setattr(kernels, "masked_smooth_l1_fwdg", never)
    g = torch.Generator().manual_seed(2)
    out = torch.randn(2, 9, 120, generator=g).requires_grad_(True)
    tgt = torch.randn(2, 9, 120, generator=g)
    mask = (torch.rand(2, 9, 1, generator=g) < 0.7).float()
    loss = arap.loss_fn(out, tgt, mask, 2)
    loss.backward()
    ref = out.detach().clone().requires_grad_(True)
    want = torch.nn.functional.smooth_l1_loss(ref * mask, tgt, reduction="sum") / 2
    want.backward()
    assert torch.allclose(loss, want, rtol=1e-5) and torch.allclose(out.grad, ref.grad, rtol=1e-5, atol=1e-7)
