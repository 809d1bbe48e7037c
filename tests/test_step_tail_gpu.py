"""The output end of the ARAP step without the passes its result does not need (arap.FUSED_TAIL): the last-frame residual added in
the last GEMM's store (sn_linear_fwd_frame_f32), the loss gradient written by the loss pass (sn_masked_smooth_l1_fwdg_f32 /
_bwdg_f32), the last Dirac block's pre-activation vertex output not written.  Every part is built to give the bits of the unfused
composition, which stays the fallback and is the oracle here: all comparisons are torch.equal."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

from helpers import _arena, _outside_untouched  # noqa: E402
from surfacenetworks_amd import _lib, arap, blocks, kernels, mesh_ops, plans  # noqa: E402
from surfacenetworks_amd import utils_pt as U  # noqa: E402
from surfacenetworks_amd.kernels import _ld, _p, _stream  # noqa: E402
from surfacenetworks_amd.operators import SparseOperator  # noqa: E402

CANARY = 7.0


@pytest.fixture(autouse=True)
def _clean():
    plans.reset()
    plans.set_enabled(True)
    yield
    arap.FUSED_TAIL = True
    plans.set_enabled(True)
    kernels.clear_absmax()


# ---- the frame epilogue --------------------------------------------------------------------------------------------------------------
# 1 / 31 / 33 / 97 rows: either side of the 32-row tile, a ragged last tile; 16 481 = 515 tiles + 1 row: more tiles than the largest
# grid (2 workgroups on each of 256 compute units), so workgroups walk on to a second tile with every window advanced
@pytest.mark.parametrize("rows", [1, 31, 33, 97, 16481])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("J", [120, 12])
def test_frame_epilogue_equals_gemm_then_broadcast_add(rows, K, J):
    assert kernels.linear_fwd_frame_supported(K, J)
    rng = np.random.default_rng(rows + K + J)
    W = torch.from_numpy((rng.standard_normal((J, K)) / np.sqrt(K)).astype(np.float32)).to(DEV)
    bias = torch.from_numpy(rng.standard_normal(J).astype(np.float32)).to(DEV)
    _, x = _arena(rows, K, seed=1)
    inputs = torch.from_numpy(rng.standard_normal((rows, 6)).astype(np.float32)).to(DEV)
    plain = kernels.linear_fwd(x, W, bias)
    want = arap._add_last_frame(plain.view(1, rows, J), inputs.view(1, rows, 6), J // 3).view(rows, J)
    assert bool(torch.isfinite(want).all())
    for nan_first in (False, True):
        inp = inputs.clone()
        if nan_first:
            inp[:, :3] = float("nan")            # the first input frame is not the kernel's to read
        frame = inp[:, 3:]                       # (rows, 3), row stride 6, 12 bytes past a 16-byte boundary
        ya, y = _arena(rows, J, fill=CANARY, values=torch.full((rows, J), CANARY))
        _lib.call("sn_linear_fwd_frame_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), _p(frame), _ld(frame) if rows > 1 else 6, _p(y),
                  _ld(y) if rows > 1 else J + 16, rows, K, J, _stream())
        assert _outside_untouched(ya, rows, J, CANARY), nan_first
        assert torch.equal(y, want), nan_first
        assert torch.equal(kernels.linear_fwd_frame(x, W, bias, frame), want), nan_first


def test_frame_epilogue_refuses_what_it_does_not_cover():
    x = torch.zeros(4, 128, device=DEV)
    W = torch.zeros(16, 128, device=DEV)
    b = torch.zeros(16, device=DEV)
    f = torch.zeros(4, 6, device=DEV)[:, 3:]
    assert not kernels.linear_fwd_frame_supported(128, 16) and not kernels.linear_fwd_frame_supported(64, 120)
    with pytest.raises(Exception):
        kernels.linear_fwd_frame(x, W, b, f)                                   # 16 outputs: no whole groups of twelve
    with pytest.raises(ValueError):
        kernels.linear_fwd_frame(x, W[:12], b[:12], torch.zeros(4, 4, device=DEV))


def _conv2(seed=3):
    from helpers import deterministic_init

    return deterministic_init(U.GraphConv1x1(128, 120, batch_norm="pre"), seed).to(DEV).train()


def test_inputs_that_want_a_gradient_take_the_unfused_add(monkeypatch):
    """arap._predict: fused for plain inputs (the frame launch runs, the result is the composition's); inputs.requires_grad takes
    elu_conv1x1 + _add_last_frame — same values — and the gradient reaches the inputs."""
    calls = []
    real = kernels.linear_fwd_frame
    monkeypatch.setattr(kernels, "linear_fwd_frame", lambda *a: (calls.append(1), real(*a))[1])
    plans.set_enabled(False)                     # (a replayed launch plan does not come through the Python launcher)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 37, 128, generator=g).to(DEV)
    inputs = torch.randn(2, 37, 6, generator=g).to(DEV)
    got = arap._predict(_conv2(), x, inputs)
    assert len(calls) == 1
    arap.FUSED_TAIL = False
    want = arap._predict(_conv2(), x, inputs)
    assert len(calls) == 1 and torch.equal(got, want)
    arap.FUSED_TAIL = True
    ig = inputs.clone().requires_grad_(True)
    again = arap._predict(_conv2(), x, ig)
    assert len(calls) == 1 and torch.equal(again, want)
    again.sum().backward()
    assert torch.equal(ig.grad[:, :, 3:], torch.full((2, 37, 3), 40.0, device=DEV)) and not bool(ig.grad[:, :, :3].any())
    with torch.no_grad():                                                        # (evaluation: fused whatever the flag says)
        assert torch.equal(arap._predict(_conv2(), x, ig), want) and len(calls) == 2
    # another dtype, a frame whose rows one 2-D view cannot address, a layer without whole groups of twelve: the torch add
    assert blocks.elu_conv_frame_ok(_conv2(), x, inputs[:, :, 3:])
    assert not blocks.elu_conv_frame_ok(_conv2(), x, inputs.double()[:, :, 3:])
    assert not blocks.elu_conv_frame_ok(_conv2(), x, torch.zeros(2, 40, 6, device=DEV)[:, :37, 3:])
    assert not blocks.elu_conv_frame_ok(U.GraphConv1x1(128, 16, batch_norm="pre").to(DEV), x, inputs[:, :, 3:])


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def _loss_operands(rows, C, seed, nonfinite):
    rng = np.random.default_rng(seed)
    out = (1.5 * rng.standard_normal((rows, C))).astype(np.float32)
    tgt = rng.standard_normal((rows, C)).astype(np.float32)
    mask = (rng.random(rows) < 0.7).astype(np.float32)
    if rows > 2:
        mask[1] = 0.0                                                            # rows the mask removes: the gradient is 0·…, the loss l(-t)
        mask[rows // 2] = 0.3                                                    # (not a 0/1 value: the product out·m rounds)
        mask[0] = 1.0
    else:
        mask[:] = 1.0
    one = np.float32(1.0)
    edge = [one, -one, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), -np.nextafter(one, np.float32(0)),
            -np.nextafter(one, np.float32(2))]
    for k, d in enumerate(edge[:C]):                                             # row 0, mask 1: out·m - tgt is exactly d
        tgt[0, k] = np.float32(0.0)
        out[0, k] = d
    if nonfinite:
        r = rows - 1
        out[r, 0], out[r, 1], out[r, 2] = np.inf, -np.inf, np.nan
        tgt[r, 3] = np.inf
    return [torch.from_numpy(a).to(DEV) for a in (out, tgt, mask)]


def _same(a, b):
    """torch.equal, with NaN equal to NaN (a loss over non-finite entries IS NaN, in both forms)."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("rows", [1, 7, 1025])
@pytest.mark.parametrize("C", [120, 6])
@pytest.mark.parametrize("nonfinite", [False, True])
def test_loss_with_gradient_equals_the_two_passes(rows, C, nonfinite):
    """sn_masked_smooth_l1_fwdg_f32: the loss of the forward kernel and the gradient of the backward kernel at gloss = 1;
    sn_masked_smooth_l1_bwdg_f32 over that buffer for gloss 1 / 0.5 / 3: the backward kernel's gradient.  120 columns: 16-byte items;
    6: single floats.  1025 rows: more than one workgroup and a ragged last one (at most one item per thread: the four-item groups
    are test_loss_with_gradient_on_many_items_per_thread's)."""
    out, tgt, mask = _loss_operands(rows, C, rows * C, nonfinite)
    scale = 1.0 / 3.0
    eq = _same if nonfinite else torch.equal
    for m in (mask, None):
        want_loss = kernels.masked_smooth_l1_fwd(out, tgt, m, scale)
        assert nonfinite or bool(torch.isfinite(want_loss))
        for gl in (1.0, 0.5, 3.0):
            gloss = torch.tensor(gl, device=DEV)
            want_g = kernels.masked_smooth_l1_bwd(out, tgt, m, scale, gloss)
            loss, g = kernels.masked_smooth_l1_fwdg(out, tgt, m, scale)
            assert eq(loss, want_loss), (gl, m is None)
            if gl == 1.0:
                assert eq(g, want_g)                                             # already final: the backward launch only looks at gloss
            got = kernels.masked_smooth_l1_bwdg(out, tgt, m, scale, gloss, g)
            assert got.data_ptr() == g.data_ptr() and eq(got, want_g), (gl, m is None)


@pytest.mark.parametrize("rows,C", [(65539, 120), (180001, 6)])
def test_loss_with_gradient_on_many_items_per_thread(rows, C):
    """More than 4 x 1024 x 256 items (16-byte items at 120 columns, single floats at 6): every thread runs a whole four-item group
    and the one-item tail, (row, column) carried across the grid stride."""
    g_ = torch.Generator().manual_seed(8)
    out = (1.5 * torch.randn(rows, C, generator=g_)).to(DEV)
    tgt = torch.randn(rows, C, generator=g_).to(DEV)
    mask = (torch.rand(rows, generator=g_) < 0.8).float().to(DEV)
    loss, g = kernels.masked_smooth_l1_fwdg(out, tgt, mask, 0.25)
    assert torch.equal(loss, kernels.masked_smooth_l1_fwd(out, tgt, mask, 0.25))
    assert torch.equal(g, kernels.masked_smooth_l1_bwd(out, tgt, mask, 0.25, torch.tensor(1.0, device=DEV)))


@pytest.mark.parametrize("gl", [1.0, 0.5, 3.0])
def test_loss_fn_gradients_do_not_depend_on_the_flag(gl):
    out, tgt, mask = _loss_operands(1025, 120, 5, False)
    res = {}
    for fused in (True, False):
        arap.FUSED_TAIL = fused
        o = out.view(5, 205, 120).clone().requires_grad_(True)
        loss = arap.loss_fn(o, tgt.view(5, 205, 120), mask.view(5, 205, 1), 5)
        (loss * gl).backward()
        res[fused] = (loss.detach().clone(), o.grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_no_gradient_buffer_without_a_backward(monkeypatch):
    """torch.no_grad(), and outputs that want no gradient: the read-only forward kernel, nothing of the gradient's size allocated."""
    out, tgt, mask = _loss_operands(1025, 120, 6, False)
    calls = []
    real = kernels.masked_smooth_l1_fwdg
    monkeypatch.setattr(kernels, "masked_smooth_l1_fwdg", lambda *a: (calls.append(1), real(*a))[1])
    o3, t3, m3 = out.view(5, 205, 120), tgt.view(5, 205, 120), mask.view(5, 205, 1)
    want = arap.loss_fn(o3.clone().requires_grad_(True), t3, m3, 5).detach()
    assert len(calls) == 1
    torch.cuda.synchronize()
    for ctx, o in ((torch.no_grad(), o3.clone().requires_grad_(True)), (torch.enable_grad(), o3)):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with ctx:
            loss = arap.loss_fn(o, t3, m3, 5)
        assert len(calls) == 1 and torch.equal(loss.detach(), want)
        assert torch.cuda.max_memory_allocated() - base < out.numel() * 4 // 2


# ---- the whole tail --------------------------------------------------------------------------------------------------------------------
def _snapshot(model, loss, out):
    return ([loss.detach().clone(), out.detach().clone()] + [p.grad.clone() for p in model.parameters()] +
            [b.clone() for b in model.buffers()] + [p.detach().clone() for p in model.parameters()])


def _tail_run(kind, fused, mode, steps):
    """`steps` training steps of a 2-mesh, 5 x 5-vertex batch from a fixed seed; per step the loss, the model output (of a forward
    pass after the update), every parameter gradient, every buffer, the updated parameters."""
    arap.FUSED_TAIL = fused
    plans.reset()
    plans.set_enabled(mode != "eager")
    torch.manual_seed(5)
    ds = arap.ClothSequences([(5, 5)] * 2, frames=arap.INPUT_FRAMES + arap.OUTPUT_FRAMES + 3, op_frames=3, seed=11, device=DEV,
                             model=kind)
    model = (arap.DirModel() if kind == "dir" else arap.Model()).to(DEV).train()
    opt = arap.make_optimizer(model)
    ids = np.arange(2)
    graphed = None
    if mode == "graph":
        graphed = arap.GraphedTrainStep(model, opt, ds.sample_batch(2, np.random.default_rng(0), seq_ids=ids), global_batch=2)
    rng = np.random.default_rng(1)
    snaps = []
    for _ in range(steps):
        batch = ds.sample_batch(2, rng, seq_ids=ids)
        loss = graphed(batch) if graphed is not None else arap.train_step(model, opt, batch, global_batch=2)
        with torch.no_grad():
            out = arap.forward_loss(model, batch, 2)[1]
        snaps.append(_snapshot(model, loss, out))
    return snaps


def _assert_same_runs(a, b, what):
    assert len(a) == len(b)
    for k, (sa, sb) in enumerate(zip(a, b)):
        assert len(sa) == len(sb)
        for i, (ta, tb) in enumerate(zip(sa, sb)):
            assert torch.equal(ta, tb), f"{what}: step {k}, tensor {i} differs"
        assert bool(torch.isfinite(sa[0])) and bool(torch.isfinite(sa[1]).all())


@pytest.mark.parametrize("mode,steps", [("eager", 2), ("plans", 3), ("graph", 3)])
def test_dirac_model_steps_do_not_depend_on_the_flag(mode, steps):
    _assert_same_runs(_tail_run("dir", True, mode, steps), _tail_run("dir", False, mode, steps), mode)


def test_laplacian_model_steps_do_not_depend_on_the_flag():
    _assert_same_runs(_tail_run("lap", True, "eager", 2), _tail_run("lap", False, "eager", 2), "lap")


def test_the_fused_tail_launches_what_it_says(monkeypatch):
    """With the flag on a Dirac step runs the frame GEMM and the one-pass loss and its last block leaves v unwritten; off: none."""
    seen = {"frame": 0, "fwdg": 0, "need_v": []}
    real_frame, real_fwdg, real_block = kernels.linear_fwd_frame, kernels.masked_smooth_l1_fwdg, blocks.dirac_block
    monkeypatch.setattr(kernels, "linear_fwd_frame", lambda *a: (seen.__setitem__("frame", seen["frame"] + 1), real_frame(*a))[1])
    monkeypatch.setattr(kernels, "masked_smooth_l1_fwdg", lambda *a: (seen.__setitem__("fwdg", seen["fwdg"] + 1), real_fwdg(*a))[1])

    def block(mod, Di, DiA, v, f, need_f=True, num_faces=None, avg_next=None, need_v=True):
        seen["need_v"].append(need_v)
        return real_block(mod, Di, DiA, v, f, need_f, num_faces, avg_next, need_v)

    monkeypatch.setattr(blocks, "dirac_block", block)
    _tail_run("dir", True, "eager", 1)
    # (the step, then _tail_run's forward pass under no_grad: the frame GEMM again, the read-only loss)
    assert seen["frame"] == 2 and seen["fwdg"] == 1 and seen["need_v"] == ([True] * 7 + [False]) * 2
    seen.update(frame=0, fwdg=0, need_v=[])
    _tail_run("dir", False, "eager", 1)
    assert seen["frame"] == 0 and seen["fwdg"] == 0 and seen["need_v"] == [True] * 16


def test_the_unwritten_vertex_output_is_loud():
    """v_out_needed=False: what comes back is NaN to everyone but elu_conv1x1, which reads the activated hand-off and gives the
    result of the block that wrote v; without the hand-off it refuses."""
    rng = np.random.default_rng(0)
    V, F = mesh_ops.grid_cloth(7, 6, rng)
    ops = mesh_ops.mesh_operators(V, F)
    Di, DiA = SparseOperator.from_scipy(ops["Di"], DEV), SparseOperator.from_scipy(ops["DiA"], DEV)
    torch.manual_seed(2)
    blk = U.DirResNet2(128).to(DEV).train()
    conv = _conv2()
    v = torch.randn(1, V.shape[0], 128, device=DEV)
    res = {}
    for need in (True, False):
        b_, c_ = copy.deepcopy(blk), copy.deepcopy(conv)
        vi = v.clone().requires_grad_(True)
        vo, _ = b_(Di, DiA, vi, None, f_out_needed=False, num_faces=F.shape[0], avg_next=False, v_out_needed=need)
        if not need:
            assert bool(torch.isnan(vo + 0).all()) and bool(torch.isnan(vo.detach().sum()))
        y = U.elu_conv1x1(c_, vo)
        y.square().mean().backward()
        res[need] = [y.detach().clone(), vi.grad.clone()] + [p.grad.clone() for p in list(b_.parameters()) + list(c_.parameters())]
        if not need:
            with pytest.raises(RuntimeError, match="placeholder"):
                U.elu_conv1x1(c_, vo)                                            # the hand-off went to the first call
    assert all(torch.equal(a, b) for a, b in zip(res[True], res[False]))
    assert bool(torch.isfinite(res[True][0]).all())
