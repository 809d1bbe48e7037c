"""ARAP deformation on the device against its host statement (mesh_ops.arap_*), bit for bit: kernels.arap_weights, arap_frames,
operators.arap_deform and arap.ClothSequences(dynamics="arap").  Every comparison is bitwise; no tolerance anywhere."""
import warnings

import numpy as np
import pytest
import torch

import arap_cases as cases
from surfacenetworks_amd import arap, kernels, mesh_ops, operators

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # (a copy: the cases are read-only)


def _run(c, weights=None, frames_per_launch=None, first_step=True):
    V = _dev(c.V)
    weights = weights if weights is not None else kernels.arap_weights(V, _dev(c.F))
    nmax = int(np.diff(c.voff).max())
    return kernels.arap_frames(V, weights, _dev(c.voff), _dev(c.hoff), _dev(c.handles), _dev(c.H), nmax, c.iters, c.tol, c.max_cg,
                               frames_per_launch=frames_per_launch, first_step=first_step)


def _bytes(out):
    return tuple(None if t is None else t.cpu().numpy().tobytes() for t in out)


@pytest.mark.parametrize("name", cases.NAMES)
def test_weights_equal_the_statement(name):
    c = cases.case(name)
    want = cases.host_weights(name)
    got = kernels.arap_weights(_dev(c.V), _dev(c.F))
    nnz = int(want.rowptr[-1])
    assert np.array_equal(got.rowptr.cpu().numpy(), want.rowptr) and np.array_equal(got.colind.cpu().numpy()[:nnz], want.colind)
    assert got.w.cpu().numpy()[:nnz].tobytes() == want.w.tobytes() and got.d.cpu().numpy().tobytes() == want.d.tobytes()
    assert got.status.tolist() == [want.status]


@pytest.mark.parametrize("name", cases.NAMES)
def test_frames_equal_the_statement(name):
    c = cases.case(name)
    got = _run(c)
    frames, R_first, rhs_first = got.frames.cpu().numpy(), got.R_first.cpu().numpy(), got.rhs_first.cpu().numpy()
    for b, want in enumerate(cases.host_result(name)):
        v0, v1 = c.voff[b], c.voff[b + 1]
        assert R_first[v0:v1].tobytes() == want.R_first.tobytes(), "rotations of the first local step"
        assert rhs_first[v0:v1].tobytes() == want.rhs_first.tobytes(), "right-hand side of the first global step"
        assert np.array_equal(got.cg_iters[b].cpu().numpy(), want.cg_iters)
        assert got.energy[b].cpu().numpy().tobytes() == want.energy.tobytes()
        assert frames[:, v0:v1].tobytes() == want.frames.tobytes()
        assert int(got.status[b]) == want.status
    if name == "capped":
        assert int(got.status[0]) == mesh_ops.ARAP_NOT_CONVERGED


@pytest.mark.parametrize("name", ["cloth9x7", "ragged_pair", "cloth34x33"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    assert _bytes(_run(c)) == _bytes(_run(c))


def test_each_mesh_of_a_batch_equals_its_single_run():
    pair = cases.case("ragged_pair")
    got = _run(pair, first_step=False)
    for b, name in enumerate(("cloth5x5", "cloth9x7")):
        one = _run(cases.case(name), first_step=False)
        assert torch.equal(got.frames[:, pair.voff[b]:pair.voff[b + 1]], one.frames)
        assert torch.equal(got.cg_iters[b], one.cg_iters[0]) and torch.equal(got.energy[b], one.energy[0])
        assert torch.equal(got.status[b], one.status[0])


@pytest.mark.parametrize("name", ["cloth9x7", "ragged_pair"])
def test_chunks_of_one_frame_equal_one_call(name):
    c = cases.case(name)
    assert _bytes(_run(c, frames_per_launch=1)) == _bytes(_run(c, frames_per_launch=c.H.shape[0]))


def test_a_mesh_larger_than_the_launch_allows_is_left_at_rest():
    c = cases.case("ragged_pair")
    V = _dev(c.V)
    w = kernels.arap_weights(V, _dev(c.F))
    got = kernels.arap_frames(V, w, _dev(c.voff), _dev(c.hoff), _dev(c.handles), _dev(c.H), 25, c.iters, c.tol, c.max_cg)
    one = _run(cases.case("cloth5x5"), first_step=False)
    assert torch.equal(got.frames[:, :25], one.frames) and torch.equal(got.cg_iters[0], one.cg_iters[0])
    assert got.status.tolist() == [0, mesh_ops.ARAP_TOO_LARGE] and not got.cg_iters[1].any() and not got.energy[1].any()
    assert torch.equal(got.frames[:, 25:], V[25:].expand(c.H.shape[0], -1, -1))


def test_a_free_vertex_without_weights_breaks_down_like_the_statement():
    c = cases.case("cloth5x5")
    V = np.concatenate([c.V, [[5.0, 5.0, 5.0]]]).astype(np.float32)
    want = mesh_ops.arap_deform(V, c.F, c.handles, c.H)
    assert want.status == mesh_ops.ARAP_BREAKDOWN
    got = _run(c._replace(V=V, voff=np.array([0, 26], np.int32)), first_step=False)
    assert got.frames.cpu().numpy().tobytes() == want.frames.tobytes() and not got.cg_iters.any()
    assert got.energy[0].cpu().numpy().tobytes() == want.energy.tobytes() and got.status.tolist() == [want.status]


def test_every_output_element_is_written(monkeypatch):
    """The outputs come from torch.empty: pre-fill every new allocation of the wrapper with NaN bytes and find none left."""
    c = cases.case("ragged_pair")
    empty = torch.empty

    def poisoned(*size, **kw):
        t = empty(*size, **kw)
        t.view(torch.uint8).fill_(0xFF) if t.numel() else None
        return t

    want = _bytes(_run(c))
    monkeypatch.setattr(torch, "empty", poisoned)
    w = kernels.arap_weights(_dev(c.V), _dev(c.F))
    got = _run(c, weights=w)
    monkeypatch.undo()
    nnz = int(w.rowptr[-1])
    assert not torch.isnan(w.w[:nnz]).any() and not torch.isnan(w.d).any() and (w.colind[:nnz] >= 0).all()
    for t in got:
        assert not torch.isnan(t.double()).any() if t.is_floating_point() else (t >= 0).all()
    assert _bytes(got) == want


def test_operator_single_batch_and_numpy_inputs():
    c = cases.case("cloth5x5")
    want = cases.host_result("cloth5x5")[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        one = operators.arap_deform(c.V, c.F, c.handles, c.H)
        two = operators.arap_deform(_dev(np.stack([c.V, c.V])), _dev(np.stack([c.F, c.F])), _dev(np.stack([c.handles, c.handles])),
                                    _dev(np.stack([c.H, c.H])))
    assert one.frames.cpu().numpy().tobytes() == want.frames.tobytes() and np.array_equal(one.cg_iters.cpu().numpy(), want.cg_iters)
    assert one.energy.cpu().numpy().tobytes() == want.energy.tobytes() and int(one.status) == 0
    assert two.frames.shape == (2,) + want.frames.shape and torch.equal(two.frames[0], one.frames) and torch.equal(two.frames[1], one.frames)
    assert torch.equal(two.cg_iters[1], one.cg_iters) and two.status.tolist() == [0, 0]


def test_operator_refuses_and_warns():
    c = cases.case("cloth5x5")
    h = c.handles.copy()
    h[0] = 25
    with pytest.raises(ValueError, match="outside"):
        operators.arap_deform(c.V, c.F, h, c.H)
    h[0] = c.handles[1]
    with pytest.raises(ValueError, match="repeated"):
        operators.arap_deform(c.V, c.F, h, c.H)
    n = cases.case("no_handle_component")
    with pytest.raises(ValueError, match="no handle"):
        operators.arap_deform(n.V, n.F, n.handles, n.H)
    capped = cases.case("capped")
    with pytest.warns(RuntimeWarning, match="max_cg"):
        out = operators.arap_deform(capped.V, capped.F, capped.handles, capped.H, max_cg=capped.max_cg)
    assert int(out.status) == mesh_ops.ARAP_NOT_CONVERGED


def _cloth_statement(grids, frames, seed, dynamics):
    """What ClothSequences stores, recomputed on the host in the order of its draws: the wave from its formula, or the host's ARAP
    frames (the handle motion is drawn after the wave's three numbers, from the same stream)."""
    rng = np.random.default_rng(seed)
    out = []
    for n, m in grids:
        V0, F = mesh_ops.grid_cloth(n, m, rng)
        V0, F = mesh_ops.MeshOrder.of_mesh(F, V0.shape[0], "auto").mesh(V0, F)
        amp = 0.03 * (0.5 + rng.random())
        k = 2 * np.pi * (1 + rng.integers(0, 3))
        ph = rng.random() * 2 * np.pi
        t = np.arange(frames)[:, None]
        Vt = np.repeat(V0[None], frames, 0)
        Vt[:, :, 2] += amp * np.sin(k * V0[None, :, 0] + 0.25 * t + ph)
        Vt[:, :, 1] += 0.5 * amp * np.cos(k * V0[None, :, 1] + 0.2 * t)
        if dynamics == "arap":
            handles, H = mesh_ops.arap_handle_motion(V0, frames, rng)
            out.append(mesh_ops.arap_deform(V0.astype(np.float32), F, handles, H).frames)
        else:
            out.append(Vt.astype(np.float32))
    return out


def test_cloth_sequences_with_arap_dynamics():
    grids, frames, seed = [(5, 5), (5, 5)], arap.INPUT_FRAMES + arap.OUTPUT_FRAMES + 1, 3
    for dynamics in ("arap", "wave"):
        want = _cloth_statement(grids, frames, seed, dynamics)
        ds = arap.ClothSequences(grids, frames=frames, seed=seed, **({"dynamics": "arap"} if dynamics == "arap" else {}))
        assert ds.dynamics == dynamics and ds.xyz.shape == (2, frames, 25, 3)
        for s in range(2):
            assert ds.xyz[s].cpu().numpy().tobytes() == want[s].tobytes(), dynamics
        if dynamics == "arap":                              # one training step on the deformed sequences
            assert not torch.equal(ds.xyz[:, 0], ds.xyz[:, -1])
            torch.manual_seed(0)
            model = arap.DirModel().to("cuda")
            loss = arap.train_step(model, arap.make_adam(model), ds.sample_batch(2, np.random.default_rng(0)), global_batch=2)
            assert np.isfinite(float(loss.detach()))
