"""Mesh repair on the device against its host statement (mesh_ops.repair_mesh and its steps), bit for bit: kernels.mesh_weld,
mesh_unique_faces, mesh_orient, operators.repair_mesh and the frame builders with repair=True.  Every comparison is an exact
integer or bitwise one; no tolerance anywhere."""
import numpy as np
import pytest
import torch

import repair_cases as cases
from surfacenetworks_amd import datasets, kernels, mesh_ops, operators

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # (a copy: the cases are read-only)


def _np(t):
    return t.cpu().numpy()


def assert_same_repair(got, want, what):
    """A RepairedMesh of the device against a Repaired / Expect of numpy arrays, field by field."""
    for k in cases.ARRAYS:
        g = getattr(got, k)
        assert torch.is_tensor(g) and g.is_cuda, f"{what}: {k} is no device tensor"
        assert cases.same_bits(_np(g), np.asarray(getattr(want, k))), f"{what}: {k} differs"
    for k in cases.COUNTS:
        assert type(getattr(got, k)) is int and getattr(got, k) == getattr(want, k), \
            f"{what}: {k} = {getattr(got, k)}, expected {getattr(want, k)}"


@pytest.mark.parametrize("name", cases.NAMES)
def test_repair_equals_the_host_statement(name):
    c = cases.case(name)
    got = operators.repair_mesh(_dev(c.V), _dev(c.F), c.tol)
    assert_same_repair(got, cases.host_repair(name), name)
    assert_same_repair(got, c.want, f"{name} (construction)")
    assert got.V.dtype == torch.float32 and got.F.dtype == torch.int32 and got.flipped.dtype == torch.int32


@pytest.mark.parametrize("name", ["moebius5", "book3", "nan_vertex", "dup_faces", "tol_grid", "strip_alternating"])
def test_steps_equal_their_host_statements(name):
    c = cases.case(name)
    nV = len(c.V)
    V, F = _dev(c.V), _dev(c.F)
    w, ww = kernels.mesh_weld(V, F, c.tol), mesh_ops.weld_vertices(c.V, c.F, c.tol)
    assert np.array_equal(_np(w.rep), ww.rep) and np.array_equal(_np(w.F), ww.F)
    assert _np(w.counts).tolist() == ww.counts.tolist() and _np(w.status).tolist() == [ww.status]
    u, wu = kernels.mesh_unique_faces(w.F, nV, V), mesh_ops.unique_faces(ww.F, nV, c.V)
    assert np.array_equal(_np(u.keep), wu.keep) and _np(u.counts).tolist() == wu.counts.tolist()
    assert _np(u.status).tolist() == [wu.status]
    o, wo = kernels.mesh_orient(w.F, u.keep, nV), mesh_ops.orient_faces(ww.F, wu.keep, nV)
    for k in ("flip", "label", "F", "counts"):
        assert getattr(o, k).dtype == torch.int32 and np.array_equal(_np(getattr(o, k)), getattr(wo, k)), k
    assert _np(o.status).tolist() == [wo.status]
    nov = kernels.mesh_unique_faces(w.F, nV)                              # without coordinates: no degenerate count
    assert torch.equal(nov.keep, u.keep) and _np(nov.counts).tolist() == wu.counts.tolist()[:2] + [0]


@pytest.mark.parametrize("name", ["strip_alternating", "torus_soup_shuffled", "coincident"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    V, F = _dev(c.V), _dev(c.F)
    a, b = operators.repair_mesh(V, F, c.tol), operators.repair_mesh(V, F, c.tol)
    for k in cases.ARRAYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a[6:] == b[6:]
    w1, w2 = kernels.mesh_weld(V, F, c.tol), kernels.mesh_weld(V, F, c.tol)
    u = kernels.mesh_unique_faces(w1.F, len(c.V), V)
    o1, o2 = kernels.mesh_orient(w1.F, u.keep, len(c.V)), kernels.mesh_orient(w1.F, u.keep, len(c.V))
    assert all(torch.equal(x, y) for x, y in zip(w1, w2)) and all(torch.equal(x, y) for x, y in zip(o1, o2))


@pytest.mark.parametrize("name,switch", [("torus_soup_shuffled", "weld"), ("dup_faces", "unique"), ("torus_soup_shuffled", "orient"),
                                         ("nan_vertex", "weld"), ("moebius5", "orient")])
def test_one_step_switched_off(name, switch):
    c = cases.case(name)
    flags = {"weld": True, "unique": True, "orient": True, switch: False}
    got = operators.repair_mesh(_dev(c.V), _dev(c.F), c.tol, **flags)
    assert_same_repair(got, cases.host_repair(name, **flags), f"{name} without {switch}")


def test_int64_faces_and_numpy_inputs():
    c = cases.case("two_triangle_soup")
    want = cases.host_repair("two_triangle_soup")
    assert_same_repair(operators.repair_mesh(_dev(c.V), _dev(c.F.astype(np.int64))), want, "int64 F")
    assert_same_repair(operators.repair_mesh(c.V, c.F), want, "numpy")
    assert_same_repair(operators.repair_mesh(c.V.astype(np.float64), c.F.astype(np.int64)), want, "numpy float64 / int64")


def test_error_paths():
    c = cases.case("tetra_one_turned")
    V, F = _dev(c.V), _dev(c.F)
    with pytest.raises(ValueError, match="tol"):
        operators.repair_mesh(V, F, tol=-1e-3)
    with pytest.raises(ValueError, match="tol"):
        operators.repair_mesh(V, F, tol=float("nan"))
    with pytest.raises(ValueError, match=r"\(nV, 3\)"):
        operators.repair_mesh(V[:, :2], F)
    with pytest.raises(ValueError, match=r"\(nF, 3\)"):
        operators.repair_mesh(V, F.reshape(-1))
    with pytest.raises(TypeError):
        operators.repair_mesh(V, F.float())
    with pytest.raises(TypeError):
        operators.repair_mesh(V.int(), F)
    with pytest.raises(Exception):
        operators.repair_mesh(V.cpu(), F.cpu())
    with pytest.raises(TypeError):
        kernels.mesh_weld(V, F.long())
    with pytest.raises(TypeError):
        kernels.mesh_orient(F, torch.ones(len(c.F), dtype=torch.int64, device="cuda"), 4)
    with pytest.raises(ValueError):
        kernels.mesh_orient(F, torch.ones(len(c.F) + 1, dtype=torch.int32, device="cuda"), 4)
    with pytest.raises(ValueError):
        kernels.mesh_unique_faces(F, 5, V)


def test_empty_mesh():
    got = operators.repair_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert got.V.shape == (0, 3) and got.F.shape == (0, 3) and got[6:] == (0,) * 7
    got = operators.repair_mesh(np.ones((3, 3), np.float32), np.zeros((0, 3), np.int32))
    assert got.V.shape == (0, 3) and got.welded_vertices == 2 and _np(got.vertex_index).tolist() == [-1, -1, -1]


def _wound_as_stored(c):
    """The welded mesh of a case by its books, its faces wound as they were stored: want.F with the flipped rows turned back."""
    F = np.array(c.want.F)
    t = c.want.flipped == 1
    F[t] = F[t][:, [0, 2, 1]]
    return F


def test_intrinsic_laplacian_refuses_the_scan_and_takes_the_repaired_mesh():
    c = cases.case("torus_soup_shuffled")
    # today: welded by the books but wound as it was stored, the scan is refused, and the refusal names the orientation
    with pytest.raises(ValueError, match="not consistently oriented"):
        operators.laplacian_operator_from_mesh(_dev(c.want.V), _dev(_wound_as_stored(c)), intrinsic=True)
    rm = operators.repair_mesh(_dev(c.V), _dev(c.F))
    got = operators.laplacian_operator_from_mesh(rm.V, rm.F, intrinsic=True)
    want = operators.laplacian_operator_from_mesh(_dev(c.want.V), _dev(c.want.F), intrinsic=True)
    assert torch.equal(got.rowptr, want.rowptr) and torch.equal(got.colind, want.colind) and torch.equal(got.vals, want.vals)
    assert got.rowptr.shape[0] == len(c.V0) + 1


def test_faust_frame_of_the_soup_has_the_geodesics_of_the_torus():
    c = cases.case("torus_soup_shuffled")
    frame = datasets.faust_frame_from_mesh(c.V, c.F, repair=True, component="largest")
    assert_same_repair(frame["repair"], c.want, "frame['repair']")
    vm = frame["vertex_map"]
    assert vm.dtype == torch.int64 and np.array_equal(_np(vm), c.want.vertex_map)
    orig = _dev(c.vert_orig)[vm]                                          # the torus vertex behind every vertex of the frame
    assert np.array_equal(np.sort(_np(orig)), np.arange(len(c.V0)))
    G0 = operators.geodesic_matrix_from_mesh(_dev(c.V0), _dev(c.F0))
    assert torch.equal(frame["G"], G0[orig][:, orig])
    with pytest.raises(ValueError, match="label"):
        datasets.faust_frame_from_mesh(c.V, c.F, label=np.arange(len(c.V)), repair=True)


def test_normal_frame_repair_gives_the_targets_of_the_clean_mesh():
    c = cases.case("torus_soup_shuffled")
    got = datasets.normal_frame_from_mesh(c.V, c.F, repair=True)
    want = datasets.normal_frame_from_mesh(c.want.V, c.want.F)
    assert_same_repair(got["repair"], c.want, "frame['repair']")
    assert torch.equal(got["V"], want["V"]) and torch.equal(got["F"], want["F"])
    assert torch.equal(got["target_dist"], want["target_dist"]) and torch.equal(got["L"].vals, want["L"].vals)
    assert "repair" not in want
