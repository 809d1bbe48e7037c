"""Mesh descriptors, host side (no GPU): what the host statement mesh_ops.vertex_descriptors / libigl_laplacian must satisfy
on meshes whose geometry is known (a sphere, a torus, a tetrahedron, a planar grid), its bookkeeping on junk input and under a
renumbering, and the agreement of header, ctypes table and plan table on the new symbols.  The figures are conditions the
definition meets (include/sn_spmm.h, "Mesh descriptors"), not tolerances of a kernel."""
import os
import re

import numpy as np
import pytest

import descriptor_cases as cases
from surfacenetworks_amd import mesh_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U48, U52, U23 = 2.0 ** -48, 2.0 ** -52, 2.0 ** -23


def test_sphere_normals_and_curvatures():
    c, h = cases.case("sphere"), cases.host("sphere")
    assert c.V.shape == (258, 3) and c.F.shape == (512, 3) and h.status == 0
    assert (np.einsum("fk,fk->f", h.face_normal, c.V[c.F[:, 0]]) > 0).all()              # outward faces
    assert np.abs(h.n_area - c.V).max() <= 0.031
    assert np.abs(h.n_angle - c.V).max() <= 0.012
    ratio = h.gauss.astype(np.float64) / h.mass_voronoi
    assert 1.009 <= ratio.min() and ratio.max() <= 1.018
    assert (h.mean > 0).all() and 0.9999 <= h.mean.min() and h.mean.max() <= 1.0006


@pytest.mark.parametrize("name", ["torus", "sphere"])
def test_gauss_bonnet(name):
    s = cases.host_sums(name)
    K = 2 * np.pi - s["theta"]
    assert abs(K.sum() - 2 * np.pi * cases.EULER[name]) <= 3 * cases.case(name).F.shape[0] * U48


@pytest.mark.parametrize("name", ["grid", "torus", "disc", "sphere", "obtuse"])
def test_both_masses_sum_to_the_surface_area(name):
    s = cases.host_sums(name)
    total, nF = s["area"].sum(), s["area"].shape[0]
    assert s["valid"].all() and total > 0
    assert abs(s["M_bary"].sum() - total) <= nF * U52 * total
    assert abs(s["M_voronoi"].sum() - total) <= nF * U52 * total


def test_tetrahedron_defects_are_pi():
    s = cases.host_sums("tetra")
    assert np.abs((2 * np.pi - s["theta"]) - np.pi).max() <= 4 * U48
    assert np.array_equal(cases.host("tetra").gauss, np.full(4, np.float32(np.pi)))


def test_planar_grid_is_flat_inside_with_an_exact_normal():
    s, h = cases.host_sums("grid_flat"), cases.host("grid_flat")
    inside = s["degree"] == 6
    assert inside.sum() == 16
    assert np.abs(2 * np.pi - s["theta"])[inside].max() <= 6 * U48
    for n in (h.n_area, h.n_uniform, h.n_angle):
        assert np.array_equal(n[:, :2], np.zeros((36, 2), np.float32)) and np.array_equal(np.abs(n[:, 2]), np.ones(36, np.float32))
        assert len(set(n[:, 2].tolist())) == 1                                            # one sign for the whole sheet


def test_junk_sets_its_three_bits_and_leaves_the_grid_alone():
    g, j = cases.host("grid"), cases.host("junk")
    assert g.status == 0
    assert j.status == mesh_ops.DESC_BAD_FACE | mesh_ops.DESC_FLAT_FACE | mesh_ops.DESC_NO_NORMAL
    nV = cases.case("grid").V.shape[0]
    real = np.setdiff1d(np.arange(cases.case("junk").F.shape[0]), cases.JUNK_FACE_ROWS)
    for field in cases.FIELDS:
        got, want = getattr(j, field), getattr(g, field)
        if field in cases.FACE_FIELDS:
            assert got[real].tobytes() == want.tobytes(), field
            assert not got[list(cases.JUNK_FACE_ROWS)].any(), field                       # bad and flat faces: zeros
        else:
            assert got[:nV].tobytes() == want.tobytes(), field                            # no grid vertex is touched by the junk
    # the collinear face's vertices and the isolated vertex: no normal, no mass, the full 2 pi, no mean curvature
    assert not j.n_area[nV:].any() and not j.n_uniform[nV:].any() and not j.n_angle[nV:].any()
    assert not j.mass_bary[nV:].any() and not j.mass_voronoi[nV:].any() and not j.mean[nV:].any()
    assert np.array_equal(j.gauss[nV:], np.full(4, np.float32(2 * np.pi)))


def test_permuted_grid_maps_back():
    perm, fperm = cases.permutation()
    g, p = cases.host("grid"), cases.host("grid_permuted")
    assert p.status == 0
    for field in cases.FACE_FIELDS:                                                       # a face's values do not depend on its place
        assert getattr(p, field).tobytes() == getattr(g, field)[fperm].tobytes(), field
    for field in cases.FIELDS:
        if field in cases.FACE_FIELDS:
            continue
        got, want = getattr(p, field).astype(np.float64), getattr(g, field)[perm].astype(np.float64)
        ulp = np.spacing(np.abs(getattr(g, field)[perm]).astype(np.float32)).astype(np.float64)
        assert (np.abs(got - want) <= ulp).all(), field                                   # the order of the faces at a vertex changed


@pytest.mark.parametrize("mass", cases.MASSES)
@pytest.mark.parametrize("name", ["grid", "torus", "disc", "sphere", "obtuse", "tetra"])
def test_libigl_laplacian_rows_sum_to_zero(name, mass):
    L, status = cases.host_laplacian(name, mass)
    assert status == 0 and L.dtype == np.float32 and L.has_sorted_indices
    deg = np.diff(L.indptr) - 1
    rowsum = np.abs(np.asarray(L.astype(np.float64).sum(axis=1)).ravel())
    largest = np.abs(L).max(axis=1).toarray().ravel().astype(np.float64)
    assert (rowsum <= deg * U23 * largest).all()
    coo = L.tocoo()
    assert np.array_equal(np.sort(coo.row[coo.row == coo.col]), np.arange(L.shape[0]))    # every row stores its diagonal


@pytest.mark.parametrize("name", ["grid", "torus"])
def test_libigl_laplacian_is_the_reference_one_without_its_epsilons(name):
    """-2 M_bary^-1 C = A^-1 (D - W) up to the 1e-6 in 8a + 1e-6 (a >= 0.012 here: a gap of about 1e-5) and the 1e-9 in A."""
    c = cases.case(name)
    L, _ = cases.host_laplacian(name)
    ref = mesh_ops.laplacian(c.V.astype(np.float64), c.F)
    ref.sort_indices()
    assert np.array_equal(L.indptr, ref.indptr) and np.array_equal(L.indices, ref.indices)
    gap = np.abs((-2 * L.astype(np.float64) - ref).toarray()).max(axis=1)
    assert (gap <= 1e-4 * np.abs(ref.toarray()).max(axis=1)).all()


def test_hack_replaces_what_is_not_finite():
    nV = cases.case("grid").V.shape[0]
    L0, st0 = cases.host_laplacian("junk", "barycentric", None)
    L1, st1 = cases.host_laplacian("junk", "barycentric", 1)
    assert st0 == mesh_ops.DESC_BAD_FACE | mesh_ops.DESC_FLAT_FACE and st1 == st0 | mesh_ops.DESC_CLAMPED
    assert np.isnan(L0.diagonal()[nV:]).all() and np.array_equal(L1.diagonal()[nV:], np.ones(4, np.float32))
    assert np.isfinite(L1.data).all()
    assert np.array_equal(L0.indptr, L1.indptr) and np.array_equal(L0.indices, L1.indices)
    keep = np.isfinite(L0.data)
    assert L0.data[keep].tobytes() == L1.data[keep].tobytes()
    # the rows of the grid's own vertices are the grid's rows
    G, _ = cases.host_laplacian("grid")
    assert np.array_equal(L1.indptr[:nV + 1], G.indptr) and L1.data[:G.nnz].tobytes() == G.data.tobytes()


def test_explicit_zeros_are_kept():
    """A right angle in the plane: the cotangent opposite the hypotenuse is exactly zero and stays in the pattern."""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    L, status = mesh_ops.libigl_laplacian(V, np.array([[0, 1, 2]]))
    assert status == 0 and L.nnz == 9 and L[1, 2] == 0 and L[2, 1] == 0
    assert np.array_equal(L.toarray(), np.array([[-6, 3, 3], [3, -3, 0], [3, 0, -3]], np.float32))


def test_fan_descriptors_have_no_degree_limit():
    s, h = cases.host_sums("fan40"), cases.host("fan40")
    assert s["degree"][0] == 40 > mesh_ops.LAP_MAX_DEGREE and h.status == 0
    assert h.n_area[0, 2] > 0.9 and h.mass_bary[0] > 0 and h.mass_voronoi[0] > 0


def test_header_ctypes_and_plan_table_agree_on_the_new_symbols():
    from surfacenetworks_amd import _lib, kernels

    header = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    for name in ("sn_mesh_descriptors_workspace_bytes", "sn_mesh_descriptors_f32", "sn_mesh_cot_laplacian_workspace_bytes",
                 "sn_mesh_cot_laplacian_f32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
        assert (f"SN_PLAN_FN({name})" in table) == (not name.endswith("_bytes"))
    for macro in ("BAD_FACE", "FLAT_FACE", "NO_NORMAL", "CLAMPED", "DEGREE"):
        value = getattr(mesh_ops, "DESC_" + macro)
        assert re.search(rf"#define\s+SN_DESC_{macro}\s+{value}\b", header) and getattr(kernels, "DESC_" + macro) == value
    assert re.search(rf"#define\s+SN_LAP_MAX_DEGREE\s+{mesh_ops.LAP_MAX_DEGREE}\b", header)
    assert len(_lib.SIGNATURES["sn_mesh_descriptors_f32"][1]) == 17
