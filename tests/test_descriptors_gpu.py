"""Mesh descriptors on the device against their host statement (mesh_ops.vertex_descriptors / libigl_laplacian).
Everything built from + - * / sqrt alone is compared bit for bit: those are correctly rounded on both sides and the definition
(include/sn_spmm.h, "Mesh descriptors") fixes their order.  The two outputs that go through atan2 (gauss, n_angle) get an
allowance per angle: the device library's atan2 and numpy's are fed bit-identical arguments and may differ in their last places.
ATAN2_SLACK = 2^-48 = 8 ulp of pi per angle (LABNOTES.md#descriptors has the figure's origin and the largest difference seen)."""
import functools

import numpy as np
import pytest
import torch

import descriptor_cases as cases
from surfacenetworks_amd import _lib, datasets, functional, kernels, mesh_ops, operators

pytestmark = pytest.mark.gpu

ATAN2_SLACK = 2.0 ** -48
U23 = 2.0 ** -23


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # (a copy: the cases are read-only)


def _np(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device(name):
    """All outputs of one case, computed once: {field: numpy array} and the status as an int."""
    c = cases.case(name)
    d = operators.vertex_descriptors(_dev(c.V), _dev(c.F))
    out = {f: _np(getattr(d, f)) for f in cases.FIELDS}
    out["status"] = int(d.status.item())
    return out


@pytest.mark.parametrize("name", cases.NAMES)
def test_exact_outputs_equal_the_host_statement_bit_for_bit(name):
    want, got = cases.host(name), device(name)
    for field in cases.EXACT_FIELDS:
        g, w = got[field], getattr(want, field)
        assert g.dtype == np.float32 and g.shape == w.shape, field
        assert g.tobytes() == w.tobytes(), (field, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
    assert got["status"] == want.status


@pytest.mark.parametrize("name", cases.NAMES)
def test_angle_outputs_stay_inside_the_atan2_allowance(name):
    want, got, deg = cases.host(name), device(name), cases.host_sums(name)["degree"]
    gd = np.abs(got["gauss"].astype(np.float64) - want.gauss.astype(np.float64))
    nd = np.abs(got["n_angle"].astype(np.float64) - want.n_angle.astype(np.float64))
    print(f"{name}: gauss differs in {int((gd > 0).sum())} of {gd.size} entries, largest {gd.max():.3e}; "
          f"n_angle in {int((nd > 0).sum())} of {nd.size}, largest {nd.max():.3e}")
    assert (gd <= deg * ATAN2_SLACK + U23 * np.abs(want.gauss.astype(np.float64))).all()
    assert (nd <= U23).all()


@pytest.mark.parametrize("hack", cases.HACKS)
@pytest.mark.parametrize("mass", cases.MASSES)
@pytest.mark.parametrize("name", [n for n in cases.NAMES if n != "fan40"])
def test_libigl_laplacian_equals_the_host_statement_bit_for_bit(name, mass, hack):
    c = cases.case(name)
    want, want_status = cases.host_laplacian(name, mass, hack)
    rowptr, colind, vals, status = kernels.cot_laplacian_from_mesh(_dev(c.V), _dev(c.F), mass, hack)
    assert np.array_equal(_np(rowptr), want.indptr) and np.array_equal(_np(colind), want.indices)
    assert _np(vals).tobytes() == want.data.tobytes()
    assert status == want_status


@pytest.mark.parametrize("name", ["disc", "grid_permuted"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    first = device(name)
    again = operators.vertex_descriptors(_dev(c.V), _dev(c.F))
    for field in cases.FIELDS:                                   # the angle-dependent outputs included
        assert _np(getattr(again, field)).tobytes() == first[field].tobytes(), field
    a = kernels.cot_laplacian_from_mesh(_dev(c.V), _dev(c.F), "voronoi", None)
    b = kernels.cot_laplacian_from_mesh(_dev(c.V), _dev(c.F), "voronoi", None)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_fan_has_descriptors_and_no_libigl_laplacian():
    c, got, want = cases.case("fan40"), device("fan40"), cases.host("fan40")
    assert cases.host_sums("fan40")["degree"][0] == 40 > mesh_ops.LAP_MAX_DEGREE
    assert got["status"] == 0 and got["mass_voronoi"][0] == want.mass_voronoi[0] > 0 and got["n_area"][0, 2] > 0.9
    with pytest.raises(_lib.SnError, match="SN_DESC_DEGREE"):
        kernels.cot_laplacian_from_mesh(_dev(c.V), _dev(c.F))
    with pytest.raises(_lib.SnError, match="SN_DESC_DEGREE"):
        operators.laplacian_operator_from_mesh(_dev(c.V), _dev(c.F), convention="libigl")


@pytest.mark.parametrize("field", cases.FIELDS)
def test_one_output_alone_equals_it_among_all(field):
    c, both = cases.case("junk"), device("junk")
    d = operators.vertex_descriptors(_dev(c.V), _dev(c.F), want=[field])
    assert _np(getattr(d, field)).tobytes() == both[field].tobytes()
    assert all(getattr(d, other) is None for other in cases.FIELDS if other != field)
    assert d.status.dtype == torch.int32 and d.status.numel() == 1


def test_named_conveniences_are_the_descriptor_fields():
    c, got = cases.case("disc"), device("disc")
    V, F = _dev(c.V), _dev(c.F)
    for weighting in ("area", "uniform", "angle"):
        assert _np(operators.vertex_normals(V, F, weighting)).tobytes() == got["n_" + weighting].tobytes()
    assert _np(operators.face_areas(V, F)).tobytes() == got["face_area"].tobytes()
    assert _np(operators.vertex_mass(V, F)).tobytes() == got["mass_voronoi"].tobytes()
    assert _np(operators.vertex_mass(V, F, kind="barycentric")).tobytes() == got["mass_bary"].tobytes()
    assert _np(operators.gaussian_curvature(V, F)).tobytes() == got["gauss"].tobytes()
    assert _np(operators.gaussian_curvature(V, F, area_avg=True)).tobytes() == (got["gauss"] / got["mass_voronoi"]).tobytes()
    with pytest.raises(ValueError):
        operators.vertex_normals(V, F, "cotangent")
    with pytest.raises(ValueError):
        operators.vertex_descriptors(V, F, want=["normals"])


def test_batch_equals_three_single_calls():
    c = cases.case("batch")
    V, F = _dev(c.V), _dev(c.F)
    whole = operators.vertex_descriptors(V, F)
    per_mesh = operators.vertex_descriptors(V, F.unsqueeze(0).expand(3, -1, -1).contiguous())      # per-mesh faces: the same
    singles = [operators.vertex_descriptors(V[b], F) for b in range(3)]
    for field in cases.FIELDS:
        w = getattr(whole, field)
        assert w.shape[0] == 3 and torch.equal(w, getattr(per_mesh, field)), field
        for b in range(3):
            assert _np(w[b]).tobytes() == _np(getattr(singles[b], field)).tobytes(), (field, b)
    assert _np(singles[0].n_area).tobytes() == device("grid")["n_area"].tobytes()                   # batch[0] is the grid
    L = operators.laplacian_operator_from_mesh(V, F, convention="libigl", mass="voronoi")
    nV, at = c.V.shape[1], 0
    for b in range(3):
        one = operators.laplacian_operator_from_mesh(V[b], F, convention="libigl", mass="voronoi")
        n = one.vals.numel()
        assert torch.equal(L.vals[at:at + n], one.vals) and torch.equal(L.colind[at:at + n], one.colind + b * nV)
        at += n
    assert L.batch == 3 and at == L.vals.numel()


def test_batch_keeps_a_bad_index_out_of_the_neighbouring_mesh():
    """junk has a face with the index nV + 1: offset into a batch it would name a vertex of the next mesh."""
    c = cases.case("junk")
    V, F = _dev(np.stack([c.V, 1.5 * c.V])), _dev(c.F)
    whole = operators.vertex_descriptors(V, F)
    for b in range(2):
        one = operators.vertex_descriptors(V[b], F)
        for field in cases.FIELDS:
            assert _np(getattr(whole, field)[b]).tobytes() == _np(getattr(one, field)).tobytes(), (field, b)
        assert int(whole.status.item()) == int(one.status.item()) == cases.host("junk").status
    assert _np(whole.n_area[0]).tobytes() == device("junk")["n_area"].tobytes()


def test_reference_convention_is_untouched_and_the_combinations_are_refused():
    c = cases.case("disc")
    V, F = _dev(c.V), _dev(c.F)
    a = operators.laplacian_operator_from_mesh(V, F)
    b = operators.laplacian_operator_from_mesh(V, F, convention="reference")
    rp, ci, v = kernels.laplacian_from_mesh(V, F)
    assert torch.equal(a.vals, v) and torch.equal(b.vals, v) and torch.equal(a.colind, ci) and torch.equal(a.rowptr, rp)
    with pytest.raises(ValueError):
        operators.laplacian_operator_from_mesh(V, F, intrinsic=True, convention="libigl")
    with pytest.raises(ValueError):
        operators.laplacian_operator_from_mesh(V, F, convention="igl")
    with pytest.raises(ValueError):
        operators.laplacian_operator_from_mesh(V, F, hack=1)


def test_normal_frame_on_the_sphere():
    c = cases.case("sphere")
    frame = datasets.normal_frame_from_mesh(c.V, c.F, model="lap", name="sphere")
    assert set(frame) == {"V", "F", "input", "target_dist", "name", "L"} and frame["name"] == "sphere"
    P = c.V.astype(np.float64)
    P = P - P.min(axis=0)
    P = (P / P.max()).astype(np.float32)                                             # sampler.py:48-50
    assert _np(frame["V"]).tobytes() == P.tobytes() and frame["input"] is frame["V"]
    assert np.array_equal(_np(frame["F"]), c.F) and frame["F"].dtype == torch.int64
    assert frame["target_dist"].shape == (258, 3)
    assert torch.equal(frame["target_dist"], operators.vertex_normals(frame["V"], frame["F"], "area"))
    L = frame["L"]
    want, want_status = mesh_ops.libigl_laplacian(P, c.F, "barycentric", 1)
    assert L.status == want_status == 0 and _np(L.vals).tobytes() == want.data.tobytes()
    # L @ V is the cotangent Laplacian of the positions over the mass: dP / M_bary of the host statement
    s = mesh_ops.descriptor_sums(P, c.F)
    got = _np(functional.spmm(L, frame["V"].contiguous())).astype(np.float64)
    assert got.shape == (258, 3)
    term = np.abs(want.data).astype(np.float64) * np.abs(P).max(axis=1).astype(np.float64)[want.indices]       # |l_vj| |p_j|
    largest = np.maximum.reduceat(term, want.indptr[:-1])                            # (every row has its diagonal: none is empty)
    deg = np.diff(want.indptr) - 1
    err = np.abs(got - s["dP"] / s["M_bary"][:, None]).max(axis=1)
    print(f"L @ V against dP / M_bary: largest error {(err / (deg * 2.0 ** -22 * largest)).max():.3f} of the allowance")
    assert (err <= deg * 2.0 ** -22 * largest).all()


def test_normal_frame_gives_up_like_read_npz():
    c = cases.case("junk")
    with pytest.warns(UserWarning, match="non-finite Laplacian"):
        assert datasets.normal_frame_from_mesh(c.V, c.F, model="lap", hack=None, name="junk") is None
    frame = datasets.normal_frame_from_mesh(c.V, c.F, model="lap", hack=1, name="junk")             # the clamp saves the frame
    assert frame is not None and frame["L"].status & kernels.DESC_CLAMPED and bool(torch.isfinite(frame["L"].vals).all())
    with pytest.raises(ValueError, match="bad faces"):
        datasets.normal_frame_from_mesh(c.V, c.F, model="dir")


def test_normal_frame_dirac_operators_are_the_existing_builder_s():
    c = cases.case("sphere")
    frame = datasets.normal_frame_from_mesh(c.V, c.F, model="dir", uniform_mesh=False, target="angle")
    assert set(frame) == {"V", "F", "input", "target_dist", "name", "Di", "DiA"}
    Di, DiA = operators.dirac_operators_from_mesh(_dev(c.V), _dev(c.F))
    for got, want in ((frame["Di"], Di), (frame["DiA"], DiA)):
        assert got.shape == want.shape
        assert all(torch.equal(x, y) for x, y in zip(got._bsr4, want._bsr4))
    assert _np(frame["target_dist"]).tobytes() == device("sphere")["n_angle"].tobytes()
