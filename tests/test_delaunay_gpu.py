"""sn_delaunay2d_i32 on the MI355X against the host statement mesh_ops.delaunay_2d and the independent checker: every comparison
is an exact integer one."""
import numpy as np
import pytest
import torch

import delaunay_cases as cases
from surfacenetworks_amd import kernels, mesh_ops as mo, operators

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAXP = mo.DELAUNAY_MAX_POINTS
UNIQUE = {**cases.general_position_cases(MAXP), **cases.collinear_prefix_cases(),
          **{f"near_quad_{k}": P for k, P in zip(("in", "out"), cases.near_cocircular_quads())}}


@pytest.fixture(scope="module")
def unique_run():
    """Every case with a unique triangulation in ONE ragged batch (statement and device once, shared by the tests)."""
    names = list(UNIQUE)
    P, count = cases.pad_batch([UNIQUE[n] for n in names])
    dev = operators.delaunay_2d(P, count)
    got = {k: getattr(dev, k).cpu().numpy() for k in ("F", "nF", "status", "flips", "cocircular", "rounds", "boundary")}
    return names, got, {n: mo.delaunay_2d(UNIQUE[n]) for n in names}


@pytest.mark.parametrize("name", list(UNIQUE))
def test_device_equals_the_statement(unique_run, name):
    names, got, want = unique_run
    i, w = names.index(name), want[name]
    assert w.status == 0 and w.cocircular == 0
    assert got["status"][i] == 0 and got["nF"][i] == w.nF and got["cocircular"][i] == 0 and got["boundary"][i] == w.boundary
    assert np.array_equal(got["F"][i, : w.nF], w.F) and (got["F"][i, w.nF:] == -1).all()
    assert got["rounds"][i] <= got["flips"][i] <= kernels.DT_MAX_ROUNDS * MAXP


def test_the_diagonal_follows_the_sign_of_one_lattice_unit(unique_run):
    names, got, _ = unique_run
    f_in = got["F"][names.index("near_quad_in"), :2].tolist()
    f_out = got["F"][names.index("near_quad_out"), :2].tolist()
    assert f_in == [[0, 1, 2], [0, 2, 3]] and f_out == [[0, 1, 3], [1, 2, 3]]


def test_exactly_max_points_alone():
    P = UNIQUE["random_max"]
    assert P.shape[0] == MAXP == kernels.delaunay_max_points()
    d = operators.delaunay_2d(P)
    assert d.F.shape == (2 * MAXP, 3) and int(d.status) == 0
    assert np.array_equal(d.faces().cpu().numpy(), mo.delaunay_2d(P).F)


DEGENERATE = {**cases.degenerate_valid_cases(), **{f"dozen_{k}": P for k, P in zip(("in", "out"), cases.near_cocircular_dozen())}}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_but_valid_inputs(name):
    P = DEGENERATE[name]
    a, b = operators.delaunay_2d(P), operators.delaunay_2d(P)
    assert int(a.status) == 0
    F = a.faces().cpu().numpy()
    cocircular, boundary = cases.check_triangulation(P, F)
    assert (cocircular, boundary) == (int(a.cocircular), int(a.boundary))
    assert np.array_equal(mo.canonical_faces(F), F)
    if name in cases.degenerate_valid_cases():
        assert cocircular > 0
    if cocircular == 0:
        assert np.array_equal(F, mo.delaunay_2d(P).F)
    for k in ("F", "nF", "status", "flips", "cocircular", "rounds", "boundary"):
        assert torch.equal(getattr(a, k), getattr(b, k)), f"two runs differ in {k}"


def test_ragged_batch_with_refusals():
    sets, want = cases.ragged_refusal_batch(MAXP)
    P, count = cases.pad_batch(sets)
    d = operators.delaunay_2d(torch.from_numpy(P).to(DEV), torch.from_numpy(count).to(DEV))
    st, nF, F = d.status.cpu().numpy(), d.nF.cpu().numpy(), d.F.cpu().numpy()
    assert st.tolist() == want
    for i, (s, w) in enumerate(zip(sets, want)):
        if w:
            assert nF[i] == 0 and (F[i] == -1).all()
        else:
            one = mo.delaunay_2d(s)
            assert nF[i] == one.nF and np.array_equal(F[i, : one.nF], one.F) and (F[i, one.nF:] == -1).all()
    host = mo.delaunay_2d(P, count)
    assert np.array_equal(host.status, st) and np.array_equal(host.nF, nF) and np.array_equal(host.F, F)


def test_flip_budget_and_interface():
    P = cases.random_set(50, 12)
    d = operators.delaunay_2d(P, max_rounds=1)
    assert int(d.status) == mo.DT_NOT_CONVERGED and int(d.nF) == 0
    Pf = np.random.default_rng(4).random((40, 2)) * 27.0
    got = operators.delaunay_2d(Pf, quantum=2.0 ** -16)
    assert np.array_equal(got.faces().cpu().numpy(), mo.delaunay_2d(Pf, quantum=2.0 ** -16).F)
    with pytest.raises(TypeError, match="quantum"):
        operators.delaunay_2d(Pf)
    with pytest.raises(ValueError, match="wants P"):
        operators.delaunay_2d(np.zeros((3, 3), np.int32))
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.delaunay_2d(torch.zeros(1, 3, 2, dtype=torch.int32))
    far = operators.delaunay_2d(np.array([[0, 0], [1 << 40, 5], [7, 9]], np.int64))         # clipped to the limit: out of range
    assert int(far.status) == mo.DT_RANGE
