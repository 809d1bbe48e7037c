"""The host statement of the lattice Delaunay triangulation (mesh_ops.delaunay_2d; include/sn_spmm.h, "Lattice Delaunay and the
Mesh-MNIST maker") against an independent checker and scipy.spatial.Delaunay.  No GPU."""
import os
import re

import numpy as np
import pytest

import delaunay_cases as cases
from surfacenetworks_amd import mesh_ops as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERAL = cases.general_position_cases(mo.DELAUNAY_MAX_POINTS)


@pytest.fixture(scope="module")
def statements():
    groups = (GENERAL, cases.collinear_prefix_cases(), cases.degenerate_valid_cases())
    return {name: mo.delaunay_2d(P) for g in groups for name, P in g.items()}


@pytest.mark.parametrize("name", list(GENERAL) + list(cases.collinear_prefix_cases()) + list(cases.degenerate_valid_cases()))
def test_statement_passes_the_checker(statements, name):
    P = {**GENERAL, **cases.collinear_prefix_cases(), **cases.degenerate_valid_cases()}[name]
    d = statements[name]
    assert d.status == 0 and d.nF == d.F.shape[0] and d.F.dtype == np.int32
    cocircular, boundary = cases.check_triangulation(P, d.F)
    assert (cocircular, boundary) == (d.cocircular, d.boundary)
    assert np.array_equal(mo.canonical_faces(d.F), d.F), "faces are not in canonical form"
    if name in cases.degenerate_valid_cases():
        assert d.cocircular > 0
    if name in cases.collinear_prefix_cases():
        assert d.cocircular == 0 and cases.has_collinear_hull_triple(P)


@pytest.mark.parametrize("name", list(GENERAL))
def test_statement_equals_scipy_in_general_position(statements, name):
    from scipy.spatial import Delaunay

    P, d = GENERAL[name], statements[name]
    assert d.cocircular == 0 and not cases.has_collinear_hull_triple(P), "the case is not in general position"
    S = Delaunay(P.astype(np.float64)).simplices.astype(np.int64)
    cw = np.array([cases.orient(P[a], P[b], P[c]) < 0 for a, b, c in S])
    S[cw] = S[cw][:, [0, 2, 1]]
    assert np.array_equal(mo.canonical_faces(S), d.F)


def test_the_diagonal_follows_the_sign_of_one_lattice_unit():
    P_in, P_out = cases.near_cocircular_quads()
    d_in, d_out = mo.delaunay_2d(P_in), mo.delaunay_2d(P_out)
    assert d_in.cocircular == d_out.cocircular == 0
    assert d_in.F.tolist() == [[0, 1, 2], [0, 2, 3]] and d_out.F.tolist() == [[0, 1, 3], [1, 2, 3]]
    for P in cases.near_cocircular_dozen():
        d = mo.delaunay_2d(P)
        assert cases.check_triangulation(P, d.F) == (d.cocircular, d.boundary)


def test_incircle_needs_more_than_64_bits():
    M = cases.M24
    a, b, c, d = (-M, -M), (M, -M), (0, M), (M, M)
    val = mo.lattice_incircle(a, b, c, d)
    assert val == cases.incircle(a, b, c, d) and abs(val).bit_length() == 98
    wrapped = (val + 2 ** 63) % 2 ** 64 - 2 ** 63                 # what an int64 accumulator would hold
    assert wrapped != val


def test_refusals():
    sets, want = cases.ragged_refusal_batch(mo.DELAUNAY_MAX_POINTS)
    for s, w in zip(sets, want):
        d = mo.delaunay_2d(s)
        assert d.status == w and (d.nF == 0) == (w != 0)
    P, count = cases.pad_batch(sets)
    b = mo.delaunay_2d(P, count)
    assert b.status.tolist() == want and b.F.shape == (len(sets), 2 * P.shape[1], 3)
    for i, s in enumerate(sets):
        one = mo.delaunay_2d(s)
        assert b.nF[i] == one.nF and np.array_equal(b.F[i, : one.nF], one.F) and (b.F[i, one.nF:] == -1).all()
    assert mo.delaunay_2d(cases.random_set(30, 3), max_flips=2).status == mo.DT_NOT_CONVERGED


def test_quantum_snaps_to_the_lattice():
    rng = np.random.default_rng(4)
    P = rng.random((40, 2)) * 27.0
    L = mo.snap_to_lattice(P, 2.0 ** -16)
    assert np.array_equal(L, np.rint(P * 65536.0).astype(np.int64))
    assert np.array_equal(mo.delaunay_2d(P, quantum=2.0 ** -16).F, mo.delaunay_2d(L).F)


def test_header_and_bindings_state_the_same_constants():
    from surfacenetworks_amd import _lib, kernels

    header = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    const = lambda name: int(re.search(rf"#define {name}\s+(\d+)", header).group(1))
    assert const("SN_DELAUNAY_MAX_POINTS") == mo.DELAUNAY_MAX_POINTS == _lib.load().sn_delaunay2d_max_points() >= 512
    assert const("SN_MESHDIGITS_MAX_ATTEMPTS") == mo.MESHDIGITS_MAX_ATTEMPTS == kernels.MESHDIGITS_MAX_ATTEMPTS == 8
    assert const("SN_MESHDIGITS_MIN_DET") == mo.MESHDIGITS_MIN_DET == kernels.MESHDIGITS_MIN_DET == int(0.02 * 2 ** 32)
    for name in ("DEGENERATE", "DUPLICATE", "RANGE", "TOO_LARGE", "NOT_CONVERGED", "REJECTED", "INTERNAL"):
        assert const(f"SN_DT_{name}") == getattr(mo, f"DT_{name}") == getattr(kernels, f"DT_{name}")
    for name in ("sn_delaunay2d_i32", "sn_poisson_disc_i32", "sn_mesh_digits_u8", "sn_poisson_disc_cells"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().sn_poisson_disc_cells(27, 27, 98304) == 676 == np.prod(mo.poisson_grid(1.5, 27, 27)[2:])
    assert _lib.load().sn_poisson_disc_cells(40, 40, 98304) < 0        # more cells than SN_DELAUNAY_MAX_POINTS: refused
