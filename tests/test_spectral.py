"""The host statement of the spectral path (mesh_ops.cot_pencil, spectral_start, cheb_filter_step, laplacian_eigenpairs,
wave_kernel_signature; include/sn_spmm.h, "Spectral") against the dense oracle of tests/spectral_cases.py.  No GPU.  The bounds
are derived where they can be (eigenvalues and residuals from tol b, the recomputed residual from the rounding of one product)
and measured where they cannot (M-orthonormality, the WKS error: spectral_cases has the figures and where they come from)."""
import ctypes
import os
import re

import numpy as np
import pytest

import spectral_cases as cases
from surfacenetworks_amd import mesh_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.mark.parametrize("name", cases.NAMES)
def test_pencil_is_symmetric_bit_for_bit_and_is_the_laplacians_numerator(name):
    c = cases.case(name)
    S, mass, status = cases.pencil(name)
    St = S.T.tocsr()
    St.sort_indices()
    assert np.array_equal(S.indptr, St.indptr) and np.array_equal(S.indices, St.indices) and S.data.tobytes() == St.data.tobytes()
    assert (np.diff(S.indices) > 0)[np.setdiff1d(np.arange(S.nnz - 1), S.indptr[1:-1] - 1)].all()      # columns ascending per row
    # the libigl-convention Laplacian is this pencil divided by the mass and rounded: L = M^-1 C, C = -S
    L, lstatus = mesh_ops.libigl_laplacian(c.V, c.F, mass="voronoi")
    assert np.array_equal(L.indptr, S.indptr) and np.array_equal(L.indices, S.indices) and lstatus == status
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    with np.errstate(all="ignore"):
        want = ((0 - S.data) / mass[rows]).astype(np.float32)
    assert want.tobytes() == L.data.tobytes()
    assert mass.tobytes() == mesh_ops.descriptor_sums(c.V, c.F)["M_voronoi"].tobytes()
    assert S.diagonal().min() >= 0 and np.abs(S @ np.ones(S.shape[0])).max() <= 64 * EPS * np.abs(S.data).max()


def test_junk_raises_the_status_bits_and_clips_the_mass():
    S, mass, status = cases.pencil("junk")
    assert status == mesh_ops.DESC_BAD_FACE | mesh_ops.DESC_FLAT_FACE
    assert (mass == 0).sum() == 4 and (np.diff(S.indptr)[mass == 0] == 1).all()       # the diagonal alone, and it is zero
    ep = cases.statement("junk")[0]
    assert ep.status == status | mesh_ops.EIG_CLIPPED_MASS
    assert abs(ep.mass.sum() - 1) <= 64 * EPS and ep.mass.min() > 0
    assert (ep.values[:5] <= cases.TOL * ep.bound).all() and ep.values[5] > 1      # four massless vertices and the grid's constant


def test_start_block_is_a_function_of_seed_row_in_mesh_and_column():
    X = mesh_ops.spectral_start(7, [0, 5, 5, 12], 9)
    assert X.shape == (12, 9) and X.dtype == np.float64 and (X >= -0.5).all() and (X < 0.5).all()
    assert np.array_equal(X[:5], X[5:10]) and np.array_equal(X[:5], mesh_ops.spectral_start(7, [0, 5], 9))
    assert not np.array_equal(X, mesh_ops.spectral_start(8, [0, 5, 5, 12], 9))
    g, mask = mesh_ops._GOLDEN, mesh_ops._M64
    for r, c in ((0, 0), (3, 8), (6, 2)):          # the scalar definition
        h = mesh_ops._mix64((mesh_ops._mix64((7 + g + r) & mask) + g + c) & mask)
        assert X[5 + r, c] == (h >> 11) * 2.0 ** -53 - 0.5
    assert len(np.unique(X[5:])) == X[5:].size


@pytest.mark.parametrize("kind", ["single", "ragged", "empty_row"])
def test_filter_step_statement_against_a_dense_product(kind):
    f, Z = cases.filter_input(kind, 7), cases.filter_expected(kind, 7)
    import scipy.sparse as sp

    A = sp.csr_matrix((f.vals, f.colind, f.rowptr), shape=(len(f.rowptr) - 1,) * 2)
    per = lambda x: np.repeat(x, np.diff(f.voff))[:, None]
    want = per(f.alpha) * (A @ f.Y - per(f.shift) * f.Y) - per(f.beta) * f.X
    # every term is rounded a bounded number of times: (entries of the row + 4) eps on the sum of the magnitudes
    mag = np.abs(per(f.alpha)) * (abs(A) @ np.abs(f.Y) + np.abs(per(f.shift) * f.Y)) + np.abs(per(f.beta) * f.X)
    assert (np.abs(Z - want) <= (np.diff(f.rowptr).max() + 4) * EPS * mag).all()
    if kind == "empty_row":
        r = np.nonzero(np.diff(f.rowptr) == 0)[0]
        assert np.array_equal(Z[r], f.alpha[0] * (0.0 - f.shift[0] * f.Y[r]) - f.beta[0] * f.X[r])


def test_filter_scalars_are_the_chebyshev_recurrence():
    """The filter p(t) the scalars define equals C_deg((t - c) / e) / C_deg((a0 - c) / e): one on a0, at most 1 / C_deg(...) inside
    [a, b]."""
    a0, a, b, deg = 0.3, 40.0, 900.0, 9
    alpha, beta, shift = mesh_ops.cheb_filter_scalars(a0, a, b, deg)
    t = np.array([a0, a, 0.5 * (a + b), b, 7.0])
    old, cur = t * 0 + 1, alpha[0] * (t - shift[0])
    for j in range(1, deg):
        old, cur = cur, alpha[j] * (t - shift[j]) * cur - beta[j] * old
    cheb = lambda x: np.sign(x) ** deg * np.cosh(deg * np.arccosh(abs(x)))          # T_deg outside [-1, 1]
    e, c = (b - a) / 2, (b + a) / 2
    want = np.array([np.cos(deg * np.arccos(x)) if abs(x) <= 1 else cheb(x) for x in (t - c) / e]) / cheb((a0 - c) / e)
    assert np.abs(cur - want).max() <= 1e-12 and abs(cur[0] - 1) <= 1e-12
    assert np.abs(cur[1:4]).max() <= 1 / abs(cheb((a0 - c) / e)) + 1e-12 < 0.05 < cur[4]


@pytest.mark.parametrize("name", cases.NAMES)
def test_eigenvalues_and_residuals_stay_within_tol_times_the_bound(name):
    k = cases.case(name).k
    for ep, orc in zip(cases.statement(name), cases.oracle(name)):
        assert ep.status & mesh_ops.EIG_NOT_CONVERGED == 0 and ep.values.shape == (k,) and ep.vectors.shape == (len(orc.mass), k)
        assert abs(ep.bound - orc.bound) <= 64 * EPS * orc.bound
        err = np.abs(ep.values - orc.values[:k])          # paired in order: a missed eigenvalue shifts every later one
        print(f"{name}: outer {ep.outer_iterations}, max |theta - lambda| = {err.max():.3e}, max residual = {ep.residuals.max():.3e}, "
              f"tol b = {cases.TOL * ep.bound:.3e}")
        assert (np.diff(ep.values) >= 0).all()
        assert (err <= cases.TOL * ep.bound).all()
        assert (ep.residuals <= cases.TOL * ep.bound).all()


@pytest.mark.parametrize("name", cases.NAMES)
def test_returned_residuals_equal_a_recomputation_from_the_returned_pairs(name):
    rowptr, colind, A, d = cases.standard_form(name)
    off = cases.voff(name)
    x = np.concatenate([ep.vectors for ep in cases.statement(name)]) / d[:, None]
    one, zero = np.ones(len(off) - 1), np.zeros(len(off) - 1)
    Ax = mesh_ops.cheb_filter_step(rowptr, colind, A, off, one, zero, zero, x, x)
    for b, ep in enumerate(cases.statement(name)):
        p = slice(off[b], off[b + 1])
        r = np.sqrt(((Ax[p] - x[p] * ep.values) ** 2).sum(axis=0))
        print(f"{name}[{b}]: max |r - r'| = {np.abs(r - ep.residuals).max():.3e}, allowed {cases.RESIDUAL_SLACK_EPS * EPS * ep.bound:.3e}")
        assert (np.abs(r - ep.residuals) <= cases.RESIDUAL_SLACK_EPS * EPS * ep.bound).all()


def test_two_parts_has_two_zero_eigenvalues():
    ep = cases.statement("two_parts")[0]
    assert (np.abs(ep.values[:2]) <= cases.TOL * ep.bound).all() and ep.values[2] > 1


def test_one_outer_iteration_is_reported_as_not_converged():
    V, F = cases.parts("cloth20x17")[0]
    with pytest.warns(RuntimeWarning, match="did not reach tol"):
        ep = mesh_ops.laplacian_eigenpairs(V, F, k=cases.case("cloth20x17").k, max_outer=1)
    assert ep.status & mesh_ops.EIG_NOT_CONVERGED and ep.outer_iterations == 1
    assert not (ep.residuals <= cases.TOL * ep.bound).all()


@pytest.mark.parametrize("name", cases.NAMES)
def test_measured_bounds_orthonormality_and_wks(name):
    k = cases.case(name).k
    st = cases.statement(name)
    orth = max(cases.orthonormality(ep.vectors, ep.mass) for ep in st)
    wks = np.concatenate([mesh_ops.wave_kernel_signature(None, None, cases.N_WKS, k, ep, np.float64) for ep in st])
    err = cases.wks_error(wks, name)
    print(f"{name}: max |phi^T Am phi - I| = {orth:.3e} (bound {cases.ORTH_BOUND:.3e}), WKS error = {err:.3e} (bound {cases.WKS_BOUND:.3e})")
    assert wks.shape == (len(cases.case(name).V), cases.N_WKS) and np.isfinite(wks).all() and (wks >= 0).all()
    assert orth <= cases.ORTH_BOUND
    assert err <= cases.WKS_BOUND


@pytest.mark.parametrize("name", cases.NAMES)
def test_wks_statement_is_the_references_formula_on_the_same_eigenpairs(name):
    """mesh_ops.wks_weights / wks_contract against compute_wks as written, on the ORACLE's pairs: the two differ in the order of
    a sum of k non-negative terms, at most k eps relative each."""
    k = cases.case(name).k
    for o in cases.oracle(name):
        W, C = mesh_ops.wks_weights(o.values[:k], cases.N_WKS)
        got = mesh_ops.wks_contract(o.vectors[:, :k], W, C)
        want = cases.reference_wks(o.values[:k], o.vectors[:, :k])
        assert (np.abs(got - want) <= 4 * k * EPS * np.abs(want)).all()
    f32 = mesh_ops.wave_kernel_signature(None, None, cases.N_WKS, k, cases.statement(name)[0])
    assert f32.dtype == np.float32


def test_refusals():
    V, F = cases.parts("tetra")[0]
    for k in (0, 5):
        with pytest.raises(ValueError, match="k must lie in 1..4"):
            mesh_ops.laplacian_eigenpairs(V, F, k=k)
    with pytest.raises(ValueError, match="N >= 2 and k >= 2"):
        mesh_ops.wks_weights(np.array([0.0, 1.0]), 1)
    with pytest.raises(ValueError, match="N >= 2 and k >= 2"):
        mesh_ops.wks_weights(np.array([1.0]), 100)


def test_header_ctypes_and_plan_table_agree_on_the_new_symbols():
    from surfacenetworks_amd import _lib, kernels

    header = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    for name in ("sn_mesh_cot_pencil_f64", "sn_spectral_start_f64", "sn_cheb_filter_step_f64", "sn_wks_f64"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
        assert f"SN_PLAN_FN({name})" in table
    for macro in ("NOT_CONVERGED", "CLIPPED_MASS"):
        value = getattr(mesh_ops, "EIG_" + macro)
        assert re.search(rf"#define\s+SN_EIG_{macro}\s+{value}\b", header) and getattr(kernels, "EIG_" + macro) == value
        assert value & 31 == 0          # clear of the SN_DESC_* bits that share the word
    lib = _lib.load()
    # the pencil takes the workspace of the Laplacian it shares its phases with: one byte less is refused, by both
    ws = int(lib.sn_mesh_cot_laplacian_workspace_bytes(100, 200))
    one = ctypes.c_void_p(16)          # never dereferenced: the size is checked first
    assert lib.sn_mesh_cot_pencil_f64(one, one, 100, 200, 0, one, None, None, None, one, one, ws - 1, None) == -6
    assert lib.sn_mesh_cot_pencil_f64(one, one, 100, 200, 2, one, None, None, None, one, one, ws, None) == -2
    # argument errors are answered before anything is launched
    assert lib.sn_cheb_filter_step_f64(None, None, None, None, 1, 4, 0, None, None, None, None, None, None, None) == -2
    assert lib.sn_cheb_filter_step_f64(None, None, None, None, 0, 4, 3, None, None, None, None, None, None, None) == -2
    assert lib.sn_cheb_filter_step_f64(None, None, None, None, 1, 4, 3, None, None, None, None, None, None, None) == -1
    assert lib.sn_wks_f64(None, None, 1, 4, 0, 5, None, None, 1, None, None) == -2
    assert lib.sn_spectral_start_f64(0, None, 1, 4, 3, None, None) == -1
