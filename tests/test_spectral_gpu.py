"""The spectral path on the device (include/sn_spmm.h, "Spectral").  The pencil, the filter step, the start block and the WKS
contraction are compared with their numpy statements bit for bit, no tolerance.  The solver and the WKS as a whole are held to
the same bounds as the host statement in tests/test_spectral.py: tol b where the bound is derived, 16 x the statement's own
measured error where it had to be measured (tests/spectral_cases.py has the figures)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import spectral_cases as cases
from surfacenetworks_amd import _lib, datasets, kernels, mesh_ops, operators

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # (a copy: the cases are read-only)


def _np(t):
    return t.cpu().numpy()


def _same(got, want):
    got = _np(got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint8) != want.view(np.uint8)).reshape(-1, got.itemsize).any(axis=1).sum())


def _sizes(name):
    c = cases.case(name)
    return list(c.sizes) if len(c.sizes) > 1 else None


@functools.lru_cache(maxsize=None)
def device(name) -> operators.Eigenpairs:
    c = cases.case(name)
    return operators.laplacian_eigenpairs(_dev(c.V), _dev(c.F), k=c.k, tol=cases.TOL, sizes=_sizes(name))


# ---- bit-exact: the kernels against their numpy statements ---------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_pencil_equals_the_host_statement_bit_for_bit(name):
    c = cases.case(name)
    S, mass, status = cases.pencil(name)
    rowptr, colind, vals, m, st = kernels.cot_pencil_from_mesh(_dev(c.V), _dev(c.F))
    _same(rowptr, S.indptr.astype(np.int32))
    _same(colind, S.indices.astype(np.int32))
    _same(vals, S.data)
    _same(m, mass)
    assert st == status
    import scipy.sparse as sp

    T = sp.csr_matrix((_np(vals), _np(colind), _np(rowptr)), shape=S.shape).T.tocsr()
    T.sort_indices()
    assert T.data.tobytes() == _np(vals).tobytes() and np.array_equal(T.indices, _np(colind))      # S = S^T bit for bit
    again = kernels.cot_pencil_from_mesh(_dev(c.V), _dev(c.F))
    assert all(torch.equal(a, b) for a, b in zip(again[:4], (rowptr, colind, vals, m)))


def test_pencil_of_a_batch_equals_the_per_mesh_statement():
    import descriptor_cases

    c = descriptor_cases.case("batch")
    Vg, Fg, B, nV, _ = operators._offset_batch("test", _dev(c.V), _dev(c.F))
    rowptr, colind, vals, mass, st = kernels.cot_pencil_from_mesh(Vg, Fg)
    per = [mesh_ops.cot_pencil(c.V[b], c.F) for b in range(B)]
    _same(vals, np.concatenate([S.data for S, _, _ in per]))
    _same(mass, np.concatenate([m for _, m, _ in per]))
    _same(colind, np.concatenate([S.indices + b * nV for b, (S, _, _) in enumerate(per)]).astype(np.int32))
    assert st == 0 and int(rowptr[-1]) == sum(S.nnz for S, _, _ in per)


def _step(f, X=None, Y=None, out=None):
    X = _dev(f.X) if X is None else X
    Y = _dev(f.Y) if Y is None else Y
    return kernels.cheb_filter_step(_dev(f.rowptr), _dev(f.colind), _dev(f.vals), _dev(f.voff), _dev(f.alpha), _dev(f.beta),
                                    _dev(f.shift), X, Y, out=out)


@pytest.mark.parametrize("m", cases.FILTER_WIDTHS)
@pytest.mark.parametrize("kind", ["single", "ragged", "empty_row"])
def test_filter_step_equals_its_numpy_statement_bit_for_bit(kind, m):
    f, want = cases.filter_input(kind, m), cases.filter_expected(kind, m)
    Z = _step(f)
    _same(Z, want)
    assert torch.equal(Z, _step(f))                                   # two runs are byte-identical


@pytest.mark.parametrize("m", cases.FILTER_WIDTHS)
def test_filter_step_with_z_aliasing_x(m):
    f, want = cases.filter_input("ragged", m), cases.filter_expected("ragged", m)
    X = _dev(f.X)
    Z = _step(f, X=X, out=X)
    assert Z.data_ptr() == X.data_ptr()
    _same(X, want)


def test_filter_step_refuses_z_aliasing_y():
    f = cases.filter_input("single", 7)
    Y = _dev(f.Y)
    with pytest.raises(_lib.SnError, match="status -2"):
        _step(f, Y=Y, out=Y)
    both = torch.empty(2 * Y.shape[0] - 1, Y.shape[1], dtype=torch.float64, device="cuda")      # a partial overlap with X
    X = both[: Y.shape[0]]
    X.copy_(Y)
    with pytest.raises(_lib.SnError, match="status -2"):
        _step(f, X=X, out=both[Y.shape[0] - 1:])


def test_start_block_equals_its_numpy_statement_bit_for_bit():
    off = np.array([0, 5, 5, 140, 341], np.int32)
    for seed, m in ((0, 76), (2 ** 63 + 11, 1), (7, 65)):
        X = kernels.spectral_start(seed, _dev(off), int(off[-1]), m)
        _same(X, mesh_ops.spectral_start(seed, off, m))


@pytest.mark.parametrize("k,N", cases.WKS_SHAPES)
def test_wks_contraction_equals_its_numpy_statement_bit_for_bit(k, N):
    w, want = cases.wks_input(k, N), cases.wks_expected(k, N)
    args = (_dev(w.phi), _dev(w.voff), _dev(w.W), _dev(w.C))
    got = kernels.wks_contract(*args, dtype=torch.float64)
    _same(got, want)
    _same(kernels.wks_contract(*args), want.astype(np.float32))
    assert torch.equal(got, kernels.wks_contract(*args, dtype=torch.float64))


# ---- derived bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_eigenvalues_and_residuals_stay_within_tol_times_the_bound(name):
    ep, k = device(name), cases.case(name).k
    off = cases.voff(name)
    assert ep.status == cases.statement(name)[0].status | (cases.statement(name)[-1].status)
    assert ep.values.shape == (len(off) - 1, k) and ep.vectors.shape == (off[-1], k) and ep.vectors.dtype == torch.float64
    assert np.array_equal(_np(ep.voff), off)
    for b, orc in enumerate(cases.oracle(name)):
        values, res, bound = _np(ep.values[b]), _np(ep.residuals[b]), float(ep.bound[b])
        assert abs(bound - orc.bound) <= 64 * EPS * orc.bound
        err = np.abs(values - orc.values[:k])             # paired in order: a missed eigenvalue shifts every later one
        print(f"{name}[{b}]: outer {int(ep.outer_iterations[b])} (statement {cases.statement(name)[b].outer_iterations}), "
              f"max |theta - lambda| = {err.max():.3e}, max residual = {res.max():.3e}, tol b = {cases.TOL * bound:.3e}")
        assert (np.diff(values) >= 0).all()
        assert (err <= cases.TOL * bound).all()
        assert (res <= cases.TOL * bound).all()


@pytest.mark.parametrize("name", cases.NAMES)
def test_returned_residuals_equal_a_recomputation_from_the_returned_pairs(name):
    ep = device(name)
    rowptr, colind, A, d = cases.standard_form(name)
    off = cases.voff(name)
    x = _np(ep.vectors) / d[:, None]
    one, zero = np.ones(len(off) - 1), np.zeros(len(off) - 1)
    Ax = mesh_ops.cheb_filter_step(rowptr, colind, A, off, one, zero, zero, x, x)
    for b in range(len(off) - 1):
        p = slice(off[b], off[b + 1])
        r = np.sqrt(((Ax[p] - x[p] * _np(ep.values[b])) ** 2).sum(axis=0))
        diff, allowed = np.abs(r - _np(ep.residuals[b])).max(), cases.RESIDUAL_SLACK_EPS * EPS * float(ep.bound[b])
        print(f"{name}[{b}]: max |r - r'| = {diff:.3e}, allowed {allowed:.3e}")
        assert diff <= allowed


def test_two_parts_has_two_zero_eigenvalues():
    ep = device("two_parts")
    values = _np(ep.values[0])
    assert (np.abs(values[:2]) <= cases.TOL * float(ep.bound[0])).all() and values[2] > 1


def test_junk_clips_the_mass_and_carries_the_pencils_status():
    ep = device("junk")
    assert ep.status == mesh_ops.DESC_BAD_FACE | mesh_ops.DESC_FLAT_FACE | mesh_ops.EIG_CLIPPED_MASS
    mass = _np(ep.mass)
    want = cases.statement("junk")[0].mass
    assert mass.min() > 0 and np.abs(mass - want).max() <= 4 * EPS * want.max()


def test_one_outer_iteration_warns_and_is_reported_as_not_converged():
    c = cases.case("cloth20x17")
    with pytest.warns(RuntimeWarning, match="did not reach tol"):
        ep = operators.laplacian_eigenpairs(_dev(c.V), _dev(c.F), k=c.k, max_outer=1)
    assert ep.status & kernels.EIG_NOT_CONVERGED and ep.outer_iterations.tolist() == [1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert device("cloth20x17").status & kernels.EIG_NOT_CONVERGED == 0


# ---- measured bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_measured_bounds_orthonormality_and_wks(name):
    c, ep, off = cases.case(name), device(name), cases.voff(name)
    phi, mass = _np(ep.vectors), _np(ep.mass)
    orth = max(cases.orthonormality(phi[off[b]:off[b + 1]], mass[off[b]:off[b + 1]]) for b in range(len(off) - 1))
    wks = operators.wave_kernel_signature(_dev(c.V), _dev(c.F), N=cases.N_WKS, eigenpairs=ep, dtype=torch.float64, sizes=_sizes(name))
    err = cases.wks_error(_np(wks), name)
    print(f"{name}: max |phi^T Am phi - I| = {orth:.3e} (bound {cases.ORTH_BOUND:.3e}), WKS error = {err:.3e} (bound {cases.WKS_BOUND:.3e})")
    assert wks.shape == (len(c.V), cases.N_WKS) and wks.dtype == torch.float64 and bool(torch.isfinite(wks).all())
    assert orth <= cases.ORTH_BOUND
    assert err <= cases.WKS_BOUND
    f32 = operators.wave_kernel_signature(_dev(c.V), _dev(c.F), N=cases.N_WKS, eigenpairs=ep, sizes=_sizes(name))
    assert f32.dtype == torch.float32 and torch.equal(f32, wks.float())


def test_a_batch_stays_within_the_measured_bounds_of_the_per_mesh_calls():
    """Three equally sized cloths through the batch axis: every mesh meets the oracle as it does alone, and the WKS keeps the
    leading axis."""
    k = 20
    meshes = [mesh_ops.grid_cloth(9, 8, np.random.default_rng(s)) for s in (41, 42, 43)]
    V = np.stack([np.asarray(v, np.float32) for v, _ in meshes])
    F = np.asarray(meshes[0][1], np.int32)
    ep = operators.laplacian_eigenpairs(_dev(V), _dev(F), k=k)
    wks = operators.wave_kernel_signature(_dev(V), _dev(F), eigenpairs=ep, dtype=torch.float64)
    assert wks.shape == (3, 72, 100) and ep.values.shape == (3, k) and ep.status == 0
    import scipy.linalg

    for b in range(3):
        S, mass, _ = mesh_ops.cot_pencil(V[b], F)
        Am, _ = mesh_ops.eig_normalised_mass(mass, [0, 72])
        lam, phi = scipy.linalg.eigh(S.toarray(), np.diag(Am))
        assert lam[k] - lam[k - 1] >= cases.GAP * lam[k - 1]
        want = cases.reference_wks(lam[:k], phi[:, :k])
        assert (np.abs(_np(ep.values[b]) - lam[:k]) <= cases.TOL * float(ep.bound[b])).all()
        assert np.abs(_np(wks[b]) - want).max() / np.abs(want).max() <= cases.WKS_BOUND
        alone = operators.wave_kernel_signature(_dev(V[b]), _dev(F), k=k, dtype=torch.float64)
        assert np.abs(_np(alone) - want).max() / np.abs(want).max() <= cases.WKS_BOUND


# ---- the interface -------------------------------------------------------------------------------------------------------------
def test_normal_frame_with_wks_inputs():
    c = cases.case("cloth20x17")
    base = datasets.normal_frame_from_mesh(c.V, c.F)
    frame = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "wks"), wks_k=c.k)
    assert base["input"] is base["V"] and "eigenpairs" not in base
    assert frame["input"].shape == (len(c.V), 103) and frame["input"].dtype == torch.float32
    assert torch.equal(frame["input"][:, :3], base["input"]) and torch.equal(frame["V"], base["V"])
    want = operators.wave_kernel_signature(frame["V"], frame["F"], eigenpairs=frame["eigenpairs"])
    assert torch.equal(frame["input"][:, 3:], want) and frame["eigenpairs"].values.shape == (1, c.k)
    swapped = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("wks", "V"), wks_k=c.k)
    assert torch.equal(swapped["input"][:, 100:], base["input"]) and torch.equal(swapped["input"][:, :100], want)
    with pytest.raises(ValueError, match="inputs is a sequence"):
        datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "hks"))


def test_refusals():
    c = cases.case("tetra")
    V, F = _dev(c.V), _dev(c.F)
    for k in (0, 5):
        with pytest.raises(ValueError, match="k must lie in 1..4"):
            operators.laplacian_eigenpairs(V, F, k=k)
    r = cases.case("ragged_pair")
    with pytest.raises(ValueError, match="k must lie in 1..96"):
        operators.laplacian_eigenpairs(_dev(r.V), _dev(r.F), k=97, sizes=list(r.sizes))
    with pytest.raises(ValueError, match="device tensors"):
        operators.laplacian_eigenpairs(c.V, c.F, k=2)
    with pytest.raises(ValueError, match="device tensors"):
        operators.laplacian_eigenpairs(torch.from_numpy(np.array(c.V)), F, k=2)
    import descriptor_cases

    fan = descriptor_cases.case("fan40")
    with pytest.raises(ValueError, match="SN_LAP_MAX_DEGREE"):
        operators.laplacian_eigenpairs(_dev(fan.V), _dev(fan.F), k=4)
    with pytest.raises(ValueError, match="N >= 2 and k >= 2"):
        operators.wave_kernel_signature(V, F, N=1, k=3)
    with pytest.raises(ValueError, match="N >= 2 and k >= 2"):
        operators.wave_kernel_signature(V, F, N=100, k=1)
