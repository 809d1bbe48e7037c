"""Shared by tests/test_spectral.py (host) and tests/test_spectral_gpu.py (device): the named meshes of the spectral tests (the
fp64 cotangent pencil, the Chebyshev-filtered eigen-solver, the wave kernel signature), their dense oracle and the inputs of the
kernel tests.  Every case is built from the mesh_ops generators and tests/descriptor_cases.py with a fixed seed; no mesh has
more than about 350 vertices and no case asks for more than 64 eigenpairs.

The oracle of a case is scipy.linalg.eigh(S.toarray(), diag(Am)) in fp64 per mesh, fed into geom_utils.compute_wks's formula
as written out in reference_wks below.  Every case asserts here, on that oracle, the condition under which its k-th eigenvector
(and with it the WKS) is defined at all — for eigsh as much as for this solver: (lambda_{k+1} - lambda_k) >= 1e-2 lambda_k.

The two measured bounds.  ORTH_MEASURED and WKS_MEASURED are the worst values over all cases of the HOST STATEMENT
(mesh_ops.laplacian_eigenpairs / wave_kernel_signature at tol = 1e-10) against the dense oracle, measured on the CPU
(tools/spectral_probe.py --measure-bounds prints them; LABNOTES.md#spectral has the table).  The test bound for the statement and
for the device is 16 x that: the device differs from the statement in the rounding order of library QR, eigh and products,
which changes the error constant, not its order."""
import collections
import functools

import numpy as np
import scipy.linalg

import descriptor_cases
from surfacenetworks_amd import mesh_ops

Case = collections.namedtuple("Case", "V F sizes k")      # the meshes as one disjoint mesh: V fp32 (n, 3), F int32 (nF, 3), vertex counts

NAMES = ("tetra", "cloth20x17", "sphere", "two_parts", "ragged_pair", "junk")
TOL = 1e-10
GAP = 1e-2
N_WKS = 100

# measured: the host statement against the dense oracle, worst case over NAMES (see the module docstring)
ORTH_MEASURED = 2.8e-15          # max |phi^T diag(Am) phi - I|                         (worst: ragged_pair, 2.78e-15)
WKS_MEASURED = 2.1e-10           # max |WKS - WKS_oracle| / max |WKS_oracle|            (worst: ragged_pair, 2.08e-10)
ORTH_BOUND = 16 * ORTH_MEASURED
WKS_BOUND = 16 * WKS_MEASURED
# |r_returned - r_recomputed| <= RESIDUAL_SLACK_EPS eps b: both are |A x - theta x|_2 of the same pair with |x|_2 = 1 to
# rounding; a component of A x - theta x carries at most (d + 2) eps (sum_j |A_ij| |x_j| + theta |x_i|) of rounding, d <= 24 + 1
# stored entries (SN_LAP_MAX_DEGREE), so the vector's error is below 27 eps (b + theta) <= 54 eps b, for each of the two; x
# recovered from phi = D x adds 2 eps relative, the rotation X Q of an m-column block m eps: 128 + 2 m covers the sum.
RESIDUAL_SLACK_EPS = 128 + 2 * 80


def _rng(seed):
    return np.random.default_rng(seed)


def _bumped_cloth(n, m, seed):
    V, F = mesh_ops.grid_cloth(n, m, _rng(seed))
    V = np.array(V, np.float64)
    c = V[:, :2].mean(axis=0)
    V[:, 2] += 0.3 * np.exp(-((V[:, 0] - c[0]) ** 2 + (V[:, 1] - c[1]) ** 2) / 0.05)
    return V, np.asarray(F)


def _union(parts):
    V, F, off = [], [], 0
    for v, f in parts:
        V.append(np.asarray(v, np.float64))
        F.append(np.asarray(f, np.int64) + off)
        off += len(v)
    return np.concatenate(V), np.concatenate(F)


def _build(name):
    if name == "tetra":
        # descriptor_cases' tetrahedron is regular, so its three non-zero eigenvalues coincide and k = 3 would cut through the
        # shell; stretched along the axes they split (the gap below is asserted like every other case's).  n = 4, k = 3: m = n
        c = descriptor_cases.case("tetra")
        return c.V.astype(np.float64) * np.array([1.0, 1.35, 0.7]), c.F, None, 3
    if name == "cloth20x17":
        return (*_bumped_cloth(20, 17, 3), None, 60)
    if name == "sphere":                                 # octahedral symmetry: exactly degenerate shells; 1 + 3 + 5 + 7 closes one
        c = descriptor_cases.case("sphere")
        return c.V, c.F, None, 16
    if name == "two_parts":                              # one mesh, two components: two zero eigenvalues
        V, F = _union([_bumped_cloth(11, 9, 5), mesh_ops.grid_cloth(8, 7, _rng(6))])
        return V, F, None, 24
    if name == "ragged_pair":                            # a batch of two different meshes
        a, b = _bumped_cloth(13, 11, 7), mesh_ops.torus_grid(8, 12, _rng(12))
        V, F = _union([a, b])
        return V, F, [len(a[0]), len(b[0])], 18
    if name == "junk":                                   # bad and flat faces, an isolated vertex: clipped mass, status bits
        c = descriptor_cases.case("junk")
        return c.V, c.F, None, 12
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    V, F, sizes, k = _build(name)
    V = np.ascontiguousarray(V, np.float32)
    F = np.ascontiguousarray(F, np.int32).reshape(-1, 3)
    for x in (V, F):
        x.setflags(write=False)
    return Case(V, F, tuple(sizes) if sizes is not None else (V.shape[0],), k)


def voff(name) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(case(name).sizes)]).astype(np.int32)


def parts(name):
    """[(V_b, F_b)] of the meshes of a case, each with its own vertex numbering (a face belongs to the mesh of its first index;
    junk's bad faces stay with its single mesh)."""
    c, off = case(name), voff(name)
    if len(c.sizes) == 1:
        return [(c.V, c.F)]
    out = []
    for b in range(len(c.sizes)):
        sel = (c.F[:, 0] >= off[b]) & (c.F[:, 0] < off[b + 1])
        out.append((c.V[off[b]:off[b + 1]], c.F[sel] - off[b]))
    return out


@functools.lru_cache(maxsize=None)
def pencil(name):
    """mesh_ops.cot_pencil of the whole case: (S scipy CSR fp64, mass, status)."""
    c = case(name)
    return mesh_ops.cot_pencil(c.V, c.F)


Oracle = collections.namedtuple("Oracle", "values vectors mass bound")      # per mesh: every eigenpair, ascending


@functools.lru_cache(maxsize=None)
def oracle(name):
    """[Oracle] per mesh from the dense generalised eigh; asserts the case's gap condition."""
    out = []
    for V, F in parts(name):
        S, mass, _ = mesh_ops.cot_pencil(V, F)
        Am, _ = mesh_ops.eig_normalised_mass(mass, [0, len(mass)])
        lam, phi = scipy.linalg.eigh(S.toarray(), np.diag(Am))
        d = 1 / np.sqrt(Am)
        A = d[:, None] * S.toarray() * d[None, :]
        k = case(name).k
        assert k < len(lam) and lam[k] - lam[k - 1] >= GAP * lam[k - 1], (name, k, lam[k - 1], lam[k])
        out.append(Oracle(lam, phi, Am, float(np.abs(A).sum(axis=1).max())))
    return out


def reference_wks(values, vectors, N=N_WKS):
    """geom_utils.compute_wks lines 423-440 on the eigenpairs of one mesh, line for line."""
    E = np.abs(np.real(values))
    phi = np.real(vectors)
    E_ind = np.argsort(E)
    E = E[E_ind]
    phi = phi[:, E_ind]
    logE = np.log(np.clip(E, 1e-6, np.inf)).T
    ee = np.linspace(logE[1], max(logE) / 1.02, N)
    sigma = (ee[1] - ee[0]) * 6
    C = np.zeros(N)
    WKS = np.zeros((phi.shape[0], N))
    for i in range(N):
        exp_sth = np.exp((-(ee[i] - logE) ** 2) / (2 * sigma ** 2))
        C[i] = np.sum(exp_sth)
        WKS[:, i] = np.dot(phi ** 2, exp_sth)
    return np.divide(WKS, np.tile(C.T, (phi.shape[0], 1)))


@functools.lru_cache(maxsize=None)
def oracle_wks(name):
    """(n, N_WKS) fp64: reference_wks on the k lowest oracle eigenpairs of every mesh, stacked."""
    k = case(name).k
    return np.concatenate([reference_wks(o.values[:k], o.vectors[:, :k]) for o in oracle(name)])


@functools.lru_cache(maxsize=None)
def statement(name):
    """[mesh_ops.Eigenpairs] per mesh: the host statement at the defaults but k (and tol = TOL)."""
    return [mesh_ops.laplacian_eigenpairs(V, F, k=case(name).k, tol=TOL) for V, F in parts(name)]


def orthonormality(vectors, mass) -> float:
    """max |phi^T diag(Am) phi - I| of one mesh."""
    G = vectors.T @ (mass[:, None] * vectors)
    return float(np.abs(G - np.eye(G.shape[0])).max())


def wks_error(got, name) -> float:
    """max |got - oracle| / max |oracle| over the whole case."""
    want = oracle_wks(name)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def standard_form(name):
    """(rowptr, colind, A, d) of the whole case with A = D S D as the solver forms it, mesh by mesh."""
    S, mass, _ = pencil(name)
    Am, _ = mesh_ops.eig_normalised_mass(mass, voff(name))
    d = 1 / np.sqrt(Am)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    return S.indptr, S.indices, (d[rows] * S.data) * d[S.indices], d


# ---- inputs of the kernel tests ---------------------------------------------------------------------------------------------
FILTER_WIDTHS = (1, 7, 64, 65, 72)
WKS_SHAPES = ((2, 2), (60, 100), (64, 7))      # (k, N)

FilterInput = collections.namedtuple("FilterInput", "rowptr colind vals voff alpha beta shift X Y")


@functools.lru_cache(maxsize=None)
def filter_input(kind: str, m: int) -> FilterInput:
    """A filter step on a real matrix.  "single": cloth20x17's standard form.  "ragged": ragged_pair's, its two meshes with
    different alpha, beta and shift.  "empty_row": junk's pencil with the rows of two vertices emptied (an isolated vertex of
    the pencil still has its diagonal; a row without any stored entry is a path of its own)."""
    rng = _rng(100 + m)
    name = {"single": "cloth20x17", "ragged": "ragged_pair", "empty_row": "junk"}[kind]
    rowptr, colind, vals, _ = standard_form(name)
    off = voff(name)
    if kind == "empty_row":
        S = pencil(name)[0].tolil()
        for r in (5, S.shape[0] - 1):
            S.rows[r], S.data[r] = [], []
        S = S.tocsr()
        rowptr, colind, vals = S.indptr, S.indices, S.data
        assert (np.diff(rowptr) == 0).sum() == 2
    B, n = len(off) - 1, len(rowptr) - 1
    alpha = rng.standard_normal(B) * 1e-3
    beta = rng.standard_normal(B)
    shift = 100.0 + 50 * rng.standard_normal(B)
    if B > 1:
        assert len(set(alpha)) == B and len(set(beta)) == B and len(set(shift)) == B
    out = FilterInput(rowptr.astype(np.int32), colind.astype(np.int32), np.array(vals, np.float64), off, alpha, beta, shift,
                      rng.standard_normal((n, m)), rng.standard_normal((n, m)))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def filter_expected(kind: str, m: int) -> np.ndarray:
    f = filter_input(kind, m)
    return mesh_ops.cheb_filter_step(f.rowptr, f.colind, f.vals, f.voff, f.alpha, f.beta, f.shift, f.X, f.Y)


WksInput = collections.namedtuple("WksInput", "phi voff W C")


@functools.lru_cache(maxsize=None)
def wks_input(k: int, N: int) -> WksInput:
    """phi (n, k) random over a two-mesh layout (37 + 64 vertices), W and C from two sets of positive values through
    mesh_ops.wks_weights."""
    rng = _rng(1000 * k + N)
    off = np.array([0, 37, 101], np.int32)
    WC = [mesh_ops.wks_weights(np.sort(rng.random(k) * 50.0), N) for _ in range(2)]
    out = WksInput(rng.standard_normal((101, k)), off, np.stack([w for w, _ in WC]), np.stack([c for _, c in WC]))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wks_expected(k: int, N: int) -> np.ndarray:
    w = wks_input(k, N)
    return np.concatenate([mesh_ops.wks_contract(w.phi[w.voff[b]:w.voff[b + 1]], w.W[b], w.C[b]) for b in range(2)])
