"""Shared by tests/test_amplify.py (host) and tests/test_amplify_gpu.py (device): the meshes and their stored Laplacians, a
plain-numpy emulation of the written definition of the sparse x sparse product and of the symmetric scaling (include/sn_spmm.h,
"Sparse x sparse CSR products"), and the bound a differently ordered fp32 sum is held to.

The emulation: every product and every sum in np.float32 (one rounding each), the sum of entry (i, k) running over the entries
of A's row i in ascending column order from +0, exact zeros dropped afterwards.  It is vectorised along k only — row i keeps one
fp32 accumulator per column and adds a_ij * (row j of B) for j ascending — so the order inside every single sum is the definition's.

The bound, derived and never measured: a sum of n fp32 products, each rounded once, added in ANY order, lies within
gamma_n * T of the exact sum (gamma_n = n u / (1 - n u), u = 2^-24, T = sum_j |a_ij| |b_jk|; Higham, Accuracy and Stability of
Numerical Algorithms, eq. 3.5 with the product's rounding counted as one more factor: n additions at most n - 1, plus 1).  Two
orders therefore differ by at most 2 gamma_n T."""
import functools

import numpy as np
import scipy.sparse as sp

import intrinsic_cases as ic
from surfacenetworks_amd import mesh_ops

f32 = np.float32


def bipyramid(n=96):
    """Two apexes at z = +-1 over an n-gon ring with a wavy height: the apex rows of the Laplacian hold n + 1 entries, and every
    row of its square covers the whole matrix (n + 2 entries from (n + 2)^2 candidate products)."""
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(a), np.sin(a), 0.05 * np.cos(3 * a)], axis=1)
    V = np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], ring])
    i = np.arange(n)
    j = (i + 1) % n
    F = np.concatenate([np.stack([np.zeros(n, np.int64), 2 + i, 2 + j], 1), np.stack([np.ones(n, np.int64), 2 + j, 2 + i], 1)])
    return np.asarray(V, np.float32).astype(np.float64), F.astype(np.int64)


def torus():
    """The closed 12 x 9 torus grid (108 vertices of degree 6).  Its second squaring reaches 4 steps each way, all 9 columns
    of the short direction.  No sum of its sequence cancels exactly (measured with the emulation: 0 dropped in either squaring,
    for seeds 0..11 and without jitter); the dropped-zero case is flat_grid()."""
    V, F = mesh_ops.torus_grid(12, 9, np.random.default_rng(0))
    return np.asarray(V, np.float32).astype(np.float64), np.asarray(F, np.int64)


def flat_grid():
    """The regular flat 12 x 9 grid, unit spacing, z = 0: every value is shared by many entries, and 266 structural entries of
    the second squaring sum to exactly zero in fp32 — scipy drops them, and so does the definition."""
    ii, jj = np.meshgrid(np.arange(12.0), np.arange(9.0), indexing="ij")
    V = np.stack([ii.ravel(), jj.ravel(), np.zeros(ii.size)], axis=1)
    return V, mesh_ops._grid_faces(12, 9, wrap=False)


EXTRINSIC = ic.NAMES + ("torus", "flat", "bipyramid")
INTRINSIC = ("A", "E", "F_disc")
CASES = tuple(("ext", n) for n in EXTRINSIC) + tuple(("int", n) for n in INTRINSIC)
GPU_CASES = (("ext", "A"), ("ext", "F_disc"), ("int", "F_disc"), ("ext", "bipyramid"), ("ext", "torus"), ("ext", "flat"))


def mesh(name):
    if name == "torus":
        return torus()
    if name == "flat":
        return flat_grid()
    if name == "bipyramid":
        return bipyramid()
    return ic.meshes()[name]


@functools.lru_cache(maxsize=None)
def laplacian(kind, name):
    """The stored fp32 Laplacian of a case, columns ascending, as the reference's frames hold it."""
    V, F = mesh(name)
    L = ic.host_laplacian(name) if kind == "int" else mesh_ops.laplacian(V, F)
    L = sp.csr_matrix(L).astype(f32)
    L.sort_indices()
    return L


def inv_sqrt_degree(L):
    idp = L.indptr
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1 / np.sqrt(idp[1:] - idp[:-1] - 1)).astype(f32)


def _csr(rowptr, cols, vals, shape):
    return sp.csr_matrix((np.asarray(vals, f32), np.asarray(cols, np.int32), np.asarray(rowptr, np.int32)), shape=shape)


def drop_zeros(A):
    """The entries != 0 in order (explicit zeros removed, nothing summed or re-sorted)."""
    keep = A.data != 0
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))[keep]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))])
    return _csr(rowptr, A.indices[keep], A.data[keep], A.shape)


def emulate_scale(A, d, keep_zeros=False):
    """out_ij = fl(fl(d_i a_ij) d_j) on A's pattern, exact zeros dropped."""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    with np.errstate(invalid="ignore", over="ignore"):
        v = (d[rows].astype(f32) * A.data.astype(f32)).astype(f32) * d[A.indices].astype(f32)
    out = _csr(A.indptr, A.indices, v.astype(f32), A.shape)
    return out if keep_zeros else drop_zeros(out)


def emulate_spgemm(A, B, keep_zeros=False):
    """C = A B by the definition: A, B csr_matrix with ascending columns and fp32 data (explicit zeros allowed)."""
    M, N = A.shape[0], B.shape[1]
    assert A.shape[1] == B.shape[0] and A.data.dtype == f32 and B.data.dtype == f32
    rowptr, cols, vals = [0], [], []
    acc = np.zeros(N, f32)
    hit = np.zeros(N, bool)
    for i in range(M):
        acc[:] = 0
        hit[:] = False
        for p in range(A.indptr[i], A.indptr[i + 1]):          # ascending j
            j, a = A.indices[p], A.data[p]
            q0, q1 = B.indptr[j], B.indptr[j + 1]
            k = B.indices[q0:q1]
            with np.errstate(invalid="ignore", over="ignore"):
                acc[k] = acc[k] + a * B.data[q0:q1]            # fp32 product, then fp32 sum: two roundings
            hit[k] = True
        k = np.flatnonzero(hit)
        cols.append(k)
        vals.append(acc[k].copy())
        rowptr.append(rowptr[-1] + k.size)
    C = _csr(rowptr, np.concatenate(cols) if cols else [], np.concatenate(vals) if vals else [], (M, N))
    return C if keep_zeros else drop_zeros(C)


@functools.lru_cache(maxsize=None)
def emulated_sequence(kind, name):
    """([M0, M1, M2], [S1, S2], dropped): the three matrices of the definition in main.py's step order, the scaled operands of
    the two squarings (S_t squared is M_t) and the number of exact-zero sums dropped by each squaring."""
    L = laplacian(kind, name)
    d = inv_sqrt_degree(L)
    cur = emulate_scale(L, d)
    mats, scaled, dropped = [cur], [], []
    for _ in range(2):
        S = emulate_scale(cur, d)
        full = emulate_spgemm(S, S, keep_zeros=True)
        cur = drop_zeros(full)
        dropped.append(full.nnz - cur.nnz)
        scaled.append(S)
        mats.append(cur)
    return mats, scaled, dropped


def product_bound(A, B):
    """2 gamma_n T per structural entry of A B as a float64 csr_matrix on the structural pattern (see the module docstring)."""
    ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    absd = lambda X: sp.csr_matrix((np.abs(X.data.astype(np.float64)), X.indices, X.indptr), shape=X.shape)
    n = (ones(A) @ ones(B)).tocsr()
    T = (absd(A) @ absd(B) + 0 * n).tocsr()                    # on n's pattern even where T underflows
    n.sort_indices()
    T.sort_indices()
    nu = n.data * 2.0 ** -24
    bound = T.copy()
    bound.data = 2 * (nu / (1 - nu)) * T.data
    return bound


def compare_within_bound(X, Y, bound):
    """(worst ratio |x - y| / bound over the union pattern, entries stored on one side only); a missing entry counts as 0.
    An entry with bound 0 must agree exactly (ratio inf otherwise)."""
    X, Y = sp.csr_matrix(X).astype(np.float64), sp.csr_matrix(Y).astype(np.float64)
    px = sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    py = sp.csr_matrix((np.ones(Y.nnz), Y.indices, Y.indptr), shape=Y.shape)
    one_sided = int((abs(px - py)).sum())
    diff = abs(X - Y).tocoo()
    b = np.asarray(bound.tocsr()[diff.row, diff.col]).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff.data == 0, 0.0, diff.data / b)
    return (float(ratio.max()) if ratio.size else 0.0), one_sided


def same_csr(X, rowptr, colind, vals):
    """Bit identity of a csr_matrix with three arrays (values compared as their bit patterns)."""
    return (np.array_equal(X.indptr, np.asarray(rowptr)) and np.array_equal(X.indices, np.asarray(colind))
            and np.array_equal(X.data.view(np.int32), np.asarray(vals, f32).view(np.int32)))
