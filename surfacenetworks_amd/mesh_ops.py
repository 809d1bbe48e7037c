"""Sparse-direct construction of the Surface-Network operators from a triangle mesh (V, F).

Host-side (numpy/scipy, fp64 like the reference, cast to fp32 by the caller) restatement of the
reference's *dense* builders, which allocate O(F*V) memory and cannot reach the 5k-20k vertex
configurations:

    edge_lengths        <- mesh.dist                 src/utils/mesh.py:17-26
    heron_areas         <- mesh.area                 src/utils/mesh.py:67-80
    cotangent_weights   <- mesh.cotangent_weights    src/utils/mesh.py:102-112
    laplacian           <- graph.laplacian(normalized=False) then A^-1 * L
                                                     src/utils/graph.py:40-49, src/mesh_mnist/add_laplacian.py:47-48
    dirac               <- mesh.dirac                src/utils/mesh.py:35-64  (Q: mesh.py:28-33)

Everything is vectorised over faces; no dense (V,V) or (4F,4V) array is ever formed.  The results
are pinned against the imported reference on the golden fixtures (tests/golden/make_golden.py).

Also here: the synthetic mesh generators SURVEY.md §8(d) prescribes for the benchmark configs
(grid-cloth, torus-grid, seeded Delaunay) — there is no dataset in the reference tree.
"""
from __future__ import annotations

import collections
import dataclasses
import warnings

import numpy as np
import scipy.sparse as sp

from . import constants
# the status bits and limits of include/sn_spmm.h, kept once in constants.py and exposed here under the same names
from .constants import *  # noqa: F401,F403

__all__ = [
    "edge_lengths", "heron_areas", "cotangent_weights", "laplacian", "dirac", "mesh_operators",
    "grid_cloth", "torus_grid", "delaunay_disc", "read_ply_ascii",
    "locality_order", "edge_span", "MeshOrder", "permute_operator",
    "mesh_glue", "intrinsic_delaunay", "intrinsic_laplacian", "intrinsic_laplacian_from_lengths", "delaunay_margin",
    "IDT_THRESHOLD",
    "good_faces", "components", "compact", "largest_component", "Components", "Compacted", "CC_BAD_FACE", "CC_INTERNAL",
    "weld_vertices", "unique_faces", "orient_faces", "repair_mesh", "Welded", "UniqueFaces", "Oriented", "Repaired",
    "REPAIR_BAD_FACE", "REPAIR_NONFINITE", "REPAIR_NONORIENTABLE", "REPAIR_NONMANIFOLD", "REPAIR_INTERNAL",
    "descriptor_sums", "vertex_descriptors", "libigl_laplacian", "Descriptors", "LAP_MAX_DEGREE",
    "DESC_BAD_FACE", "DESC_FLAT_FACE", "DESC_NO_NORMAL", "DESC_CLAMPED", "DESC_DEGREE",
    "principal_curvatures", "curv4", "curv4_columns", "curvature_status_names", "PrincipalCurvatures", "CURV_FEW_POINTS",
    "CURV_NO_NORMAL", "CURV_OVERFLOW", "CURV_DEGENERATE", "CURV_MAX_RING", "CURV_MIN_POINTS", "CURV_PIVOT_FLOOR", "CURV_CLIP",
    "delaunay_2d", "poisson_disc", "poisson_grid", "mesh_digits", "lattice_orient", "lattice_incircle", "lattice_intensity",
    "lattice_draw", "canonical_faces", "snap_to_lattice", "Delaunay2D", "PoissonDisc", "MeshDigitsResult",
    "DT_DEGENERATE", "DT_DUPLICATE", "DT_RANGE", "DT_TOO_LARGE", "DT_NOT_CONVERGED", "DT_REJECTED", "DT_INTERNAL",
    "DELAUNAY_MAX_POINTS", "DELAUNAY_COORD_LIMIT", "MESHDIGITS_MAX_ATTEMPTS", "MESHDIGITS_Q", "MESHDIGITS_MIN_DET",
    "arap_weights", "arap_covariances", "arap_rotation_from_covariance", "arap_rotations", "arap_rhs", "arap_energy", "arap_cg",
    "arap_deform", "arap_handle_motion", "ArapWeights", "ArapSolve", "ArapResult", "ARAP_NOT_CONVERGED", "ARAP_BREAKDOWN",
    "ARAP_DEGENERATE", "ARAP_BAD_FACE", "ARAP_DEGREE", "ARAP_TOO_LARGE", "ARAP_REDUCE_WIDTH", "ARAP_JACOBI_SWEEPS", "ARAP_RANK_EPS", "ARAP_MAX_CG",
    "cot_pencil", "spectral_start", "cheb_filter_step", "cheb_filter_scalars", "eig_normalised_mass", "eig_guard",
    "laplacian_eigenpairs", "wks_weights", "wks_contract", "wave_kernel_signature", "Eigenpairs", "EIG_NOT_CONVERGED",
    "EIG_CLIPPED_MASS", "EIG_MASS_FLOOR",
    "hierarchy_scores", "handshake_matching", "coarsen_operator", "mesh_hierarchy", "MeshHierarchy",
]

_PERMS = np.array([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]])  # itertools.permutations order


def edge_lengths(V: np.ndarray, F: np.ndarray) -> np.ndarray:
    """(F,3) lengths l[f] = (|v0 v1|, |v1 v2|, |v2 v0|)  — the entries mesh.dist stores at (i,j)."""
    V = np.asarray(V, dtype=np.float64)
    i, j, k = F[:, 0], F[:, 1], F[:, 2]

    def d(a, b):
        return np.sqrt(((V[a] - V[b]) ** 2).sum(axis=1))

    return np.stack([d(i, j), d(j, k), d(k, i)], axis=1)


def heron_areas(l: np.ndarray) -> np.ndarray:
    """Heron's formula with the reference's 1e-6 floor for degenerate faces (mesh.py:75-78)."""
    lij, ljk, lki = l[:, 0], l[:, 1], l[:, 2]
    s = (lij + ljk + lki) / 2
    q = s * (s - lij) * (s - ljk) * (s - lki)
    out = np.full(l.shape[0], 1e-6)
    pos = q > 0
    out[pos] = np.sqrt(q[pos])
    return out


def cotangent_weights(F: np.ndarray, a: np.ndarray, l: np.ndarray, num_vertices: int):
    """W (symmetric cotangent weights, CSR) and A^-1 = diag(1/(A+1e-9)) as mesh.cotangent_weights.

    For every face and every ordered pair (i,j) of its vertices with k the third one:
        W[i,j] += (-l_ij^2 + l_jk^2 + l_ki^2) / (8 a_f + 1e-6);   A[i] += a_f/3/4  (once per permutation)
    """
    nF = F.shape[0]
    l2 = l ** 2                      # squares of (01, 12, 20)
    # squared length of the edge between local corners p,q
    e2 = np.empty((nF, 3, 3))
    e2[:, 0, 1] = e2[:, 1, 0] = l2[:, 0]
    e2[:, 1, 2] = e2[:, 2, 1] = l2[:, 1]
    e2[:, 2, 0] = e2[:, 0, 2] = l2[:, 2]
    rows, cols, vals = [], [], []
    denom = 8 * a + 1e-6
    for p, q, r in _PERMS:
        rows.append(F[:, p])
        cols.append(F[:, q])
        vals.append((-e2[:, p, q] + e2[:, q, r] + e2[:, r, p]) / denom)
    rows = np.stack(rows, axis=1).ravel()    # face-major, permutation-minor == reference loop order
    cols = np.stack(cols, axis=1).ravel()
    vals = np.stack(vals, axis=1).ravel()
    W = sp.coo_matrix((vals, (rows, cols)), shape=(num_vertices, num_vertices)).tocsr()
    W.eliminate_zeros()              # csr_matrix(dense) in the reference drops exact zeros
    A = np.zeros(num_vertices)
    np.add.at(A, rows, np.repeat(a / 3 / 4, 6))
    return W, sp.diags(1 / (A + 1e-9), 0)


def laplacian(V: np.ndarray, F: np.ndarray) -> sp.csr_matrix:
    """Mass-normalised cotangent Laplacian  L = A^-1 (D - W),  D = diag(column sums of W)."""
    V = np.asarray(V, dtype=np.float64)
    l = edge_lengths(V, F)
    a = heron_areas(l)
    W, Ainv = cotangent_weights(F, a, l, V.shape[0])
    d = np.asarray(W.sum(axis=0)).squeeze()
    L = sp.diags(d, 0) - W
    return (Ainv * L).tocsr()


def dirac(V: np.ndarray, F: np.ndarray):
    """Quaternionic Dirac operator D (4F x 4V) and its adjoint DA (4V x 4F) as mesh.dirac.

    Block (face i, corner vertex j), e = V[next] - V[next-next], a = 0:
        D [4i:4i+4, 4j:4j+4] = -Q(0,e) / (2 Af_i),     Q = [[a,-b,-c,-d],[b,a,-d,c],[c,d,a,-b],[d,-c,b,a]]
        DA[4j:4j+4, 4i:4i+4] = D_block^T * Af_i / Av_j,  Av_j = sum over incident faces of Af/3
    """
    V = np.asarray(V, dtype=np.float64)
    nV, nF = V.shape[0], F.shape[0]
    Af = heron_areas(edge_lengths(V, F))
    Av = np.zeros(nV)
    np.add.at(Av, F.ravel(), np.repeat(Af / 3, 3))       # face-major, corner-minor like the reference loop
    # (row r, col c, sign, component of e) of the 12 non-zeros of Q(0,e) with e = (0,b,c,d) -> index 0,1,2
    q_pat = [(0, 1, -1, 0), (0, 2, -1, 1), (0, 3, -1, 2),
             (1, 0, +1, 0), (1, 2, -1, 2), (1, 3, +1, 1),
             (2, 0, +1, 1), (2, 1, +1, 2), (2, 3, -1, 0),
             (3, 0, +1, 2), (3, 1, -1, 1), (3, 2, +1, 0)]
    fi = np.arange(nF)
    d_rows, d_cols, d_vals, da_vals = [], [], [], []
    for corner in range(3):
        j = F[:, corner]
        e = V[F[:, (corner + 1) % 3]] - V[F[:, (corner + 2) % 3]]      # (F,3)
        scale = 2 * Af
        for r, c, sgn, comp in q_pat:
            m = -(sgn * e[:, comp]) / scale                # entry of  -Q/(2Af)
            d_rows.append(4 * fi + r)
            d_cols.append(4 * j + c)
            d_vals.append(m)
            da_vals.append(m * Af / Av[j])                 # mat.T * Af / Av lands at (4j+c, 4i+r)
    d_rows = np.concatenate(d_rows)
    d_cols = np.concatenate(d_cols)
    D = sp.coo_matrix((np.concatenate(d_vals), (d_rows, d_cols)), shape=(4 * nF, 4 * nV)).tocsr()
    DA = sp.coo_matrix((np.concatenate(da_vals), (d_cols, d_rows)), shape=(4 * nV, 4 * nF)).tocsr()
    D.eliminate_zeros()
    DA.eliminate_zeros()
    D.sort_indices()
    DA.sort_indices()
    return D, DA


def mesh_operators(V: np.ndarray, F: np.ndarray, dtype=np.float32):
    """{'L','Di','DiA'} in CSR with `dtype` values — the per-sample record the reference stores
    (src/mesh_mnist/add_laplacian.py:63-71, src/as_rigid_as_possible/add_laplacian.py:61-65)."""
    L = laplacian(V, F)
    Di, DiA = dirac(V, F)
    return {"L": L.astype(dtype), "Di": Di.astype(dtype), "DiA": DiA.astype(dtype)}


# --------------------------------------------------------------------------------------------------
# intrinsic Delaunay triangulation and its Laplacian (definition: include/sn_spmm.h, "Intrinsic Delaunay Laplacian").
# Bobenko & Springborn 2007 for the triangulation, Fisher et al. 2006 for the edge-flip algorithm.  The state is a
# Delta-complex keyed by FACE SIDES (code 3 f + s): after flips two faces may share two edges, a face may have a self-edge and
# one vertex pair may carry several edges, so nothing here is keyed by vertex pairs.
# --------------------------------------------------------------------------------------------------


def mesh_glue(F: np.ndarray, num_vertices: int) -> np.ndarray:
    """(nF, 3) glue map of a manifold, consistently oriented mesh: G[f, s] = 3 g + t, the side that traverses the edge
    F[f, s] -> F[f, s+1] the other way, -1 on the boundary.  ValueError names the refusal: a face with an index outside
    0..nV-1 or a repeated index; an edge with more than two faces; an edge its two faces traverse in the same direction."""
    F = np.asarray(F)
    nF = F.shape[0]
    if nF and (F.min() < 0 or F.max() >= num_vertices):
        raise ValueError("mesh_glue: a face has an index outside 0..nV-1")
    if nF and ((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 2] == F[:, 0])).any():
        raise ValueError("mesh_glue: a face has a repeated index")
    sides = {}
    for f in range(nF):
        for s in range(3):
            sides.setdefault((int(F[f, s]), int(F[f, (s + 1) % 3])), []).append(3 * f + s)
    same = any(len(v) > 1 for v in sides.values())
    if any(len(v) + len(sides.get((b, a), ())) > 2 for (a, b), v in sides.items()):
        raise ValueError("mesh_glue: an edge has more than two faces (the mesh is not manifold)")
    if same:
        raise ValueError("mesh_glue: an edge is traversed in the same direction by its two faces (the mesh is not "
                         "consistently oriented)")
    G = np.full((nF, 3), -1, dtype=np.int64)
    for (a, b), v in sides.items():
        twin = sides.get((b, a))
        if twin:
            G[v[0] // 3, v[0] % 3] = twin[0]
    return G


def _heron_q(a, b, c):
    s = ((a + b) + c) / 2
    return ((s * (s - a)) * (s - b)) * (s - c)


def _side_cot(l, f, s):
    """cot of the angle opposite side s of face f, (b^2 + c^2 - a^2) / (4 A); None for a degenerate face (radicand <= 0)."""
    a, b, c = l[f, s], l[f, (s + 1) % 3], l[f, (s + 2) % 3]
    q = _heron_q(a, b, c)
    if not q > 0:
        return None
    return ((b * b + c * c) - a * a) / (4 * np.sqrt(q))


def delaunay_margin(l: np.ndarray, G: np.ndarray):
    """(smallest cot_f + cot_g over the interior sides whose two faces are distinct and not degenerate, number of degenerate
    faces): the state is intrinsic Delaunay iff the first is >= IDT_THRESHOLD."""
    best, nF = np.inf, l.shape[0]
    for f in range(nF):
        for s in range(3):
            p = int(G[f, s])
            if p < 0 or p // 3 == f:
                continue
            cf, cg = _side_cot(l, f, s), _side_cot(l, p // 3, p % 3)
            if cf is not None and cg is not None:
                best = min(best, cf + cg)
    return best, int(sum(not _heron_q(*l[f]) > 0 for f in range(nF)))


def _flip(Fp, l, G, f, s):
    """Flip the side (f, s) glued to (g, t), as the header defines it: f = (i, j, k), g = (j, i, m) become f = (k, i, m),
    g = (m, j, k); sides 2 are the new edge."""
    p = int(G[f, s])
    g, t = p // 3, p % 3
    s1, s2, t1, t2 = (s + 1) % 3, (s + 2) % 3, (t + 1) % 3, (t + 2) % 3
    i, j, k, m = Fp[f, s], Fp[f, s1], Fp[f, s2], Fp[g, t2]
    a, ljk, lki, lim, lmj = l[f, s], l[f, s1], l[f, s2], l[g, t1], l[g, t2]
    # i at the origin, j at (a, 0), k above and m below the axis
    a2 = a * a
    xk = ((a2 + lki * lki) - ljk * ljk) / (2 * a)
    xm = ((a2 + lim * lim) - lmj * lmj) / (2 * a)
    yk = np.sqrt(max((lki - xk) * (lki + xk), 0.0))
    ym = -np.sqrt(max((lim - xm) * (lim + xm), 0.0))
    dx, dy = xk - xm, yk - ym
    lkm = np.sqrt(dx * dx + dy * dy)
    # the four outer sides: old code -> new code;  a partner that is itself one of them is remapped first
    remap = {3 * f + s1: 3 * g + 1, 3 * f + s2: 3 * f, 3 * g + t1: 3 * f + 1, 3 * g + t2: 3 * g}
    partner = {new: remap.get(int(G[old // 3, old % 3]), int(G[old // 3, old % 3])) for old, new in remap.items()}
    Fp[f] = (k, i, m)
    Fp[g] = (m, j, k)
    l[f] = (lki, lim, lkm)
    l[g] = (lmj, ljk, lkm)
    for new, q in partner.items():
        G[new // 3, new % 3] = q
        if q >= 0:
            G[q // 3, q % 3] = new
    G[f, 2], G[g, 2] = 3 * g + 2, 3 * f + 2


def intrinsic_delaunay(V: np.ndarray, F: np.ndarray, order: str = "fifo", seed: int = 0):
    """(F', l', flips): the intrinsic Delaunay triangulation of the mesh (V, F) by edge flips — faces (nF, 3), fp64 side
    lengths (nF, 3) in the layout of edge_lengths, and the number of flips.  V is rounded to fp32 first (the device reads fp32
    coordinates), everything after that is fp64.  order: "fifo" | "lifo" | "random" (seeded) — the work-list discipline; the
    triangulation does not depend on it unless four vertices are cocircular, only the flip count and the last bits of l' do.
    Plain Python loops over a work list: the yardstick of the device builder and the CPU path of dataset construction, slow at
    FAUST size (half a second for 13 780 faces and 13 000 flips, some 600 times the device builder: LABNOTES.md#intrinsic).
    Raises ValueError for a mesh mesh_glue refuses."""
    if order not in ("fifo", "lifo", "random"):
        raise ValueError('intrinsic_delaunay: order must be "fifo", "lifo" or "random"')
    Fp, l, G, flips = _intrinsic_state(V, F, order, seed)
    return Fp, l, flips


def _intrinsic_state(V, F, order="fifo", seed=0):
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    Fp = np.array(F, dtype=np.int64)
    G = mesh_glue(Fp, V.shape[0])
    l = edge_lengths(V, Fp)
    rng = np.random.default_rng(seed)
    from collections import deque

    work = deque(range(3 * Fp.shape[0]))
    flips = 0
    while work:
        if order == "fifo":
            c = work.popleft()
        elif order == "lifo":
            c = work.pop()
        else:
            k = int(rng.integers(len(work)))
            work[k], work[-1] = work[-1], work[k]
            c = work.pop()
        f, s = c // 3, c % 3
        p = int(G[f, s])
        if p < 0 or p // 3 == f:
            continue
        cf, cg = _side_cot(l, f, s), _side_cot(l, p // 3, p % 3)
        if cf is None or cg is None or not cf + cg < IDT_THRESHOLD:
            continue
        _flip(Fp, l, G, f, s)
        flips += 1
        g = p // 3
        work.extend((3 * f, 3 * f + 1, 3 * g, 3 * g + 1))      # the four outer sides, where they are now
    return Fp, l, G, flips


def intrinsic_laplacian_from_lengths(Fp: np.ndarray, l: np.ndarray, num_vertices: int, dtype=np.float64) -> sp.csr_matrix:
    """L = A^-1 (D - W) of a Delta-complex given by faces and side lengths, in this project's convention and in the
    summation order of the device builder: per face and ordered pair (p, q, r), w = (-l_pq^2 + l_qr^2 + l_rp^2)/(8a + 1e-6)
    goes to W[F[p], F[q]], its mirror (-l_qp^2 + l_pr^2 + l_rq^2)/(8a + 1e-6) to the column sum d[F[p]], a/3/4 to A[F[p]];
    a pair with F[p] == F[q] (a self-edge) contributes its mass only.  Every entry is the serial sum of its contributions in
    (face, permutation) order.  Pattern: every vertex pair joined by an edge plus the whole diagonal, zeros kept."""
    Fp = np.asarray(Fp)
    nF, nV = Fp.shape[0], int(num_vertices)
    a = heron_areas(l)
    l2 = l * l
    e2 = np.empty((nF, 3, 3))
    e2[:, 0, 1] = e2[:, 1, 0] = l2[:, 0]
    e2[:, 1, 2] = e2[:, 2, 1] = l2[:, 1]
    e2[:, 2, 0] = e2[:, 0, 2] = l2[:, 2]
    den = 8 * a + 1e-6
    W, d, A = {}, np.zeros(nV), np.zeros(nV)
    for f in range(nF):
        for p, q, r in _PERMS:
            i, j = int(Fp[f, p]), int(Fp[f, q])
            A[i] += a[f] / 3 / 4
            if i == j:
                continue
            W[(i, j)] = W.get((i, j), 0.0) + ((-e2[f, p, q] + e2[f, q, r]) + e2[f, r, p]) / den[f]
            d[i] += ((-e2[f, q, p] + e2[f, p, r]) + e2[f, r, q]) / den[f]
    ainv = 1 / (A + 1e-9)
    rows = [i for i, _ in W] + list(range(nV))
    cols = [j for _, j in W] + list(range(nV))
    vals = [ainv[i] * (0 - w) for (i, _), w in W.items()] + list(ainv * d)
    o = np.lexsort((cols, rows))
    rows, cols, vals = np.asarray(rows)[o], np.asarray(cols)[o], np.asarray(vals)[o]
    rowptr = np.zeros(nV + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=nV), out=rowptr[1:])
    return sp.csr_matrix((vals.astype(dtype), cols.astype(np.int32), rowptr), shape=(nV, nV))


def intrinsic_laplacian(V: np.ndarray, F: np.ndarray, order: str = "fifo", seed: int = 0) -> sp.csr_matrix:
    """The reference's mesh.intrinsic_laplacian by name (src/utils/mesh.py imports an unpublished module for it): this
    project's mass-normalised cotangent Laplacian A^-1 (D - W) on the intrinsic Delaunay triangulation of (V, F), fp64 CSR.
    Scaling and sign of the unpublished matrix are unknown; this is not a reproduction of it.  Every off-diagonal weight of an
    interior edge is >= 0 (the maximum principle the extrinsic operator lacks).  Host loops: slow at FAUST size."""
    Fp, l, _ = intrinsic_delaunay(V, F, order, seed)
    return intrinsic_laplacian_from_lengths(Fp, l, np.asarray(V).shape[0])


# --------------------------------------------------------------------------------------------------
# mesh clean-up: components, the largest one, compaction (definition: include/sn_spmm.h, "Mesh clean-up").  The host statement
# of igl.facet_components + scipy.stats.mode + igl.slice + igl.remove_unreferenced as the reference's
# src/dense_correspondence/largest_component.py:28-47 chains them; what the device kernels are compared to, bit for bit.
# --------------------------------------------------------------------------------------------------
Components = collections.namedtuple("Components", "vlabel flabel count summary status")
Compacted = collections.namedtuple("Compacted", "I J Fsrc Fnew Vnew sizes")


def good_faces(F: np.ndarray, num_vertices: int) -> np.ndarray:
    """(nF,) bool: all three indices inside 0..nV-1 and pairwise different."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    inside = ((F >= 0) & (F < num_vertices)).all(axis=1)
    return inside & (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])


def _class_minima(n: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """label[x] = the smallest node of x's class under the equivalence generated by a[i] ~ b[i].  Rounds of: every pair whose
    ends carry different labels lowers the larger label's own label to the smaller (minimum over the pairs), then labels are
    chased to their fixed point.  Labels only decrease and never leave the class; a round without such a pair ends it."""
    label = np.arange(n, dtype=np.int64)
    while a.size:
        la, lb = label[a], label[b]
        live = la != lb
        if not live.any():
            break
        a, b, la, lb = a[live], b[live], la[live], lb[live]
        np.minimum.at(label, np.maximum(la, lb), np.minimum(la, lb))
        while True:
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
    return label


def components(F: np.ndarray, num_vertices: int, mode: str = "edge") -> Components:
    """Connected components of a triangle mesh: Components(vlabel, flabel, count, summary, status), int32 arrays and a Python
    int.  mode "vertex": vertices are joined by the good faces that hold them, a label is the smallest vertex id of a class,
    flabel[f] = vlabel[F[f, 0]], count has nV entries.  mode "edge" (igl.facet_components): good faces are joined across a
    shared unordered vertex pair — any number of faces on an edge, any orientation; a shared vertex alone joins nothing — a
    label is the smallest face id, count has nF entries, vlabel is None.  A bad face has flabel -1 and sets CC_BAD_FACE.
    summary = (labels with a face, the winner: largest count, smallest label on a tie, its count), (0, -1, 0) without faces."""
    if mode not in ("edge", "vertex"):
        raise ValueError(f'components: mode must be "edge" or "vertex", got {mode!r}')
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV, nF = int(num_vertices), F.shape[0]
    good = good_faces(F, nV)
    Fg, fid = F[good], np.nonzero(good)[0]
    flabel = np.full(nF, -1, dtype=np.int64)
    vlabel = None
    if mode == "vertex":
        vlabel = _class_minima(nV, np.concatenate([Fg[:, 0], Fg[:, 1]]), np.concatenate([Fg[:, 1], Fg[:, 2]]))
        flabel[fid] = vlabel[Fg[:, 0]]
        n = nV
    else:
        a = np.concatenate([Fg[:, 0], Fg[:, 1], Fg[:, 2]])
        b = np.concatenate([Fg[:, 1], Fg[:, 2], Fg[:, 0]])
        key = np.minimum(a, b) * max(nV, 1) + np.maximum(a, b)
        face = np.concatenate([fid, fid, fid])
        order = np.argsort(key, kind="stable")
        same = key[order][1:] == key[order][:-1]                  # neighbours in the sorted list on one edge: a chain per edge
        flabel[fid] = _class_minima(nF, face[order][:-1][same], face[order][1:][same])[fid]
        n = nF
    count = np.bincount(flabel[fid], minlength=n).astype(np.int32)
    if fid.size:
        win = int(np.argmax(count))                               # the first maximum: the smallest label among the largest
        summary = np.array([np.count_nonzero(count), win, count[win]], dtype=np.int32)
    else:
        summary = np.array([0, -1, 0], dtype=np.int32)
    return Components(None if vlabel is None else vlabel.astype(np.int32), flabel.astype(np.int32), count, summary,
                      0 if good.all() else CC_BAD_FACE)


def compact(V, F: np.ndarray, keep, num_vertices: int = None) -> Compacted:
    """igl.slice + igl.remove_unreferenced: keep the good faces with keep[f] != 0 and the vertices they use.
    Compacted(I, J, Fsrc, Fnew, Vnew, sizes): I (nV,) old -> new vertex id, -1 for a dropped vertex; J (nV',) new -> old,
    ascending; Fsrc (nF',) the original index of every kept face, ascending; Fnew = I[F[Fsrc]]; Vnew = V[J] (None without V);
    sizes = (nV', nF').  num_vertices is needed only when V is None."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV = int(np.asarray(V).shape[0] if V is not None else num_vertices)
    stay = good_faces(F, nV) & (np.asarray(keep).reshape(-1) != 0)
    Fsrc = np.nonzero(stay)[0]
    used = np.zeros(nV, dtype=bool)
    used[F[Fsrc].ravel()] = True
    J = np.nonzero(used)[0]
    I = np.full(nV, -1, dtype=np.int64)
    I[J] = np.arange(J.size)
    return Compacted(I.astype(np.int32), J.astype(np.int32), Fsrc.astype(np.int32), I[F[Fsrc]].astype(np.int32).reshape(-1, 3),
                     None if V is None else np.asarray(V)[J], np.array([J.size, Fsrc.size], dtype=np.int32))


def largest_component(V, F: np.ndarray, connectivity: str = "edge"):
    """(V', F', J, Fsrc): the component with the most faces (on a tie the one with the smallest label) with its vertices
    renumbered in ascending order, J its vertices' and Fsrc its faces' original indices — largest_component.py:28-47.
    ValueError when no good face exists."""
    V = np.asarray(V)
    cc = components(F, V.shape[0], connectivity)
    if cc.summary[1] < 0:
        raise ValueError("largest_component: the mesh has no face with three distinct vertices of the mesh")
    out = compact(V, F, cc.flabel == cc.summary[1])
    return out.Vnew, out.Fnew, out.J, out.Fsrc


# --------------------------------------------------------------------------------------------------
# mesh repair: weld, duplicate faces, orientation (definition: include/sn_spmm.h, "Mesh repair").  The host statement of
# igl.remove_duplicate_vertices + igl.bfs_orient and the face filter of src/normal_predict/fix_degenerate.py, by sorting and
# frontier sweeps; what the device's hash tables and parity union-find are compared to, bit for bit.
# --------------------------------------------------------------------------------------------------
Welded = collections.namedtuple("Welded", "rep F counts status")
UniqueFaces = collections.namedtuple("UniqueFaces", "keep counts status")
Oriented = collections.namedtuple("Oriented", "flip label F counts status")
Repaired = collections.namedtuple("Repaired", "V F vertex_map vertex_index face_map flipped welded_vertices bad_faces "
                                              "duplicate_faces degenerate_faces nonmanifold_edges nonorientable_classes classes")


def _group_minima(cols, ids: np.ndarray) -> np.ndarray:
    """For rows given as equally long key columns: the smallest id among the rows equal to each row, in the order of ids."""
    if ids.size == 0:
        return ids.copy()
    order = np.lexsort(tuple(cols[::-1]))
    new = np.zeros(ids.size, dtype=bool)
    new[0] = True
    for c in cols:
        s = c[order]
        new[1:] |= s[1:] != s[:-1]
    start = np.nonzero(new)[0]
    low = np.minimum.reduceat(ids[order], start)
    out = np.empty_like(ids)
    out[order] = np.repeat(low, np.diff(np.append(start, ids.size)))
    return out


def weld_vertices(V: np.ndarray, F: np.ndarray, tol: float = 0.0, weld: bool = True) -> Welded:
    """Steps 1 and 2: Welded(rep, F, counts, status).  rep (nV,) int32 the smallest vertex id with v's key (v itself for an
    unweldable vertex); F (nF, 3) int32 through rep, -1 for an unweldable vertex, an index outside 0..nV-1 unchanged; counts
    (1,) = vertices with rep != id.  tol == 0: fp32 values (-0.0 == +0.0); tol > 0: the grid rint(float64(x) / tol), a quotient
    outside +-2**62 unweldable.  weld=False: rep is the identity and only non-finite coordinates are unweldable."""
    tol = float(tol)
    if not 0.0 <= tol < np.inf:
        raise ValueError(f"weld_vertices: tol must be finite and >= 0, got {tol!r}")
    V = np.asarray(V, dtype=np.float32).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV = V.shape[0]
    ok = np.isfinite(V).all(axis=1)
    rep = np.arange(nV, dtype=np.int64)
    if weld:
        if tol > 0:
            with np.errstate(all="ignore"):
                q = np.rint(V.astype(np.float64) / tol)
                ok &= (np.abs(q) <= 2.0 ** 62).all(axis=1)
            key = q[ok].astype(np.int64)
        else:
            key = V[ok]                                             # sorted and compared as values: -0.0 == +0.0
        ids = np.nonzero(ok)[0]
        rep[ids] = _group_minima([key[:, 0], key[:, 1], key[:, 2]], ids)
    inside = (F >= 0) & (F < nV)
    Fc = np.where(inside, F, 0)
    Fw = np.where(inside, np.where(ok[Fc], rep[Fc], -1), F)
    status = REPAIR_NONFINITE if (inside & ~ok[Fc]).any() else 0
    return Welded(rep.astype(np.int32), Fw.astype(np.int32), np.array([np.count_nonzero(rep != np.arange(nV))], dtype=np.int32),
                  status)


def unique_faces(F: np.ndarray, num_vertices: int, V=None, unique: bool = True) -> UniqueFaces:
    """Step 3: UniqueFaces(keep, counts, status).  keep (nF,) int32 = 1 for a good face with the smallest face id on its
    unordered vertex triple (unique=False: every good face); counts (3,) = bad faces, duplicate faces, kept faces whose fp64
    squared double-area is exactly 0 (0 without V)."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV = int(num_vertices)
    good = good_faces(F, nV)
    fid = np.nonzero(good)[0]
    keep = good.copy()
    if unique:
        T = np.sort(F[fid], axis=1)
        keep[fid] = _group_minima([T[:, 0], T[:, 1], T[:, 2]], fid) == fid
    flat = 0
    if V is not None:
        P = np.asarray(V, dtype=np.float32).astype(np.float64)
        K = F[keep]
        u, w = P[K[:, 1]] - P[K[:, 0]], P[K[:, 2]] - P[K[:, 0]]
        with np.errstate(all="ignore"):
            c = _cross3(u, w)
            flat = np.count_nonzero(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) == 0.0)
    counts = np.array([F.shape[0] - fid.size, fid.size - np.count_nonzero(keep), flat], dtype=np.int32)
    return UniqueFaces(keep.astype(np.int32), counts, 0 if good.all() else REPAIR_BAD_FACE)


def orient_faces(F: np.ndarray, keep, num_vertices: int) -> Oriented:
    """Step 4: Oriented(flip, label, F, counts, status) for the good faces with keep[f] != 0.  An edge with exactly two of them
    is a link; label (nF,) int32 = the smallest face id of the class under links, -1 for a face that takes no part; flip (nF,)
    int32 = 1 where (a, b, c) becomes (a, c, b) so that every link is traversed in opposite directions, the smallest face of a
    class keeping its winding; a class that has no such winding is left as it came.  counts (3,) = edges with three and more
    faces, classes without a consistent winding, classes.  The parities spread from the class minima, a frontier at a time."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV, nF = int(num_vertices), F.shape[0]
    good = good_faces(F, nV)
    part = good & (np.asarray(keep).reshape(-1) != 0)
    fid = np.nonzero(part)[0]
    Fk = F[fid]
    a = np.concatenate([Fk[:, 0], Fk[:, 1], Fk[:, 2]])
    b = np.concatenate([Fk[:, 1], Fk[:, 2], Fk[:, 0]])
    face = np.concatenate([fid, fid, fid])
    key = np.minimum(a, b) * max(nV, 1) + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.nonzero(np.append(True, ks[1:] != ks[:-1]))[0] if ks.size else np.zeros(0, dtype=np.int64)
    size = np.diff(np.append(start, ks.size))
    two = start[size == 2]
    s0, s1 = order[two], order[two + 1]
    lf, lg, lp = face[s0], face[s1], (a[s0] == a[s1]).astype(np.int64)      # the same direction twice: one of the two turns
    label = np.full(nF, -1, dtype=np.int64)
    label[fid] = _class_minima(nF, lf, lg)[fid]
    # the neighbours of every face over its links, as a CSR list
    src, dst, par = np.concatenate([lf, lg]), np.concatenate([lg, lf]), np.concatenate([lp, lp])
    o = np.argsort(src, kind="stable")
    src, dst, par = src[o], dst[o], par[o]
    ptr = np.zeros(nF + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=nF), out=ptr[1:])
    flip = np.full(nF, -1, dtype=np.int64)
    front = fid[label[fid] == fid]
    flip[front] = 0
    while front.size:
        n = ptr[front + 1] - ptr[front]
        e = np.repeat(ptr[front] - np.cumsum(n) + n, n) + np.arange(int(n.sum()))
        nxt, val = dst[e], flip[np.repeat(front, n)] ^ par[e]
        new = flip[nxt] < 0
        flip[nxt[new]] = val[new]                                   # (two frontier faces may reach one face: a clash shows below)
        front = np.unique(nxt[new])
    twisted = np.zeros(nF, dtype=bool)
    twisted[label[lf[(flip[lf] ^ flip[lg]) != lp]]] = True
    flip[~part] = 0
    flip[part & twisted[np.where(part, label, 0)]] = 0
    Fo = F.copy()
    t = flip == 1
    Fo[t, 1], Fo[t, 2] = F[t, 2], F[t, 1]
    counts = np.array([np.count_nonzero(size > 2), np.count_nonzero(twisted), np.count_nonzero(label[fid] == fid)], dtype=np.int32)
    status = (0 if (good | (np.asarray(keep).reshape(-1) == 0)).all() else REPAIR_BAD_FACE) | \
             (REPAIR_NONMANIFOLD if counts[0] else 0) | (REPAIR_NONORIENTABLE if counts[1] else 0)
    return Oriented(flip.astype(np.int32), label.astype(np.int32), Fo.astype(np.int32), counts, int(status))


def repair_mesh(V, F, tol: float = 0.0, weld: bool = True, unique: bool = True, orient: bool = True) -> Repaired:
    """The five steps chained: what operators.repair_mesh computes on the device, field by field (numpy arrays and Python
    ints).  orient=False leaves every winding and reports -1 for nonmanifold_edges, nonorientable_classes and classes."""
    V = np.asarray(V, dtype=np.float32).reshape(-1, 3)
    nV = V.shape[0]
    w = weld_vertices(V, F, tol, weld)
    u = unique_faces(w.F, nV, V, unique)
    if orient:
        o = orient_faces(w.F, u.keep, nV)
        Fo, flip, oc = o.F, o.flip, [int(c) for c in o.counts]
    else:
        Fo, flip, oc = w.F, np.zeros(w.F.shape[0], dtype=np.int32), [-1, -1, -1]
    c = compact(V, Fo, u.keep)
    vertex_index = c.I[w.rep]
    return Repaired(c.Vnew, c.Fnew, c.J, vertex_index, c.Fsrc, flip[c.Fsrc], int(w.counts[0]), int(u.counts[0]), int(u.counts[1]),
                    int(u.counts[2]), oc[0], oc[1], oc[2])


# --------------------------------------------------------------------------------------------------
# mesh descriptors: normals, mass, curvature and the libigl-convention Laplacian (definition: include/sn_spmm.h, "Mesh
# descriptors").  The host statement of what src/utils/geom_utils.py takes from pyigl, in numpy float64 with the operation
# order of the header: elementwise ufuncs only (each rounds on its own), np.add.at for the ordered sums, no np.sum, no np.cross.
# --------------------------------------------------------------------------------------------------
Descriptors = collections.namedtuple("Descriptors", "face_area face_normal n_area n_uniform n_angle mass_bary mass_voronoi gauss "
                                                    "mean status")


def _dot3(u, w):
    return (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]


def _cross3(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def descriptor_sums(V: np.ndarray, F: np.ndarray) -> dict:
    """Everything the header defines per face and per vertex, in float64 BEFORE the rounding to fp32: a dict with
    n (nF, 3), dbl, area, nhat (nF, 3), valid (nF,) bool (neither bad nor flat), good (nF,) bool (not bad), the vertex sums
    N_area, N_uniform, N_angle (nV, 3), M_bary, M_voronoi, theta (the angle sum), dP (nV, 3), degree (valid faces per vertex),
    and the per-corner lists of the valid faces in (face, corner) order: corner_v, corner_a, corner_b, corner_cot_a,
    corner_cot_b."""
    P = np.asarray(V, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV, nF = P.shape[0], F.shape[0]
    good = good_faces(F, nV)
    Fs = np.where(good[:, None], F, 0) if nV else np.zeros_like(F)
    Pc = [P[Fs[:, c]] if nV else np.zeros((nF, 3)) for c in range(3)]
    with np.errstate(all="ignore"):
        n = _cross3(Pc[1] - Pc[0], Pc[2] - Pc[0])
        dbl = np.sqrt(_dot3(n, n))
        valid = good & (dbl > 0)
        area = np.where(valid, dbl / 2, 0.0)
        nhat = np.where(valid[:, None], n / dbl[:, None], 0.0)
        d = np.stack([_dot3(Pc[(c + 1) % 3] - Pc[c], Pc[(c + 2) % 3] - Pc[c]) for c in range(3)], axis=1)
        obtuse = (d[:, 0] < 0) | (d[:, 1] < 0) | (d[:, 2] < 0)
        # per corner, face-major and corner-minor, valid faces only: a vertex meets its faces in ascending order
        fid = np.repeat(np.nonzero(valid)[0], 3)
        cid = np.tile(np.arange(3), int(valid.sum()))
        v, a, b = Fs[fid, cid], Fs[fid, (cid + 1) % 3], Fs[fid, (cid + 2) % 3]
        u, w = P[a] - P[v], P[b] - P[v]
        dv, da, db = d[fid, cid], d[fid, (cid + 1) % 3], d[fid, (cid + 2) % 3]
        dblc, af = dbl[fid], dbl[fid] / 2
        theta = np.arctan2(dblc, dv)
        cota, cotb = da / dblc, db / dblc
        vor = np.where(obtuse[fid], np.where(dv < 0, af / 2, af / 4), (_dot3(u, u) * cotb + _dot3(w, w) * cota) / 8)
        lap = (0.5 * cotb)[:, None] * u + (0.5 * cota)[:, None] * w
        out = {"n": n, "dbl": dbl, "area": area, "nhat": nhat, "valid": valid, "good": good,
               "N_area": np.zeros((nV, 3)), "N_uniform": np.zeros((nV, 3)), "N_angle": np.zeros((nV, 3)), "M_bary": np.zeros(nV),
               "M_voronoi": np.zeros(nV), "theta": np.zeros(nV), "dP": np.zeros((nV, 3)), "degree": np.zeros(nV, dtype=np.int64),
               "corner_v": v, "corner_a": a, "corner_b": b, "corner_cot_a": cota, "corner_cot_b": cotb}
        np.add.at(out["N_area"], v, n[fid])
        np.add.at(out["N_uniform"], v, nhat[fid])
        np.add.at(out["N_angle"], v, theta[:, None] * nhat[fid])
        np.add.at(out["M_bary"], v, af / 3)
        np.add.at(out["M_voronoi"], v, vor)
        np.add.at(out["theta"], v, theta)
        np.add.at(out["dP"], v, lap)
        np.add.at(out["degree"], v, 1)
    return out


def vertex_descriptors(V: np.ndarray, F: np.ndarray) -> Descriptors:
    """Descriptors(face_area, face_normal, n_area, n_uniform, n_angle, mass_bary, mass_voronoi, gauss, mean, status): the fp32
    arrays of sn_mesh_descriptors_f32 and its status word as a Python int (DESC_BAD_FACE | DESC_FLAT_FACE | DESC_NO_NORMAL).
    Replaces geom_utils.compute_normals / area / laplacian_and_mass / gaussian_curvature (all pyigl) in this project's own
    definition: area-, uniform- and angle-weighted unit normals, barycentric and Voronoi (Meyer mixed) mass, the raw angle
    defect K, and the mean curvature H from the cotangent Laplacian of the positions, positive on an outward sphere."""
    s = descriptor_sums(V, F)
    status = 0
    if not s["good"].all():
        status |= DESC_BAD_FACE
    if (s["good"] & ~s["valid"]).any():
        status |= DESC_FLAT_FACE
    normals = []
    with np.errstate(all="ignore"):
        for key in ("N_area", "N_uniform", "N_angle"):
            N = s[key]
            length = np.sqrt(_dot3(N, N))
            ok = length > 0
            if not ok.all():
                status |= DESC_NO_NORMAL
            normals.append(np.where(ok[:, None], N / length[:, None], 0.0).astype(np.float32))
        K = 2 * np.pi - s["theta"]
        dP, Mv = s["dP"], s["M_voronoi"]
        sign = np.where(_dot3(dP, s["N_area"]) > 0, -1.0, 1.0)
        H = np.where(Mv > 0, (sign * np.sqrt(_dot3(dP, dP))) / (2 * Mv), 0.0)
        f32 = lambda x: np.asarray(x).astype(np.float32)
        return Descriptors(f32(s["area"]), f32(s["nhat"]), *normals, f32(s["M_bary"]), f32(Mv), f32(K), f32(H), status)


def libigl_laplacian(V: np.ndarray, F: np.ndarray, mass: str = "barycentric", hack=None):
    """(L, status): L = M^-1 C, igl.cotmatrix scaled by the inverse of igl.massmatrix, as fp32 scipy CSR with columns ascending
    and explicit zeros kept (sn_mesh_cot_laplacian_f32; geom_utils.hacky_compute_laplacian and compute_laplacian).  mass:
    "barycentric" | "voronoi".  hack: None, or the value that replaces every entry whose fp32 value is not finite or exceeds
    1e10 in magnitude (DESC_CLAMPED is then set in status, next to DESC_BAD_FACE / DESC_FLAT_FACE).  A vertex without mass has
    a NaN diagonal when no hack is given.  No degree limit here: the device builder refuses past LAP_MAX_DEGREE."""
    if mass not in ("barycentric", "voronoi"):
        raise ValueError(f'libigl_laplacian: mass must be "barycentric" or "voronoi", got {mass!r}')
    s = descriptor_sums(V, F)
    nV = s["M_bary"].shape[0]
    M = s["M_bary"] if mass == "barycentric" else s["M_voronoi"]
    v, a, b = s["corner_v"], s["corner_a"], s["corner_b"]
    # per valid face and corner: (v, a) gets 0.5 cot_b, (v, b) gets 0.5 cot_a; still face-major, so add.at sums in face order
    rows = np.stack([v, v], axis=1).ravel()
    cols = np.stack([a, b], axis=1).ravel()
    cw = np.stack([0.5 * s["corner_cot_b"], 0.5 * s["corner_cot_a"]], axis=1).ravel()
    keys, inv = np.unique(rows * max(nV, 1) + cols, return_inverse=True)          # ascending (row, col)
    krow, kcol = keys // max(nV, 1), keys % max(nV, 1)
    Cv = np.zeros(keys.size)
    S = np.zeros(nV)
    with np.errstate(all="ignore"):
        np.add.at(Cv, inv.ravel(), cw)
        np.add.at(S, krow, Cv)                                                     # j ascending inside every row
        vals = np.concatenate([Cv / M[krow], (0 - S) / M]).astype(np.float32)
    r = np.concatenate([krow, np.arange(nV)])
    c = np.concatenate([kcol, np.arange(nV)])
    o = np.lexsort((c, r))
    vals, c = vals[o], c[o]
    status = (0 if s["good"].all() else DESC_BAD_FACE) | (DESC_FLAT_FACE if (s["good"] & ~s["valid"]).any() else 0)
    if hack is not None:
        with np.errstate(all="ignore"):
            bad = ~(np.abs(vals) <= np.float32(1e10))
        if bad.any():
            vals[bad] = np.float32(hack)
            status |= DESC_CLAMPED
    rowptr = np.zeros(nV + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=nV), out=rowptr[1:])
    return sp.csr_matrix((vals, c.astype(np.int32), rowptr), shape=(nV, nV)), status


# --------------------------------------------------------------------------------------------------
# principal curvatures: a quadric fitted over the k-ring patch of every vertex (definition: include/sn_spmm.h, "Principal
# curvatures").  The host statement of geom_utils.compute_curv4 (igl.principal_curvature) in this project's own definition:
# numpy float64, every ufunc rounding on its own, the patch sums serial over ascending vertex id.
# --------------------------------------------------------------------------------------------------
CURV_CLIP = 100.0            # compute_curv4 clips the four columns to +-100
_CURV_CHUNK = 4096           # vertices taken together by the host statement (memory only, no effect on any value)
_CURV_PAIRS = [(i, j) for i in range(5) for j in range(i, 5)]


@dataclasses.dataclass
class PrincipalCurvatures:
    """k1 >= k2 (nV,) fp32, d1 / d2 (nV, 3) fp32 unit directions, ring_size (nV,) int32 (the final patch size, CURV_MAX_RING + 1
    where the search overflowed), status: DESC_BAD_FACE and CURV_* bits (an int on the host, a 1-element int32 tensor on the
    device).  A vertex that failed holds NaN."""
    k1: object = None
    k2: object = None
    d1: object = None
    d2: object = None
    ring_size: object = None
    status: object = None


def _padded_rows(indptr, indices, rows, skip=None):
    """(idx, mask): the CSR rows `rows` side by side, padded with 0 / False; skip: rows left empty."""
    cnt = indptr[rows + 1] - indptr[rows]
    if skip is not None:
        cnt = np.where(skip, 0, cnt)
    width = int(cnt.max()) if cnt.size else 0
    j = np.arange(width)[None, :]
    mask = j < cnt[:, None]
    if not indices.size:
        return np.zeros(mask.shape, dtype=np.int64), mask
    pos = np.minimum(indptr[rows][:, None] + j, indices.size - 1)
    return np.where(mask, indices[pos], 0).astype(np.int64), mask


def principal_curvatures(V: np.ndarray, F: np.ndarray, radius: int = 5) -> PrincipalCurvatures:
    """Principal curvatures and directions of every vertex from a quadric fitted over its `radius`-ring patch: the numpy
    statement of sn_mesh_principal_curvature_f32, scalar for scalar (include/sn_spmm.h, "Principal curvatures", has the text).
    Replaces igl.principal_curvature in geom_utils.compute_curv4 with this project's own definition in libigl's conventions."""
    radius = int(radius)
    if radius < 1:
        raise ValueError(f"principal_curvatures: radius must be at least 1, got {radius}")
    P = np.asarray(V, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV = P.shape[0]
    s = descriptor_sums(V, F)
    status = 0 if s["good"].all() else DESC_BAD_FACE
    with np.errstate(all="ignore"):
        Na = s["N_area"]
        length = np.sqrt(_dot3(Na, Na))
        has_normal = length > 0
        n = np.where(has_normal[:, None], Na / length[:, None], 0.0)
    # neighbours through the faces that are not bad; A: the 1-ring with the vertex itself, R: the patch
    Fg = F[s["good"]]
    r = np.concatenate([Fg[:, 0], Fg[:, 1], Fg[:, 2], Fg[:, 0], Fg[:, 1], Fg[:, 2], np.arange(nV)])
    c = np.concatenate([Fg[:, 1], Fg[:, 2], Fg[:, 0], Fg[:, 2], Fg[:, 0], Fg[:, 1], np.arange(nV)])
    A = sp.csr_matrix((np.ones(r.size, dtype=np.int32), (r, c)), shape=(nV, nV))
    A.sum_duplicates()
    A.data[:] = 1
    R = A
    for _ in range(radius - 1):
        R = R @ A
        R.data[:] = 1
    A.sort_indices()
    R.sort_indices()
    k1 = np.full(nV, np.nan, dtype=np.float32)
    k2 = np.full(nV, np.nan, dtype=np.float32)
    d1 = np.full((nV, 3), np.nan, dtype=np.float32)
    d2 = np.full((nV, 3), np.nan, dtype=np.float32)
    ring_size = np.zeros(nV, dtype=np.int32)
    for begin in range(0, nV, _CURV_CHUNK):
        vs = np.arange(begin, min(begin + _CURV_CHUNK, nV))
        out = _curvature_chunk(P, n, has_normal, A, R, vs)
        k1[vs], k2[vs], d1[vs], d2[vs], ring_size[vs] = out[:5]
        status |= out[5]
    return PrincipalCurvatures(k1, k2, d1, d2, ring_size, int(status))


def _curvature_chunk(P, n, has_normal, A, R, vs):
    nb = vs.size
    col = lambda x: x[:, None]
    with np.errstate(all="ignore"):
        count = (R.indptr[vs + 1] - R.indptr[vs]).astype(np.int64)
        fail = np.where(count > CURV_MAX_RING, CURV_OVERFLOW, 0)
        idx, mask = _padded_rows(R.indptr, R.indices, vs, skip=fail != 0)
        W = idx.shape[1]
        Pv, nv = P[vs], n[vs]
        fail = np.where((fail == 0) & ~has_normal[vs], CURV_NO_NORMAL, fail)
        # projection-plane check
        keep = mask & (_dot3(n[idx].reshape(-1, 3), np.repeat(nv, W, axis=0)).reshape(nb, W) > 0)
        kept = keep.sum(axis=1)
        use = (kept >= CURV_MIN_POINTS) & (kept < count) & (fail == 0)
        mask = np.where(col(use), keep, mask)
        count = np.where(use, kept, count)
        ring_size = np.where(fail == CURV_OVERFLOW, CURV_MAX_RING + 1, count).astype(np.int32)
        fail = np.where((fail == 0) & (count < CURV_MIN_POINTS), CURV_FEW_POINTS, fail)
        # fit normal and the patch's extent, serial over ascending ids
        m = np.zeros((nb, 3))
        h2 = np.zeros(nb)
        for j in range(W):
            mj = mask[:, j]
            m = np.where(col(mj), m + n[idx[:, j]], m)
            cj = P[idx[:, j]] - Pv
            cc = _dot3(cj, cj)
            h2 = np.where(mj & (cc > h2), cc, h2)
        lm = np.sqrt(_dot3(m, m))
        fail = np.where((fail == 0) & ~(lm > 0), CURV_DEGENERATE, fail)
        m = m / col(lm)
        # frame: the neighbour of smallest id with a projection of positive length
        nidx, nmask = _padded_rows(A.indptr, A.indices, vs)
        nmask &= nidx != col(vs)
        t = np.zeros((nb, 3))
        lt = np.zeros(nb)
        for j in range(nidx.shape[1]):
            cj = P[nidx[:, j]] - Pv
            tj = cj - col(_dot3(cj, m)) * m
            lj = np.sqrt(_dot3(tj, tj))
            take = nmask[:, j] & ~(lt > 0) & (lj > 0)
            t = np.where(col(take), tj, t)
            lt = np.where(take, lj, lt)
        fail = np.where((fail == 0) & ~(lt > 0), CURV_DEGENERATE, fail)
        e1 = t / col(lt)
        e2 = _cross3(m, e1)
        h = np.sqrt(h2)
        fail = np.where((fail == 0) & ~(h > 0), CURV_DEGENERATE, fail)
        # normal equations of z = a x^2 + b x y + c y^2 + d x + e y in the scaled frame
        G = np.zeros((nb, 5, 5))
        g = np.zeros((nb, 5))
        for j in range(W):
            mj = mask[:, j]
            cj = P[idx[:, j]] - Pv
            xi, eta, zeta = _dot3(cj, e1) / h, _dot3(cj, e2) / h, _dot3(cj, m) / h
            row = [xi * xi, xi * eta, eta * eta, xi, eta]
            for a, b in _CURV_PAIRS:
                G[:, a, b] = np.where(mj, G[:, a, b] + row[a] * row[b], G[:, a, b])
            for a in range(5):
                g[:, a] = np.where(mj, g[:, a] + zeta * row[a], g[:, a])
        for a, b in _CURV_PAIRS:
            G[:, b, a] = G[:, a, b]
        # Cholesky G = L L^T without pivoting, column by column
        L = np.zeros((nb, 5, 5))
        for j in range(5):
            d = G[:, j, j].copy()
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            fail = np.where((fail == 0) & ~(d > CURV_PIVOT_FLOOR * G[:, j, j]), CURV_DEGENERATE, fail)
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 5):
                x = G[:, i, j].copy()
                for k in range(j):
                    x = x - L[:, i, k] * L[:, j, k]
                L[:, i, j] = x / L[:, j, j]
        y = np.zeros((nb, 5))
        for i in range(5):
            x = g[:, i].copy()
            for k in range(i):
                x = x - L[:, i, k] * y[:, k]
            y[:, i] = x / L[:, i, i]
        q = np.zeros((nb, 5))
        for i in range(4, -1, -1):
            x = y[:, i].copy()
            for k in range(i + 1, 5):
                x = x - L[:, k, i] * q[:, k]
            q[:, i] = x / L[:, i, i]
        qa, qb, qc, qd, qe = q[:, 0] / h, q[:, 1] / h, q[:, 2] / h, q[:, 3], q[:, 4]
        # fundamental forms and the symmetric 2 x 2 matrix
        E, Ff, Gg = 1 + qd * qd, qd * qe, 1 + qe * qe
        w = np.sqrt((1 + qd * qd) + qe * qe)
        Lf, Mf, Nf = (2 * qa) / w, qb / w, (2 * qc) / w
        den = E * Gg - Ff * Ff
        s11, s12, s22 = (Lf * Gg - Mf * Ff) / den, (Mf * E - Lf * Ff) / den, (Nf * E - Mf * Ff) / den
        # eigenvalues (negated: k = -lambda) and directions
        tr2 = (s11 + s22) / 2
        df = s11 - s22
        disc = df * df + 4 * (s12 * s12)
        rt = np.sqrt(disc) / 2
        k1 = rt - tr2
        k2 = (0 - tr2) - rt
        dirs = []
        for lam, fallback in ((tr2 - rt, e1), (tr2 + rt, e2)):
            p, q2 = s11 - lam, s22 - lam
            first = np.abs(p) >= np.abs(q2)
            u1 = np.where(first, s12, lam - s22)
            u2 = np.where(first, lam - s11, s12)
            flip = (u1 < 0) | ((u1 == 0) & (u2 < 0))
            u1, u2 = np.where(flip, -u1, u1), np.where(flip, -u2, u2)
            dv = col(u1) * e1 + col(u2) * e2
            ld = np.sqrt(_dot3(dv, dv))
            dirs.append(np.where(col((disc > 0) & (ld > 0)), dv / col(ld), fallback))
        bad = fail != 0
        f32 = lambda x: np.where(bad if x.ndim == 1 else col(bad), np.nan, x).astype(np.float32)
        status = int(np.bitwise_or.reduce(fail)) if nb else 0
        return f32(k1), f32(k2), f32(dirs[0]), f32(dirs[1]), ring_size, status


def curv4_columns(k1, k2):
    """[k1, k2, (k1 + k2) / 2, k1 k2] clipped to +-CURV_CLIP, in the dtype of k1 (every operation rounds on its own)."""
    half = k1.dtype.type(2)
    return np.clip(np.stack([k1, k2, (k1 + k2) / half, k1 * k2], axis=1), -k1.dtype.type(CURV_CLIP), k1.dtype.type(CURV_CLIP))


def curv4(V: np.ndarray, F: np.ndarray, radius: int = 5):
    """geom_utils.compute_curv4 on principal_curvatures: (nV, 4) fp32 [k1, k2, H, K] with H = (k1 + k2) / 2 and K = k1 k2, formed
    in fp32 from the fp32 curvatures, clipped to +-100 and divided column by column by the largest magnitude (an fp32 division).
    None after a warning where a vertex failed (the reference's `return None`)."""
    pc = principal_curvatures(V, F, radius)
    if np.isnan(pc.k1).any() or np.isnan(pc.k2).any():
        warnings.warn(f"curv4: {int(np.isnan(pc.k1).sum())} vertices have no curvature ({curvature_status_names(pc.status)}); "
                      "no columns")
        return None
    C = curv4_columns(pc.k1, pc.k2)
    with np.errstate(all="ignore"):
        return C / np.abs(C).max(axis=0, keepdims=True)


def curvature_status_names(status: int) -> str:
    return " | ".join(constants.status_names("curvature", status)) or "no status bit"


# --------------------------------------------------------------------------------------------------
# synthetic meshes
# --------------------------------------------------------------------------------------------------
def _grid_faces(n: int, m: int, wrap: bool) -> np.ndarray:
    if wrap:
        ii, jj = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
        ni, nj = (ii + 1) % n, (jj + 1) % m
    else:
        ii, jj = np.meshgrid(np.arange(n - 1), np.arange(m - 1), indexing="ij")
        ni, nj = ii + 1, jj + 1
    v00 = (ii * m + jj).ravel()
    v01 = (ii * m + nj).ravel()
    v10 = (ni * m + jj).ravel()
    v11 = (ni * m + nj).ravel()
    F = np.empty((2 * v00.size, 3), dtype=np.int64)
    F[0::2] = np.stack([v00, v01, v11], axis=1)
    F[1::2] = np.stack([v00, v11, v10], axis=1)
    return F


def grid_cloth(n: int, m: int, rng: np.random.Generator, jitter: float = 0.25, permute: bool = False):
    """Open n x m jittered grid with a smooth height field: V = n*m, F = 2(n-1)(m-1). Row-major vertex order
    (or a seeded random permutation of it, to expose gather locality)."""
    ii, jj = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(m, dtype=np.float64), indexing="ij")
    x = ii + jitter * (rng.random((n, m)) - 0.5)
    y = jj + jitter * (rng.random((n, m)) - 0.5)
    ph = rng.random(4) * 2 * np.pi
    z = 0.15 * n * (np.sin(2 * np.pi * ii / n + ph[0]) * np.cos(2 * np.pi * jj / m + ph[1])
                    + 0.5 * np.sin(4 * np.pi * ii / n + ph[2]) * np.sin(2 * np.pi * jj / m + ph[3]))
    V = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) / max(n, m)
    F = _grid_faces(n, m, wrap=False)
    return _maybe_permute(V, F, rng, permute)


def torus_grid(n: int, m: int, rng: np.random.Generator, jitter: float = 0.1, permute: bool = False):
    """Closed n x m torus: V = n*m, F = 2*n*m (every vertex has degree 6)."""
    ii, jj = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(m, dtype=np.float64), indexing="ij")
    u = 2 * np.pi * (ii + jitter * (rng.random((n, m)) - 0.5)) / n
    w = 2 * np.pi * (jj + jitter * (rng.random((n, m)) - 0.5)) / m
    R, r = 1.0, 0.35
    V = np.stack([((R + r * np.cos(w)) * np.cos(u)).ravel(), ((R + r * np.cos(w)) * np.sin(u)).ravel(),
                  (r * np.sin(w)).ravel()], axis=1)
    F = _grid_faces(n, m, wrap=True)
    return _maybe_permute(V, F, rng, permute)


def delaunay_disc(num_vertices: int, rng: np.random.Generator):
    """Mesh-MNIST-like open mesh: seeded random points on the 27x27 image plane, Delaunay-triangulated,
    intensity-like z, then the reference scaling V/27 - (0.5,0.5,0) (src/mesh_mnist/add_laplacian.py:40-41)."""
    from scipy.spatial import Delaunay

    pts = rng.random((num_vertices, 2)) * 27.0
    tri = Delaunay(pts)
    z = 0.5 + 0.5 * np.sin(pts[:, 0] / 4.0) * np.cos(pts[:, 1] / 5.0)
    V = np.concatenate([pts, z[:, None]], axis=1)
    V = V / 27 - np.array([0.5, 0.5, 0.0])
    return V, tri.simplices.astype(np.int64)


def _maybe_permute(V, F, rng, permute):
    """permute=True / "vertices": a seeded random renumbering of the vertices (SURVEY.md §8d's "random-permuted variant"; the
    face list keeps the generator's order); "both": the face list is shuffled as well (what a scanned mesh looks like)."""
    if not permute:
        return V, F
    perm = rng.permutation(V.shape[0])       # new index of old vertex i is inv[i]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    V, F = V[perm], inv[F]
    if permute == "both":
        F = F[rng.permutation(F.shape[0])]
    return V, F


# --------------------------------------------------------------------------------------------------
# locality order: datasets number their vertices arbitrarily (src/utils/mesh.py:35-64 builds every operator in the
# dataset's own order; FAUST scans are loaded as stored, src/dense_correspondence/main.py:66-102)
# --------------------------------------------------------------------------------------------------
def edge_span(F: np.ndarray, rank=None):
    """(mean, max) of |rank_i - rank_j| over the mesh edges: how far apart in memory the dense rows are that one operator row
    touches.  A row-major n x m grid has (2(m+1)/3, m+1); a random numbering about (V/3, V)."""
    F = np.asarray(F)
    r = F if rank is None else np.asarray(rank)[F]
    e = np.abs(np.concatenate([r[:, 0] - r[:, 1], r[:, 1] - r[:, 2], r[:, 2] - r[:, 0]]))
    return (float(e.mean()), int(e.max())) if e.size else (0.0, 0)


def locality_order(F: np.ndarray, num_vertices: int, num_faces_rows=None):
    """(vorder, forder): a numbering of the vertices and faces of a mesh under which every operator of the path is banded.
    vorder[k] = the dataset's index of the vertex stored at position k (reverse Cuthill-McKee on the vertex adjacency: the
    band of a 2-D mesh becomes ~ the width of its breadth-first level sets, <= the row-major band of a grid); forder[k]
    likewise for faces, sorted by the ranks of their corners (smallest first), so that face row ~ 2 x vertex row as in a
    generated grid.  One-time host work per mesh (milliseconds at 20 000 vertices)."""
    from scipy.sparse.csgraph import reverse_cuthill_mckee

    F = np.asarray(F, dtype=np.int64)
    nV = int(num_vertices)
    i = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    j = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    A = sp.coo_matrix((np.ones(i.size, np.int8), (i, j)), shape=(nV, nV)).tocsr()
    A = (A + A.T).tocsr()
    vorder = np.asarray(reverse_cuthill_mckee(A, symmetric_mode=True), dtype=np.int64)
    rank = np.empty(nV, np.int64)
    rank[vorder] = np.arange(nV)
    r = np.sort(rank[F], axis=1)
    forder = np.lexsort((r[:, 2], r[:, 1], r[:, 0])).astype(np.int64)
    return vorder, forder


class MeshOrder:
    """The stored numbering of one mesh: `vorder` / `forder` (stored position -> dataset index) and the inverse `vrank`
    (dataset index -> stored position).  `identity` when the dataset's own numbering was kept."""

    __slots__ = ("vorder", "forder", "vrank", "identity", "span_before", "span_after")

    def __init__(self, vorder, forder, identity=False, span_before=None, span_after=None):
        self.vorder, self.forder = np.asarray(vorder, np.int64), np.asarray(forder, np.int64)
        self.vrank = np.empty_like(self.vorder)
        self.vrank[self.vorder] = np.arange(self.vorder.size)
        self.identity = bool(identity)
        self.span_before, self.span_after = span_before, span_after

    @classmethod
    def of_mesh(cls, F, num_vertices: int, mode="auto", gain: float = 2.0) -> "MeshOrder":
        """mode False / "off": keep the dataset's numbering; True / "rcm": always renumber; "auto" (default): renumber when
        the mean edge span shrinks by more than `gain` x (a generated grid stays as it is, a scan or a permuted grid does
        not)."""
        F = np.asarray(F)
        nV, nF = int(num_vertices), int(F.shape[0])
        if mode in (False, None, "off"):
            return cls(np.arange(nV), np.arange(nF), identity=True)
        vorder, forder = locality_order(F, nV)
        rank = np.empty(nV, np.int64)
        rank[vorder] = np.arange(nV)
        before, after = edge_span(F)[0], edge_span(F, rank)[0]
        if mode == "auto" and before <= gain * after:
            return cls(np.arange(nV), np.arange(nF), identity=True, span_before=before, span_after=before)
        return cls(vorder, forder, span_before=before, span_after=after)

    def mesh(self, V, F):
        """(V, F) in the stored numbering; V may carry leading axes (frames): (..., nV, 3)."""
        if self.identity:
            return V, F
        return np.asarray(V)[..., self.vorder, :], self.vrank[np.asarray(F)[self.forder]]

    def vertex_rows(self, x):
        """Per-vertex data (nV, ...) from the dataset's numbering into the stored one."""
        return x if self.identity else np.asarray(x)[self.vorder]


def permute_operator(A, row_order, col_order, group: int = 1):
    """P_r A P_c^T for a stored operator (the reference's dataset files hold L, Di, DiA per frame): row k of the result is row
    row_order[k] of A, likewise columns; group = 4 for the quaternion operators (blocks of 4 rows / columns move together)."""
    def expand(o):
        o = np.asarray(o, np.int64)
        return o if group == 1 else (group * o[:, None] + np.arange(group)[None, :]).ravel()
    A = A.tocsr()
    out = A[expand(row_order)][:, expand(col_order)].tocsr()
    out.sort_indices()
    return out


def read_ply_ascii(path: str):
    """Minimal ASCII PLY reader (vertex xyz + triangular faces) for meshes/cube.ply-style files."""
    with open(path) as fh:
        lines = [ln.strip() for ln in fh]
    nv = nf = 0
    k = 0
    while lines[k] != "end_header":
        tok = lines[k].split()
        if tok[:2] == ["element", "vertex"]:
            nv = int(tok[2])
        if tok[:2] == ["element", "face"]:
            nf = int(tok[2])
        k += 1
    k += 1
    V = np.array([[float(t) for t in lines[k + i].split()[:3]] for i in range(nv)])
    F = np.array([[int(t) for t in lines[k + nv + i].split()[1:4]] for i in range(nf)], dtype=np.int64)
    return V, F


# ---- Mesh-MNIST from images: lattice Delaunay, Poisson-disc sampling, intensity, quality test ---------------------------------
# Definition: include/sn_spmm.h ("Lattice Delaunay and the Mesh-MNIST maker").  Everything below is Python-int arithmetic — no
# floating-point predicate, no transcendental function — and is NOT the device algorithm: a scan over the whole hull instead of a
# walk, one flip at a time from a stack instead of claim-then-flip rounds.  The device is compared to it bit for bit.
DELAUNAY_COORD_LIMIT = 1 << 24       # |x|, |y| < 2^24
MESHDIGITS_Q = 1 << 16               # lattice units per pixel
POISSON_CANDIDATES, POISSON_RETRIES = 30, 32

Delaunay2D = collections.namedtuple("Delaunay2D", "F nF status flips cocircular boundary")
PoissonDisc = collections.namedtuple("PoissonDisc", "P count steps")
MeshDigitsResult = collections.namedtuple("MeshDigitsResult", "P count V F nF status attempts")

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def lattice_orient(a, b, c) -> int:
    """Twice the signed area of (a, b, c), exact: > 0 counter-clockwise."""
    return (int(b[0]) - int(a[0])) * (int(c[1]) - int(a[1])) - (int(b[1]) - int(a[1])) * (int(c[0]) - int(a[0]))


def lattice_incircle(a, b, c, d) -> int:
    """The in-circle determinant of differences, exact: > 0 iff d lies strictly inside the circle through the counter-clockwise
    a, b, c."""
    adx, ady = int(a[0]) - int(d[0]), int(a[1]) - int(d[1])
    bdx, bdy = int(b[0]) - int(d[0]), int(b[1]) - int(d[1])
    cdx, cdy = int(c[0]) - int(d[0]), int(c[1]) - int(d[1])
    ad, bd, cd = adx * adx + ady * ady, bdx * bdx + bdy * bdy, cdx * cdx + cdy * cdy
    return ad * (bdx * cdy - bdy * cdx) - bd * (adx * cdy - ady * cdx) + cd * (adx * bdy - ady * bdx)


def canonical_faces(F) -> np.ndarray:
    """Each face rotated so that its smallest index comes first, faces sorted lexicographically."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    if F.shape[0] == 0:
        return np.zeros((0, 3), np.int32)
    k = np.argmin(F, axis=1)
    R = np.stack([F[np.arange(F.shape[0]), (k + j) % 3] for j in range(3)], axis=1)
    return R[np.lexsort((R[:, 2], R[:, 1], R[:, 0]))].astype(np.int32)


def snap_to_lattice(P, quantum: float) -> np.ndarray:
    """rint(P / quantum) in float64, as int64 (the caller's range check follows)."""
    return np.rint(np.asarray(P, dtype=np.float64) / float(quantum)).astype(np.int64)


def _delaunay_one(pts, max_flips=None):
    n = len(pts)
    none = np.zeros((0, 3), np.int32)
    if n > DELAUNAY_MAX_POINTS:
        return Delaunay2D(none, 0, DT_TOO_LARGE, 0, 0, 0)
    if any(abs(x) >= DELAUNAY_COORD_LIMIT or abs(y) >= DELAUNAY_COORD_LIMIT for x, y in pts):
        return Delaunay2D(none, 0, DT_RANGE, 0, 0, 0)
    if n < 3:
        return Delaunay2D(none, 0, DT_DEGENERATE, 0, 0, 0)
    order = sorted(range(n), key=lambda i: pts[i])
    p = [pts[i] for i in order]
    if any(p[i] == p[i + 1] for i in range(n - 1)):
        return Delaunay2D(none, 0, DT_DUPLICATE, 0, 0, 0)
    k = next((i for i in range(2, n) if lattice_orient(p[0], p[1], p[i]) != 0), None)
    if k is None:
        return Delaunay2D(none, 0, DT_DEGENERATE, 0, 0, 0)
    # sweep: the first k points are a collinear chain in sort order, p[k] fans it; every later point lies strictly outside the
    # hull so far and gets one triangle per hull edge it sees strictly (an edge it is collinear with is not seen)
    faces = []
    if lattice_orient(p[0], p[1], p[k]) > 0:
        faces += [[i, i + 1, k] for i in range(k - 1)]
        hull = list(range(k)) + [k]
    else:
        faces += [[i + 1, i, k] for i in range(k - 1)]
        hull = list(range(k - 1, -1, -1)) + [k]
    for i in range(k + 1, n):
        h = len(hull)
        vis = [lattice_orient(p[hull[j]], p[hull[(j + 1) % h]], p[i]) < 0 for j in range(h)]
        start = next(j for j in range(h) if vis[j] and not vis[j - 1])
        m = 0
        while vis[(start + m) % h]:
            a, b = hull[(start + m) % h], hull[(start + m + 1) % h]
            faces.append([b, a, i])
            m += 1
        chain = [hull[(start + j) % h] for j in range(m + 1)]
        rest = [hull[(start + m + 1 + j) % h] for j in range(h - m - 1)]
        hull = [chain[0], i, chain[-1]] + rest
    # Lawson flips, one at a time, only where the exact in-circle value is > 0
    edge = {}
    for f, (a, b, c) in enumerate(faces):
        for u, v in ((a, b), (b, c), (c, a)):
            edge.setdefault((min(u, v), max(u, v)), []).append(f)
    stack = [e for e, fs in edge.items() if len(fs) == 2]
    flips = 0
    limit = n * n if max_flips is None else int(max_flips)
    status = 0

    def opposite(f, u, v):
        """face f rotated to (u', v', w) with {u', v'} = {u, v}"""
        a, b, c = faces[f]
        for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
            if {x, y} == {u, v}:
                return x, y, z
        raise AssertionError("edge not in face")

    while stack:
        e = stack.pop()
        fs = edge.get(e)
        if fs is None or len(fs) != 2:
            continue
        f, g = fs
        u, v, w = opposite(f, *e)
        _, _, z = opposite(g, *e)
        if lattice_incircle(p[u], p[v], p[w], p[z]) <= 0:
            continue
        if flips >= limit:
            status = DT_NOT_CONVERGED
            break
        flips += 1
        faces[f], faces[g] = [u, z, w], [z, v, w]
        del edge[e]
        edge[(min(w, z), max(w, z))] = [f, g]
        for (x, y), old, new in (((u, z), g, f), ((v, w), f, g)):
            fl = edge[(min(x, y), max(x, y))]
            fl[fl.index(old)] = new
        stack += [(min(x, y), max(x, y)) for x, y in ((u, z), (z, v), (v, w), (w, u))]
    if status:
        return Delaunay2D(none, 0, status, flips, 0, 0)
    cocircular = 0
    for e, fs in edge.items():
        if len(fs) == 2:
            u, v, w = opposite(fs[0], *e)
            z = opposite(fs[1], *e)[2]
            cocircular += lattice_incircle(p[u], p[v], p[w], p[z]) == 0
    F = canonical_faces([[order[a], order[b], order[c]] for a, b, c in faces])
    return Delaunay2D(F, F.shape[0], 0, flips, int(cocircular), 2 * n - 2 - F.shape[0])


def delaunay_2d(P, count=None, quantum=None, max_flips=None) -> Delaunay2D:
    """The Delaunay triangulation of lattice point sets, host statement of operators.delaunay_2d / sn_delaunay2d_i32.
    P: (n, 2) one set, or (B, Nmax, 2) a padded batch with count (B,) (None: every set has Nmax points).  Integer input is taken as
    lattice coordinates; with quantum the input is snapped, rint(P / quantum).  One set returns Delaunay2D(F (nF, 3) int32 in
    canonical form, nF, status (DT_* bits), flips, cocircular, boundary vertices) as Python ints; a batch returns the same fields
    as arrays, F (B, 2 Nmax, 3) with -1 in the rows past nF.  A refused set has nF = 0.  With cocircular == 0 the result is THE
    Delaunay triangulation; otherwise it is one of them."""
    P = np.asarray(P)
    L = snap_to_lattice(P, quantum) if quantum is not None else P
    if L.ndim == 2:
        return _delaunay_one([(int(x), int(y)) for x, y in L[: (L.shape[0] if count is None else int(count))]], max_flips)
    B, nmax = L.shape[0], L.shape[1]
    count = np.full(B, nmax) if count is None else np.asarray(count).reshape(-1)
    F = np.full((B, 2 * nmax, 3), -1, np.int32)
    out = np.zeros((5, B), np.int32)
    for b in range(B):
        c = int(count[b])
        if c > nmax:
            r = Delaunay2D(None, 0, DT_TOO_LARGE, 0, 0, 0)
        else:
            r = _delaunay_one([(int(x), int(y)) for x, y in L[b, : max(c, 0)]], max_flips)
        F[b, : r.nF] = r.F if r.nF else 0
        out[:, b] = (r.nF, r.status, r.flips, r.cocircular, r.boundary)
    return Delaunay2D(F, out[0], out[1], out[2], out[3], out[4])


def _mix64(z: int) -> int:
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def lattice_draw(seed: int, image: int, attempt: int, step: int, cand: int, retry: int, purpose: int) -> int:
    """The counter-based 64-bit draw: h = seed; for w in (image, attempt, step, cand << 16 | retry << 8 | purpose):
    h = mix64(h + 0x9E3779B97F4A7C15 + w), all modulo 2^64, mix64 the splitmix64 finaliser."""
    h = int(seed) & _M64
    for w in (int(image), int(attempt), int(step), (int(cand) << 16) | (int(retry) << 8) | int(purpose)):
        h = _mix64((h + _GOLDEN + w) & _M64)
    return h


def _below(draw: int, m: int) -> int:
    return ((draw >> 32) * m) >> 32


def poisson_grid(r: float, width: int, height: int):
    """(R, cell, gw, gh) of the sampler's grid: R = round(r Q), cell = isqrt(R^2 / 2), gw x gh cells cover the domain."""
    import math

    R = int(round(float(r) * MESHDIGITS_Q))
    cell = math.isqrt(R * R // 2)
    if R < 4 or width < 1 or height < 1 or max(width, height) * MESHDIGITS_Q >= DELAUNAY_COORD_LIMIT or 4 * R >= (1 << 31):
        raise ValueError(f"poisson_disc: r = {r}, domain {width} x {height} is outside the lattice")
    gw, gh = -(-width * MESHDIGITS_Q // cell), -(-height * MESHDIGITS_Q // cell)
    if gw * gh > DELAUNAY_MAX_POINTS:
        raise ValueError(f"poisson_disc: {gw} x {gh} cells exceed DELAUNAY_MAX_POINTS = {DELAUNAY_MAX_POINTS}")
    return R, cell, gw, gh


def poisson_disc(seed: int, image: int, attempt: int = 0, r: float = 1.5, width: int = 27, height: int = 27) -> PoissonDisc:
    """Bridson's Poisson-disc sampling of the open rectangle (0, width Q) x (0, height Q) in integers (host statement of
    sn_poisson_disc_i32; poisson_disc.py's Grid.poisson restated, not its random stream).  Returns PoissonDisc(P (n, 2) int32 in
    the order the samples were made, n, steps)."""
    R, cell, gw, gh = poisson_grid(r, width, height)
    WQ, HQ, R2 = width * MESHDIGITS_Q, height * MESHDIGITS_Q, R * R
    draw = lambda step, cand, retry, purpose: lattice_draw(seed, image, attempt, step, cand, retry, purpose)
    grid = {}
    pts = [(1 + _below(draw(0, 0, 0, 0), WQ - 1), 1 + _below(draw(0, 0, 0, 1), HQ - 1))]
    grid[(pts[0][0] // cell, pts[0][1] // cell)] = 0
    active = [0]
    steps = 0
    for step in range(1, 2 * gw * gh + 1):
        if not active:
            break
        steps = step
        j = _below(draw(step, 0, 0, 2), len(active))
        ax, ay = pts[active[j]]
        won = None
        for c in range(POISSON_CANDIDATES):
            for t in range(POISSON_RETRIES):
                dx = _below(draw(step, c, t, 3), 4 * R) - 2 * R
                dy = _below(draw(step, c, t, 4), 4 * R) - 2 * R
                if R2 <= dx * dx + dy * dy < 4 * R2:
                    break
            else:
                continue
            x, y = ax + dx, ay + dy
            if not (0 < x < WQ and 0 < y < HQ):
                continue
            gx, gy = x // cell, y // cell
            if all((x - pts[i][0]) ** 2 + (y - pts[i][1]) ** 2 >= R2
                   for i in (grid.get((gx + u, gy + v)) for u in range(-2, 3) for v in range(-2, 3)) if i is not None):
                won = (x, y)
                break
        if won is None:
            active[j] = active[-1]
            active.pop()
        else:
            grid[(won[0] // cell, won[1] // cell)] = len(pts)
            active.append(len(pts))
            pts.append(won)
    return PoissonDisc(np.array(pts, dtype=np.int32).reshape(-1, 2), len(pts), steps)


def lattice_intensity(image: np.ndarray, P) -> np.ndarray:
    """Bilinear intensity of a uint8 image at lattice points (x, y), 16 fraction bits, with the reference's indexing
    (create_data.py:28-36: rows rows-1 - int(y) and rows-1 - int(y + 1), columns int(x) and int(x + 1)), exact in integers, then
    fp32(double(sum) / (255 2^32)).  Points with 0 <= x < (cols - 1) Q and 0 <= y < (rows - 1) Q."""
    image = np.asarray(image)
    top = image.shape[0] - 1
    Q = MESHDIGITS_Q
    out = np.zeros(len(P), np.float32)
    for i, (x, y) in enumerate(np.asarray(P).reshape(-1, 2).tolist()):
        iu, fu, iv, fv = x >> 16, x & (Q - 1), y >> 16, y & (Q - 1)
        f00, f01 = int(image[top - iv, iu]), int(image[top - iv, iu + 1])
        f10, f11 = int(image[top - iv - 1, iu]), int(image[top - iv - 1, iu + 1])
        s = f00 * (Q - fv) * (Q - fu) + f01 * (Q - fv) * fu + f10 * fv * (Q - fu) + f11 * fv * fu
        out[i] = np.float32(np.float64(s) / np.float64(255 * (1 << 32)))
    return out


def mesh_digits(images, seed: int = 0, r: float = 1.5, min_points: int = 101, min_det: int = MESHDIGITS_MIN_DET,
                image_base: int = 0, max_attempts: int = MESHDIGITS_MAX_ATTEMPTS) -> MeshDigitsResult:
    """Images to meshes (host statement of sn_mesh_digits_u8; create_data.py:62-99 restated): per image, attempt 0, 1, ...:
    Poisson-disc points, Delaunay, and the sample is taken when it has at least min_points points and every triangle's
    orientation determinant exceeds min_det (flat area > 1e-2 pixel^2 by default); after max_attempts refusals the image is
    DT_REJECTED.  images: (B, rows, cols) uint8; the domain is (cols - 1) x (rows - 1) pixels.  Returns MeshDigitsResult of
    padded arrays, Nmax = the sampler's cell count: P (B, Nmax, 2) int32, count (B,), V (B, Nmax, 3) fp32 = (x / Q, y / Q,
    intensity), F (B, 2 Nmax, 3) int32 canonical with -1 past nF, nF, status, attempts (the attempt taken; max_attempts when
    rejected).  Rows past count are 0."""
    images = np.asarray(images)
    if images.ndim != 3 or images.dtype != np.uint8:
        raise ValueError("mesh_digits wants images (B, rows, cols) uint8")
    B, rows, cols = images.shape
    _, _, gw, gh = poisson_grid(r, cols - 1, rows - 1)
    nmax = gw * gh
    min_points = max(int(min_points), 3)
    P = np.zeros((B, nmax, 2), np.int32)
    V = np.zeros((B, nmax, 3), np.float32)
    F = np.full((B, 2 * nmax, 3), -1, np.int32)
    count, nF, status, attempts = (np.zeros(B, np.int32) for _ in range(4))
    for b in range(B):
        attempts[b], status[b] = max_attempts, DT_REJECTED
        for attempt in range(max_attempts):
            s = poisson_disc(seed, image_base + b, attempt, r, cols - 1, rows - 1)
            if s.count < min_points:
                continue
            d = delaunay_2d(s.P)
            if d.status:
                continue
            pts = s.P.tolist()
            if min(lattice_orient(pts[i], pts[j], pts[k]) for i, j, k in d.F.tolist()) <= min_det:
                continue
            n = s.count
            P[b, :n], count[b], F[b, : d.nF], nF[b], status[b], attempts[b] = s.P, n, d.F, d.nF, 0, attempt
            V[b, :n, 0] = (s.P[:, 0].astype(np.float64) / MESHDIGITS_Q).astype(np.float32)
            V[b, :n, 1] = (s.P[:, 1].astype(np.float64) / MESHDIGITS_Q).astype(np.float32)
            V[b, :n, 2] = lattice_intensity(images[b], s.P)
            break
    return MeshDigitsResult(P, count, V, F, nF, status, attempts)


# --------------------------------------------------------------------------------------------------
# ARAP deformation (include/sn_spmm.h, "ARAP deformation"): the numpy statement the device equals bit for bit.
# Every sum below is written out in the header's order: slot by slot over the ascending columns of a row, rows strided over
# ARAP_REDUCE_WIDTH partial sums, then the two halving trees.
# --------------------------------------------------------------------------------------------------
ARAP_WAVE = 64

ArapWeights = collections.namedtuple("ArapWeights", "rowptr colind w d status")
ArapSolve = collections.namedtuple("ArapSolve", "x iters status")
ArapResult = collections.namedtuple("ArapResult", "frames frames64 cg_iters energy status R_first rhs_first")


def arap_weights(V0, F) -> ArapWeights:
    """w_ij = W[i, j] of cotangent_weights on the rest mesh over the vertex adjacency, kept whatever its value, columns
    ascending; every entry summed serially over its contributions in (face, permutation) order; d_i = sum_j w_ij in ascending
    column order.  V0 fp32 (nV, 3), widened; F (nF, 3).  A bad face (good_faces) contributes nothing and sets ARAP_BAD_FACE; a
    vertex with more than LAP_MAX_DEGREE incident good faces gets an empty row and sets ARAP_DEGREE."""
    V = np.asarray(V0, dtype=np.float32).astype(np.float64)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nV = V.shape[0]
    good = good_faces(F, nV)
    status = 0 if good.all() else ARAP_BAD_FACE
    fid = np.nonzero(good)[0]
    Fg = F[fid]
    l = edge_lengths(V, Fg)
    den = 8 * heron_areas(l) + 1e-6
    l2 = l * l
    e2 = np.empty((Fg.shape[0], 3, 3))
    e2[:, 0, 1] = e2[:, 1, 0] = l2[:, 0]
    e2[:, 1, 2] = e2[:, 2, 1] = l2[:, 1]
    e2[:, 2, 0] = e2[:, 0, 2] = l2[:, 2]
    rows = np.stack([Fg[:, p] for p, q, r in _PERMS], axis=1).ravel()
    cols = np.stack([Fg[:, q] for p, q, r in _PERMS], axis=1).ravel()
    vals = np.stack([((-e2[:, p, q] + e2[:, q, r]) + e2[:, r, p]) / den for p, q, r in _PERMS], axis=1).ravel()
    incident = np.bincount(Fg.ravel(), minlength=nV)
    if (incident > LAP_MAX_DEGREE).any():
        status |= ARAP_DEGREE
        keep = incident[rows] <= LAP_MAX_DEGREE
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((np.arange(rows.size), cols, rows))          # (row, col, face, permutation): the input is face-major
    rows, cols, vals = rows[order], cols[order], vals[order]
    head = np.ones(rows.size, bool)
    head[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    group = np.cumsum(head) - 1
    starts = np.nonzero(head)[0]
    w = np.zeros(starts.size)
    rank = np.arange(rows.size) - starts[group] if rows.size else np.zeros(0, np.int64)
    for k in range(int(rank.max()) + 1 if rank.size else 0):       # serial: the k-th contribution of every entry
        sel = rank == k
        w[group[sel]] = vals[sel] if k == 0 else w[group[sel]] + vals[sel]
    colind = cols[starts].astype(np.int32)
    rowptr = np.zeros(nV + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(rows[starts], minlength=nV))
    Wt = ArapWeights(rowptr, colind, w, None, status)
    col, wp, valid = _arap_padded(Wt)
    d = np.zeros(nV)
    for k in range(col.shape[1]):
        d = np.where(valid[:, k], d + wp[:, k], d)
    return Wt._replace(d=d)


def _arap_padded(Wt):
    """(col, w, valid), each (nV, D): slot k of row i is its k-th entry; D = the largest row."""
    rowptr = np.asarray(Wt.rowptr, dtype=np.int64)
    deg = np.diff(rowptr)
    D = int(deg.max()) if deg.size else 0
    slot = np.arange(D)[None, :]
    valid = slot < deg[:, None]
    idx = np.where(valid, rowptr[:-1, None] + slot, 0)
    if Wt.colind.size == 0:
        return np.zeros((deg.size, 0), np.int64), np.zeros((deg.size, 0)), np.zeros((deg.size, 0), bool)
    return np.where(valid, np.asarray(Wt.colind, dtype=np.int64)[idx], 0), np.where(valid, Wt.w[idx], 0.0), valid


def _arap_reduce(c: np.ndarray) -> np.ndarray:
    """The header's reduction of c (n,) or (n, k) over its rows: partial sums strided over ARAP_REDUCE_WIDTH lanes, each serial
    in ascending row order from +0.0; a halving tree inside every group of ARAP_WAVE lanes; a halving tree over the groups."""
    c = np.asarray(c, dtype=np.float64)
    c2 = c.reshape(c.shape[0], -1)
    n, k = c2.shape
    rows = -(-n // ARAP_REDUCE_WIDTH)
    pad = np.zeros((rows * ARAP_REDUCE_WIDTH, k))
    pad[:n] = c2
    pad = pad.reshape(rows, ARAP_REDUCE_WIDTH, k)
    part = np.zeros((ARAP_REDUCE_WIDTH, k))
    for r in range(rows):
        part = part + pad[r]
    a = part.reshape(ARAP_REDUCE_WIDTH // ARAP_WAVE, ARAP_WAVE, k).copy()
    s = ARAP_WAVE // 2
    while s:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    g = a[:, 0].copy()
    s = g.shape[0] // 2
    while s:
        g[:s] = g[:s] + g[s:2 * s]
        s //= 2
    return g[0].reshape(c.shape[1:])


def _dot3s(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _matvec3(M, v):
    return np.stack([(M[..., a, 0] * v[..., 0] + M[..., a, 1] * v[..., 1]) + M[..., a, 2] * v[..., 2] for a in range(3)], axis=-1)


def _cross3s(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def arap_covariances(Wt: ArapWeights, P0, P) -> np.ndarray:
    """S_i = sum_j w_ij e_ij e'_ij^T over ascending j, S[a][b] += (w e[a]) e'[b]."""
    col, wp, valid = _arap_padded(Wt)
    S = np.zeros((P0.shape[0], 3, 3))
    for k in range(col.shape[1]):
        j = col[:, k]
        we = wp[:, k, None] * (P0 - P0[j])
        S = np.where(valid[:, k, None, None], S + we[:, :, None] * (P - P[j])[:, None, :], S)
    return S


def arap_rotation_from_covariance(S):
    """(R, degenerate) for S (m, 3, 3): the proper rotation maximising tr(R S), by the header's procedure — cyclic Jacobi
    (ARAP_JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2)) on G = S^T S, eigenvalues sorted descending by the network (0,1), (1,2),
    (0,1), image vectors S v1, S v2 orthonormalised by one Gram-Schmidt step, third vectors by cross products, R = sum_k v_k u_k^T.
    Only + - * / sqrt.  Rank below 2: R = I and degenerate."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, 3, 3)
    m = S.shape[0]
    A = [[None] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            A[a][b] = (S[:, 0, a] * S[:, 0, b] + S[:, 1, a] * S[:, 1, b]) + S[:, 2, a] * S[:, 2, b]
    Vc = [[np.full(m, 1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]      # Vc[r][c]: row r of column c

    def sym(a, b):
        return (a, b) if a < b else (b, a)

    with np.errstate(all="ignore"):
        for _ in range(ARAP_JACOBI_SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq, app, aqq = A[p][q], A[p][p], A[q][q]
                arp, arq = A[sym(r, p)[0]][sym(r, p)[1]], A[sym(r, q)[0]][sym(r, q)[1]]
                nz = apq != 0
                theta = (aqq - app) / np.where(nz, 2 * apq, 1.0)
                t = 1 / (np.abs(theta) + np.sqrt(theta * theta + 1))
                t = np.where(theta < 0, -t, t)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                A[p][p] = np.where(nz, app - t * apq, app)
                A[q][q] = np.where(nz, aqq + t * apq, aqq)
                A[p][q] = np.where(nz, 0.0, apq)
                A[sym(r, p)[0]][sym(r, p)[1]] = np.where(nz, c * arp - s * arq, arp)
                A[sym(r, q)[0]][sym(r, q)[1]] = np.where(nz, s * arp + c * arq, arq)
                for k in range(3):
                    vp, vq = Vc[k][p], Vc[k][q]
                    Vc[k][p] = np.where(nz, c * vp - s * vq, vp)
                    Vc[k][q] = np.where(nz, s * vp + c * vq, vq)
        lam = [A[0][0], A[1][1], A[2][2]]
        for a, b in ((0, 1), (1, 2), (0, 1)):
            sw = lam[a] < lam[b]
            lam[a], lam[b] = np.where(sw, lam[b], lam[a]), np.where(sw, lam[a], lam[b])
            for k in range(3):
                Vc[k][a], Vc[k][b] = np.where(sw, Vc[k][b], Vc[k][a]), np.where(sw, Vc[k][a], Vc[k][b])
        v1 = np.stack([Vc[k][0] for k in range(3)], axis=-1)
        v2 = np.stack([Vc[k][1] for k in range(3)], axis=-1)
        v3 = _cross3s(v1, v2)
        a1, a2 = _matvec3(S, v1), _matvec3(S, v2)
        n1 = _dot3s(a1, a1)
        u1 = a1 / np.sqrt(n1)[:, None]
        a2p = a2 - _dot3s(u1, a2)[:, None] * u1
        n2 = _dot3s(a2p, a2p)
        u2 = a2p / np.sqrt(n2)[:, None]
        u3 = _cross3s(u1, u2)
        R = (v1[:, :, None] * u1[:, None, :] + v2[:, :, None] * u2[:, None, :]) + v3[:, :, None] * u3[:, None, :]
        ok = (n1 > 0) & (n2 > ARAP_RANK_EPS * n1)
    return np.where(ok[:, None, None], R, np.eye(3)[None]), ~ok


def arap_rotations(Wt: ArapWeights, P0, P):
    """The local step: (R (nV, 3, 3), degenerate (nV,) bool)."""
    return arap_rotation_from_covariance(arap_covariances(Wt, np.asarray(P0, np.float64), np.asarray(P, np.float64)))


def arap_rhs(Wt: ArapWeights, P0, R) -> np.ndarray:
    """b_i = sum_j (w_ij / 2) (R_i + R_j) e_ij over ascending j."""
    P0 = np.asarray(P0, np.float64)
    col, wp, valid = _arap_padded(Wt)
    b = np.zeros((P0.shape[0], 3))
    for k in range(col.shape[1]):
        j = col[:, k]
        v = _matvec3(R + R[j], P0 - P0[j])
        b = np.where(valid[:, k, None], b + (wp[:, k] * 0.5)[:, None] * v, b)
    return b


def arap_energy(Wt: ArapWeights, P0, P, R) -> float:
    """sum_i sum_j w_ij |e'_ij - R_i e_ij|^2, rows by the header's reduction."""
    P0, P = np.asarray(P0, np.float64), np.asarray(P, np.float64)
    col, wp, valid = _arap_padded(Wt)
    e = np.zeros(P0.shape[0])
    for k in range(col.shape[1]):
        j = col[:, k]
        df = (P - P[j]) - _matvec3(R, P0 - P0[j])
        e = np.where(valid[:, k], e + wp[:, k] * _dot3s(df, df), e)
    return float(_arap_reduce(e))


def _arap_offdiag(col, wp, valid, free, x):
    """s_i = sum over the FREE columns j of row i, ascending, of w_ij x_j, from +0.0."""
    s = np.zeros_like(x)
    for k in range(col.shape[1]):
        j = col[:, k]
        s = np.where((valid[:, k] & free[j])[:, None], s + wp[:, k, None] * x[j], s)
    return s


def arap_cg(Wt: ArapWeights, fixed, b, x0, tol: float = 1e-10, max_cg: int = 4096) -> ArapSolve:
    """The global step: Jacobi-preconditioned CG on the free rows of sum_j w_ij (x_i - x_j) = b_i, the rows of `fixed` held at
    their values in x0 and moved to the right-hand side; three columns, one matrix product, own alpha and beta, a converged
    column frozen.  Returns (x, iterations, status bits)."""
    fixed = np.asarray(fixed, dtype=bool)
    free = ~fixed
    x = np.array(x0, dtype=np.float64)
    col, wp, valid = _arap_padded(Wt)
    d = Wt.d
    fm = free[:, None]
    rhs = np.array(b, dtype=np.float64)
    for k in range(col.shape[1]):
        j = col[:, k]
        rhs = np.where((valid[:, k] & fixed[j])[:, None], rhs + wp[:, k, None] * x[j], rhs)
    with np.errstate(all="ignore"):
        r = rhs - (d[:, None] * x - _arap_offdiag(col, wp, valid, free, x))
        z = r / d[:, None]
        p = np.where(fm, z, 0.0)
        red = _arap_reduce(np.where(fm, np.concatenate([r * z, r * r, rhs * rhs], axis=1), 0.0))
        rz, rr, bb = red[0:3], red[3:6], red[6:9]
        thr = tol * np.sqrt(bb)
        conv = np.sqrt(rr) <= thr
        status, it = 0, 0
        while it < max_cg and not conv.all():
            Ap = d[:, None] * p - _arap_offdiag(col, wp, valid, free, p)
            pAp = _arap_reduce(np.where(fm, p * Ap, 0.0))
            if (~conv & ~(pAp > 0)).any():
                status |= ARAP_BREAKDOWN
                break
            alpha = rz / pAp
            upd = fm & ~conv[None, :]
            x = np.where(upd, x + alpha[None, :] * p, x)
            r = np.where(upd, r - alpha[None, :] * Ap, r)
            z = r / d[:, None]
            red = _arap_reduce(np.where(fm, np.concatenate([r * z, r * r], axis=1), 0.0))
            it += 1
            conv_new = conv | (np.sqrt(red[3:6]) <= thr)
            beta = red[0:3] / rz
            p = np.where(fm & ~conv_new[None, :], z + beta[None, :] * p, p)
            rz = np.where(conv_new, rz, red[0:3])
            conv = conv_new
        if not conv.all() and not status:
            status |= ARAP_NOT_CONVERGED
    return ArapSolve(x, it, status)


def arap_deform(V0, F, handles, H, iters: int = 2, tol: float = 1e-10, max_cg: int = 4096, weights: ArapWeights = None) -> ArapResult:
    """The whole definition for one mesh.  V0 (nV, 3) fp32, handles (nH,), H (T, nH, 3) fp32.  Returns ArapResult: frames
    (T, nV, 3) fp32, frames64 the same before the rounding, cg_iters (T, iters) int32, energy (T,) fp64 after the last step of
    every frame, status, and the rotations and right-hand side of the first local step of frame 0."""
    V0 = np.asarray(V0, dtype=np.float32)
    P0 = V0.astype(np.float64)
    H = np.asarray(H, dtype=np.float32).astype(np.float64)
    handles = np.asarray(handles, dtype=np.int64)
    Wt = weights if weights is not None else arap_weights(V0, F)
    nV, T = P0.shape[0], H.shape[0]
    fixed = np.zeros(nV, bool)
    fixed[handles] = True
    status = int(Wt.status)
    dbad = bool((~fixed & ~(Wt.d > 0)).any())
    if dbad:
        status |= ARAP_BREAKDOWN
    x = P0.copy()
    R = np.broadcast_to(np.eye(3), (nV, 3, 3)).copy()
    frames64 = np.zeros((T, nV, 3))
    cg_iters = np.zeros((T, iters), np.int32)
    energy = np.zeros(T)
    R_first = rhs_first = None
    for t in range(T):
        x[handles] = H[t]
        start = x.copy()
        for it in range(0 if dbad else iters):
            R, deg = arap_rotations(Wt, P0, x)
            if deg.any():
                status |= ARAP_DEGENERATE
            b = arap_rhs(Wt, P0, R)
            if t == 0 and it == 0:
                R_first, rhs_first = R.copy(), b.copy()
            sol = arap_cg(Wt, fixed, b, x, tol, max_cg)
            cg_iters[t, it] = sol.iters
            status |= sol.status
            x = sol.x
            if sol.status & ARAP_BREAKDOWN:
                x = start.copy()
                break
        energy[t] = arap_energy(Wt, P0, x, R)
        frames64[t] = x
    return ArapResult(frames64.astype(np.float32), frames64, cg_iters, energy, status, R_first, rhs_first)


def arap_handle_motion(V0, frames: int, rng: np.random.Generator):
    """Handles and their positions for a cloth: the vertices of the boundary edge of smallest x are held, those of the edge of
    largest x move rigidly with constant velocity — a rotation about a seeded axis through their centroid plus a translation, so
    that two frames determine the continuation.  Returns (handles (nH,) int32 ascending, H (frames, nH, 3) fp32)."""
    V = np.asarray(V0, dtype=np.float32).astype(np.float64)
    x = V[:, 0]
    ext = V.max(axis=0) - V.min(axis=0)
    h = np.sqrt(max(ext[0] * ext[1], 1e-30) / max(V.shape[0], 1))          # about one grid spacing
    held = np.nonzero(x < x.min() + 0.5 * h)[0]
    moved = np.nonzero(x > x.max() - 0.5 * h)[0]
    moved = np.setdiff1d(moved, held)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    omega = 0.01 + 0.01 * rng.random()                                       # radians per frame
    vel = 0.004 * rng.standard_normal(3)
    c = V[moved].mean(axis=0) if moved.size else np.zeros(3)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    handles = np.concatenate([held, moved])
    order = np.argsort(handles, kind="stable")
    H = np.zeros((frames, handles.size, 3))
    for t in range(frames):
        a = omega * t
        Rm = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        H[t, : held.size] = V[held]
        H[t, held.size:] = c + (V[moved] - c) @ Rm.T + vel * t
    return handles[order].astype(np.int32), H[:, order].astype(np.float32)


# --------------------------------------------------------------------------------------------------
# spectral: the cotangent pencil in fp64, Chebyshev-filtered subspace iteration for its lowest eigenpairs, and the wave kernel
# signature (definition: include/sn_spmm.h, "Spectral").  The host statement of geom_utils.compute_wks without its shift-invert
# eigsh: the same steps and parameters as operators.laplacian_eigenpairs, the three kernels' arithmetic bit for bit (elementwise
# ufuncs, products and sums rounded one by one), the dense steps through numpy's LAPACK where the device uses torch's.
# --------------------------------------------------------------------------------------------------
EIG_MASS_FLOOR = 1e-8                                # compute_wks clips the Voronoi mass here before normalising it

Eigenpairs = collections.namedtuple("Eigenpairs", "values vectors residuals bound outer_iterations mass status")


def eig_guard(k: int) -> int:
    """The default number of guard vectors next to the k wanted ones."""
    return max(16, int(k) // 8)


def cot_pencil(V: np.ndarray, F: np.ndarray):
    """(S, mass, status): the symmetric cotangent stiffness matrix S = -C of libigl_laplacian's C as fp64 scipy CSR (every
    neighbour plus the diagonal, columns ascending, exact zeros kept: S_vj = 0 - C_vj, S_vv = sum_j C_vj over ascending j from
    +0.0), the unrounded fp64 M_voronoi (nV,), and the DESC_BAD_FACE / DESC_FLAT_FACE status word (sn_mesh_cot_pencil_f64).
    C_vj and C_jv sum the same corners in the same order, so S equals its transpose bit for bit."""
    s = descriptor_sums(V, F)
    nV = s["M_voronoi"].shape[0]
    v, a, b = s["corner_v"], s["corner_a"], s["corner_b"]
    rows = np.stack([v, v], axis=1).ravel()
    cols = np.stack([a, b], axis=1).ravel()
    cw = np.stack([0.5 * s["corner_cot_b"], 0.5 * s["corner_cot_a"]], axis=1).ravel()
    keys, inv = np.unique(rows * max(nV, 1) + cols, return_inverse=True)          # ascending (row, col)
    krow, kcol = keys // max(nV, 1), keys % max(nV, 1)
    Cv = np.zeros(keys.size)
    D = np.zeros(nV)
    with np.errstate(all="ignore"):
        np.add.at(Cv, inv.ravel(), cw)                                             # face order inside every entry
        np.add.at(D, krow, Cv)                                                     # j ascending inside every row
        vals = np.concatenate([0 - Cv, D])
    r = np.concatenate([krow, np.arange(nV)])
    c = np.concatenate([kcol, np.arange(nV)])
    o = np.lexsort((c, r))
    status = (0 if s["good"].all() else DESC_BAD_FACE) | (DESC_FLAT_FACE if (s["good"] & ~s["valid"]).any() else 0)
    rowptr = np.zeros(nV + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=nV), out=rowptr[1:])
    return sp.csr_matrix((vals[o], c[o].astype(np.int32), rowptr), shape=(nV, nV)), s["M_voronoi"].copy(), status


def _mix64_array(z: np.ndarray) -> np.ndarray:
    """_mix64 on a uint64 array (the arithmetic wraps modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def spectral_start(seed: int, voff, m: int) -> np.ndarray:
    """The start block (n, m) fp64 of the eigen-solver, a fixed function of (seed, row in its mesh, column)
    (sn_spectral_start_f64): h = mix64(mix64(seed + G + row) + G + column) modulo 2^64, G = 0x9E3779B97F4A7C15, and
    x = (h >> 11) 2^-53 - 0.5.  voff (B + 1,): the first row of every mesh."""
    voff = np.asarray(voff, dtype=np.int64)
    n = int(voff[-1])
    row = np.arange(n, dtype=np.int64) - np.repeat(voff[:-1], np.diff(voff))
    g = np.uint64(_GOLDEN)
    with np.errstate(over="ignore"):
        h = _mix64_array(np.uint64(int(seed) & _M64) + g + row.astype(np.uint64))
        h = _mix64_array(h[:, None] + g + np.arange(m, dtype=np.uint64)[None, :])
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def cheb_filter_step(rowptr, colind, vals, voff, alpha, beta, shift, X, Y) -> np.ndarray:
    """Z[i, c] = (alpha_b ((sum_j A_ij Y[j, c]) - shift_b Y[i, c])) - beta_b X[i, c], b the mesh of row i (sn_cheb_filter_step_f64):
    the row sum runs over the stored entries in ascending position from +0.0, every product and sum rounded on its own."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colind = np.asarray(colind, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    voff = np.asarray(voff, dtype=np.int64)
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = rowptr.size - 1
    cnt = np.diff(rowptr)
    acc = np.zeros((n, Y.shape[1]))
    with np.errstate(all="ignore"):
        for t in range(int(cnt.max()) if n else 0):
            rows = np.nonzero(cnt > t)[0]
            at = rowptr[rows] + t
            acc[rows] = acc[rows] + vals[at][:, None] * Y[colind[at]]
        per_row = lambda x: np.repeat(np.asarray(x, dtype=np.float64), np.diff(voff))[:, None]
        return per_row(alpha) * (acc - per_row(shift) * Y) - per_row(beta) * X


def eig_normalised_mass(mass, voff):
    """(Am, clipped): compute_wks lines 415-416 per mesh — max(mass, 1e-8) divided by its sum (np.sum) over the mesh."""
    mass = np.asarray(mass, dtype=np.float64)
    Am = np.maximum(mass, EIG_MASS_FLOOR)
    clipped = bool((~(mass >= EIG_MASS_FLOOR)).any())
    for b in range(len(voff) - 1):
        Am[voff[b]:voff[b + 1]] /= np.sum(Am[voff[b]:voff[b + 1]])
    return Am, clipped


def cheb_filter_scalars(theta0: float, theta_last: float, bound: float, deg: int):
    """(alpha, beta, shift) of the deg steps of Zhou & Saad's scaled Chebyshev filter on [a, b] = [theta_last, bound], scaled at
    a0 = theta0: e = (b - a) / 2, c = (b + a) / 2, sigma_1 = e / (a0 - c), step 1 has alpha = sigma_1 / e and beta = 0, step
    j + 1 has sigma_{j+1} = 1 / (2 / sigma_1 - sigma_j), alpha = 2 sigma_{j+1} / e, beta = sigma_j sigma_{j+1}; shift = c."""
    e = (bound - theta_last) / 2
    c = (bound + theta_last) / 2
    sigma1 = e / (theta0 - c)
    alpha, beta = [sigma1 / e], [0.0]
    sigma = sigma1
    for _ in range(1, deg):
        nxt = 1 / (2 / sigma1 - sigma)
        alpha.append(2 * nxt / e)
        beta.append(sigma * nxt)
        sigma = nxt
    return np.array(alpha), np.array(beta), np.full(deg, c)


def laplacian_eigenpairs(V, F, k: int = 300, guard: int = None, deg: int = 24, tol: float = 1e-10, max_outer: int = 40,
                         seed: int = 0) -> Eigenpairs:
    """The k lowest eigenpairs S phi = lambda diag(Am) phi of one mesh's cotangent pencil by Chebyshev-filtered subspace
    iteration: the numpy statement of operators.laplacian_eigenpairs (include/sn_spmm.h, "Spectral", has the steps).
    Eigenpairs(values (k,) ascending, vectors (nV, k) with phi^T diag(Am) phi = I, residuals (k,) of the standard form
    A = D S D, D = Am^-1/2, bound = its Gershgorin bound, outer_iterations, mass = Am, status = DESC_* | EIG_* bits); EIG_NOT_CONVERGED comes with a RuntimeWarning, as on the device."""
    S, mass, status = cot_pencil(V, F)
    n = S.shape[0]
    k = int(k)
    if k < 1 or k > n:
        raise ValueError(f"laplacian_eigenpairs: k must lie in 1..{n} (the vertices of the mesh), got {k}")
    voff = np.array([0, n])
    Am, clipped = eig_normalised_mass(mass, voff)
    if clipped:
        status |= EIG_CLIPPED_MASS
    d = 1 / np.sqrt(Am)
    rowptr, colind = S.indptr, S.indices
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    A = (d[rows] * S.data) * d[colind]
    absrow = np.zeros(n)
    np.add.at(absrow, rows, np.abs(A))
    bound = float(absrow.max())
    m = min(n, k + (eig_guard(k) if guard is None else int(guard)))
    one, zero = np.ones(1), np.zeros(1)
    matvec = lambda Y: cheb_filter_step(rowptr, colind, A, voff, one, zero, zero, Y, Y)
    X = np.linalg.qr(spectral_start(seed, voff, m))[0]
    outer = 0
    while True:
        outer += 1
        AX = matvec(X)
        H = X.T @ AX
        theta, Q = np.linalg.eigh((H + H.T) / 2)
        X, AX = X @ Q, AX @ Q
        res = np.sqrt(((AX - X * theta) ** 2).sum(axis=0))
        if (res[:k] <= tol * bound).all():
            break
        if outer == max_outer:
            status |= EIG_NOT_CONVERGED
            warnings.warn(f"laplacian_eigenpairs: the mesh did not reach tol = {tol:g} within max_outer = {max_outer} outer iterations",
                          RuntimeWarning, stacklevel=2)
            break
        alpha, beta, shift = cheb_filter_scalars(theta[0], theta[m - 1], bound, deg)
        T = X
        for j in range(deg):            # two buffers: Z takes the place of the older block
            X, T = cheb_filter_step(rowptr, colind, A, voff, alpha[j:j + 1], beta[j:j + 1], shift[j:j + 1], T, X), X
        X = np.linalg.qr(X)[0]
    return Eigenpairs(theta[:k].copy(), d[:, None] * X[:, :k], res[:k].copy(), bound, outer, Am, status)


def wks_weights(values, N: int = 100):
    """(W (k, N), C (N,)) of compute_wks lines 423-438 for one mesh: E = sorted |values|, logE = log(max(E, 1e-6)),
    ee = linspace(logE[1], max(logE) / 1.02, N), sigma = 6 (ee[1] - ee[0]), W_ki = exp(-(ee_i - logE_k)^2 / (2 sigma^2)),
    C_i = sum_k W_ki."""
    E = np.sort(np.abs(np.asarray(values, dtype=np.float64)))
    if N < 2 or E.size < 2:
        raise ValueError(f"wave_kernel_signature: N >= 2 and k >= 2 are required, got N = {N} and k = {E.size}")
    logE = np.log(np.clip(E, 1e-6, np.inf))
    ee = np.linspace(logE[1], max(logE) / 1.02, N)
    sigma = (ee[1] - ee[0]) * 6
    W = np.exp((-(ee[None, :] - logE[:, None]) ** 2) / (2 * sigma ** 2))
    return W, np.sum(W, axis=0)


def wks_contract(phi, W, C) -> np.ndarray:
    """WKS[v, i] = (sum_k phi_vk^2 W_ki) / C_i, the sum serial over ascending k from +0.0 (sn_wks_f64), fp64."""
    phi, W = np.asarray(phi, dtype=np.float64), np.asarray(W, dtype=np.float64)
    acc = np.zeros((phi.shape[0], W.shape[1]))
    for j in range(W.shape[0]):
        acc = acc + (phi[:, j] * phi[:, j])[:, None] * W[j][None, :]
    return acc / np.asarray(C, dtype=np.float64)[None, :]


def wave_kernel_signature(V, F, N: int = 100, k: int = 300, eigenpairs: Eigenpairs = None, dtype=np.float32) -> np.ndarray:
    """(nV, N) wave kernel signature of one mesh, geom_utils.compute_wks line for line on the eigenpairs of
    laplacian_eigenpairs(V, F, k) (or the ones given): the numpy statement of operators.wave_kernel_signature."""
    ep = eigenpairs if eigenpairs is not None else laplacian_eigenpairs(V, F, k)
    W, C = wks_weights(ep.values, N)
    order = np.argsort(np.abs(ep.values), kind="stable")
    return wks_contract(ep.vectors[:, order], W, C).astype(dtype)


# ---- mesh hierarchy: heavy-edge matching, Galerkin coarse operators, sibling positions ------------------------------------------------
# The numpy statement of the hierarchy `cascade.LapCascade` takes its per-level operators from (the coarsening of Defferrard et
# al. 2017 the reference names and does not contain).  No device twin yet: this is the definition one will have to equal.
MeshHierarchy = collections.namedtuple("MeshHierarchy", "L real order position sizes singletons rounds mate parent positions")


def hierarchy_scores(L: sp.csr_matrix) -> np.ndarray:
    """One fp32 score per stored entry of L (square CSR, fp32, columns ascending): for an off-diagonal entry
    s_ij = fl(|L_ij| / |L_ii|) + fl(|L_ji| / |L_jj|) with L_ji the stored entry or 0, and 0 where either diagonal entry is 0 or
    absent; 0 on the diagonal.  s_ij and s_ji have the same bits (the fp32 add commutes).  For L = M^-1 C this is
    w_ij (1 / d_i + 1 / d_j): the normalised cut of Graclus, whatever the mass convention."""
    n = L.shape[0]
    indptr, col, val = L.indptr.astype(np.int64), L.indices.astype(np.int64), np.abs(L.data.astype(np.float32))
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    d = np.zeros(n, np.float32)
    d[row[row == col]] = val[row == col]
    key = row * n + col                                     # ascending: rows ascending, columns ascending inside a row
    rev = np.searchsorted(key, col * n + row)
    rev_c = np.minimum(rev, max(len(key) - 1, 0))
    back = np.where((rev < len(key)) & (key[rev_c] == col * n + row), val[rev_c], np.float32(0)) if len(key) else val
    ok = (d[row] > 0) & (d[col] > 0) & (row != col)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (val / d[row]).astype(np.float32) + (back / d[col]).astype(np.float32)
    return np.where(ok, s, np.float32(0)).astype(np.float32)


def handshake_matching(L: sp.csr_matrix, max_rounds: int = 1024):
    """(mate, rounds): in a round every unmatched i proposes to the unmatched neighbour j with the largest s_ij > 0, ties to the
    smallest j; mutual proposals become pairs; rounds repeat until one makes no pair.  mate[i] = the partner or -1 (singleton);
    rounds = the rounds that made pairs.  Every round with an eligible edge makes a pair (the smallest endpoint among the
    globally best edges and its choice are mutual); a round past max_rounds that would still make one raises RuntimeError."""
    n = L.shape[0]
    col = L.indices.astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(L.indptr))
    s = hierarchy_scores(L)
    mate = np.full(n, -1, np.int64)
    rounds = 0
    while True:
        live = (mate[row] < 0) & (mate[col] < 0) & (s > 0)
        r, c, v = row[live], col[live], s[live]
        o = np.lexsort((c, -v.astype(np.float64), r))       # per row: largest score first, then smallest column
        r, c = r[o], c[o]
        first = np.ones(len(r), bool)
        first[1:] = r[1:] != r[:-1]
        prop = np.full(n, -1, np.int64)
        prop[r[first]] = c[first]
        i = np.flatnonzero(prop >= 0)
        i = i[(prop[prop[i]] == i) & (i < prop[i])]
        if not len(i):
            return mate, rounds
        if rounds >= max_rounds:
            raise RuntimeError(f"mesh_hierarchy: the matching is not finished after max_rounds = {max_rounds} rounds")
        mate[i], mate[prop[i]] = prop[i], i
        rounds += 1


def _pair_sums(keys, vals):
    """Groups of at most two consecutive equal keys: (index of each group's first entry, fl(first + second) or first)."""
    first = np.ones(len(keys), bool)
    first[1:] = keys[1:] != keys[:-1]
    k = np.flatnonzero(first)
    two = np.zeros(len(keys), bool)
    two[:-1] = first[:-1] & ~first[1:]
    assert not (~first[1:] & ~first[:-1]).any() if len(keys) > 1 else True
    nxt = np.minimum(k + 1, max(len(keys) - 1, 0))
    return k, np.where(two[k], (vals[k] + vals[nxt]).astype(np.float32), vals[k]).astype(np.float32)


def coarsen_operator(L: sp.csr_matrix, mate: np.ndarray, mass: np.ndarray):
    """(L_c, m_c, parent): clusters = pairs and singletons, numbered by the rank of their smallest member; per fine row i,
    t_id = the sequential fp32 sum of L_ij over parent(j) = d in ascending j; L_c[c, d] = fl(fl(r_a t_ad) + fl(r_b t_bd)) for the
    members a < b of c (a missing term skipped), r_a = m_a / (m_a + m_b), r_b = m_b / (m_a + m_b), r = 1 for a singleton, all
    fp32 without contraction; m_c = fl(m_a + m_b); exact zeros dropped.  This is R (L P), the aggregation Galerkin operator
    M_c^-1 P^T M L P."""
    n = L.shape[0]
    idx = np.arange(n, dtype=np.int64)
    rep = np.where((mate >= 0) & (mate < idx), mate, idx)
    is_rep = rep == idx
    parent = (np.cumsum(is_rep) - 1)[rep]
    nc = int(is_rep.sum())
    mass = np.asarray(mass, np.float32)
    pair = mate >= 0
    msum = np.where(pair, mass + mass[np.where(pair, mate, idx)], mass).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(pair, (mass / msum).astype(np.float32), np.float32(1)).astype(np.float32)
    col = L.indices.astype(np.int64)
    row = np.repeat(idx, np.diff(L.indptr))
    val = L.data.astype(np.float32)
    o = np.lexsort((col, parent[col], row))
    k, t = _pair_sums((row * nc + parent[col])[o], val[o])
    ti, td = row[o][k], parent[col][o][k]
    keep = t != 0                                                        # (the product L P drops its exact zeros)
    ti, td, t = ti[keep], td[keep], t[keep]
    o = np.lexsort((ti, td, parent[ti]))
    k, v = _pair_sums((parent[ti] * nc + td)[o], (r[ti] * t).astype(np.float32)[o])
    ci, cd = parent[ti][o][k], td[o][k]
    keep = v != 0
    Lc = sp.csr_matrix((v[keep], (ci[keep], cd[keep])), shape=(nc, nc), dtype=np.float32)
    Lc.sort_indices()
    mc = np.zeros(nc, np.float32)
    mc[parent[is_rep]] = msum[is_rep]
    return Lc, mc, parent


def _to_positions(L: sp.csr_matrix, pos: np.ndarray, size: int) -> sp.csr_matrix:
    M = L.tocoo()
    out = sp.csr_matrix((M.data.astype(np.float32), (pos[M.row], pos[M.col])), shape=(size, size), dtype=np.float32)
    out.sort_indices()
    return out


def mesh_hierarchy(L, levels: int = 4, mass=None, pad_coarsest_to: int = 1, max_rounds: int = 1024, blocks=None) -> MeshHierarchy:
    """Hierarchy of a square fp32 CSR operator with ascending columns, level 0 the coarsest as `Laps` is indexed.

    levels - 1 times: handshake_matching on the scores of the current operator, coarsen_operator with the current masses (mass:
    (n,) fp32 restriction weights of the finest level, None = ones).  Positions: pos_0(c) = c; pos_k(child) = 2 pos_{k-1}(parent)
    + slot, slot 0 for the child with the smaller level-k number; a singleton takes slot 0 and its slot 1 is a fake node (empty
    row and column, fake descendants).  pad_coarsest_to rounds the coarsest count up with fake clusters.  blocks: the row counts
    of the meshes of a block-diagonal batch (None: one mesh); the batch coarsens block by block (no entry crosses meshes, and
    the cluster numbering keeps the meshes apart), every mesh gets the coarsest size of the largest, and positions are per mesh:
    mesh b owns positions b n_0 2^k .. (b + 1) n_0 2^k of level k.

    Returns MeshHierarchy: L[k] the operator of level k in position order, (B n_0 2^k) square; real[k] its real-node mask;
    order: position -> id in the given operator or -1; position: id -> position; sizes[k] real nodes of level k; singletons[k],
    rounds[k] of the matching that coarsened level k (0 at level 0); mate[k], parent[k] of that matching in level-k numbering
    (None at level 0); positions[k]: level-k number -> position (positions[-1] is position).  levels = 1 returns L unchanged with the identity order."""
    L = sp.csr_matrix(L, dtype=np.float32)
    L.sort_indices()
    n = L.shape[0]
    if L.shape[0] != L.shape[1] or levels < 1 or pad_coarsest_to < 1:
        raise ValueError("mesh_hierarchy: a square operator, levels >= 1 and pad_coarsest_to >= 1 are required")
    blocks = [n] if blocks is None else [int(b) for b in blocks]
    if sum(blocks) != n:
        raise ValueError(f"mesh_hierarchy: blocks sum to {sum(blocks)}, the operator has {n} rows")
    m = np.ones(n, np.float32) if mass is None else np.asarray(mass, np.float32).reshape(n)
    ops, mates, parents, rounds = [L], [None], [None], [0]
    block_of = np.repeat(np.arange(len(blocks)), blocks)
    owners = [block_of]
    for _ in range(levels - 1):
        mate, r = handshake_matching(ops[0], max_rounds)
        Lc, m, parent = coarsen_operator(ops[0], mate, m)
        mates[0], parents[0], rounds[0] = mate, parent, r
        own = np.zeros(Lc.shape[0], np.int64)
        own[parent] = owners[0]
        ops.insert(0, Lc); mates.insert(0, None); parents.insert(0, None); rounds.insert(0, 0); owners.insert(0, own)
    B = len(blocks)
    counts0 = np.bincount(owners[0], minlength=B)
    if levels == 1:                                                      # L unchanged, the identity order, whatever the blocks
        B, n0, pos = 1, n, np.arange(n, dtype=np.int64)
    else:
        n0 = int(-(-max(int(counts0.max()), 1) // pad_coarsest_to) * pad_coarsest_to)
        first0 = np.concatenate([[0], np.cumsum(counts0)[:-1]])
        pos = owners[0] * n0 + (np.arange(ops[0].shape[0]) - first0[owners[0]])
    out_L, real, sizes, single, positions = [], [], [], [], []
    for k in range(levels):
        if k > 0:
            mate = mates[k]
            idx = np.arange(len(mate))
            pos = 2 * pos[parents[k]] + ((mate >= 0) & (mate < idx))
        size = B * n0 << k
        positions.append(pos.astype(np.int64))
        out_L.append(_to_positions(ops[k], pos, size))
        mask = np.zeros(size, bool)
        mask[pos] = True
        real.append(mask)
        sizes.append(int(ops[k].shape[0]))
        single.append(int((mates[k] < 0).sum()) if mates[k] is not None else 0)
    order = np.full(len(real[-1]), -1, np.int64)
    order[pos] = np.arange(n)
    return MeshHierarchy(out_L, real, order, positions[-1], sizes, single, rounds, mates, parents, positions)
