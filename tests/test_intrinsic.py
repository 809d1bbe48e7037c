"""Host part of the intrinsic Delaunay Laplacian (mesh_ops.intrinsic_delaunay / intrinsic_laplacian): a hand case, the planar
truth against scipy's Delaunay, the fixed point and its invariants on the named meshes, order independence and the spread
between flip orders that the device bounds are built from, the Laplacian's properties, the refusals, and the new C entry points
in the header, the ctypes table and the launch-plan table.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import intrinsic_cases as ic
from surfacenetworks_amd import mesh_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAUNCHERS = ("sn_mesh_glue_i32", "sn_mesh_idt_rounds_f64", "sn_mesh_idt_laplacian_f32")
QUERIES = ("sn_mesh_glue_workspace_bytes", "sn_mesh_idt_workspace_bytes", "sn_mesh_idt_laplacian_items",
           "sn_mesh_idt_laplacian_workspace_bytes")


def test_hand_case_one_flip():
    """i = (0,0), j = (4,0), k = (2,.5), m = (2,-.5): the long diagonal ij is non-Delaunay, the flip puts in km of length 1."""
    V = np.array([[0, 0, 0], [4, 0, 0], [2, 0.5, 0], [2, -0.5, 0]], np.float64)
    F = np.array([[0, 1, 2], [1, 0, 3]])
    assert mesh_ops.mesh_glue(F, 4).tolist() == [[3, -1, -1], [0, -1, -1]]
    Fp, l, G, flips = mesh_ops._intrinsic_state(V, F)
    assert flips == 1
    assert Fp.tolist() == [[2, 0, 3], [3, 1, 2]]                   # f = (k, i, m), g = (m, j, k)
    assert G.tolist() == [[-1, -1, 5], [-1, -1, 2]]                # sides 2 glued to each other, the outer sides on the boundary
    d = np.sqrt(4.25)
    assert np.allclose(l, [[d, d, 1.0], [d, d, 1.0]], rtol=1e-15, atol=0)
    assert abs(l[0, 2] - 1.0) <= 4e-16 and l[0, 2] == l[1, 2]
    Fq, lq, fq = mesh_ops.intrinsic_delaunay(V, F)
    assert fq == 1 and np.array_equal(Fq, Fp) and np.array_equal(lq, l)
    with pytest.raises(ValueError, match="order"):
        mesh_ops.intrinsic_delaunay(V, F, order="bfs")


def _scramble(P, F, flips, rng):
    """`flips` seeded flips of interior edges whose quad is strictly convex, on a planar simplicial triangulation."""
    F = [tuple(int(v) for v in f) for f in F]

    def orient(a, b, c):
        return (P[b, 0] - P[a, 0]) * (P[c, 1] - P[a, 1]) - (P[b, 1] - P[a, 1]) * (P[c, 0] - P[a, 0])

    done = 0
    while done < flips:
        sides = {}
        for f, (a, b, c) in enumerate(F):
            for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
                sides[(u, v)] = (f, w)
        inner = sorted((u, v) for (u, v) in sides if u < v and (v, u) in sides)
        i, j = inner[int(rng.integers(len(inner)))]
        (f, k), (g, m) = sides[(i, j)], sides[(j, i)]
        # strictly convex: i and j strictly on opposite sides of the line k m (k and m are opposite of i j by construction)
        if not (orient(k, m, i) > 1e-9 and orient(k, m, j) < -1e-9 or orient(k, m, i) < -1e-9 and orient(k, m, j) > 1e-9):
            continue
        F[f], F[g] = (k, i, m), (m, j, k)
        done += 1
    return np.array(F, np.int64)


def test_planar_truth_against_scipy_delaunay():
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(12)
    P = rng.random((80, 2))
    tri = Delaunay(P)
    F0 = tri.simplices.astype(np.int64)
    area = (P[F0[:, 1], 0] - P[F0[:, 0], 0]) * (P[F0[:, 2], 1] - P[F0[:, 0], 1]) - \
           (P[F0[:, 1], 1] - P[F0[:, 0], 1]) * (P[F0[:, 2], 0] - P[F0[:, 0], 0])
    F0[area < 0] = F0[area < 0][:, [0, 2, 1]]                       # one orientation for all
    V = np.concatenate([P, np.zeros((80, 1))], 1)
    Fs = _scramble(P, F0, 200, rng)

    def edge_set(F):
        e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1)
        return set(map(tuple, e))

    assert edge_set(Fs) != edge_set(F0)
    Fp, l, flips = mesh_ops.intrinsic_delaunay(V, Fs)
    print(f"planar truth: {len(edge_set(Fs) - edge_set(F0))} edges scrambled, {flips} flips back")
    assert flips > 0 and edge_set(Fp) == edge_set(F0)
    assert np.allclose(l, mesh_ops.edge_lengths(ic._f32(V), Fp), rtol=1e-12, atol=0)      # the intrinsic lengths are the chords


@pytest.mark.parametrize("name", ic.NAMES)
def test_fixed_point_and_its_invariants(name):
    V, F = ic.meshes()[name]
    Fp, l, G, flips = ic.host_state(name)
    margin, degenerate = mesh_ops.delaunay_margin(l, G)
    print(f"{name}: {F.shape[0]} faces, {flips} flips, smallest cot_f + cot_g = {margin:.3e}")
    assert flips > 0 and degenerate == 0
    assert margin >= mesh_ops.IDT_THRESHOLD                        # no interior side below the threshold
    assert margin > 1e-6                                           # a condition on the inputs: far from cocircular
    inner = G >= 0
    assert np.array_equal(G[G[inner] // 3, G[inner] % 3], np.arange(G.size).reshape(G.shape)[inner])      # an involution
    assert np.array_equal(np.asarray(l)[G[inner] // 3, G[inner] % 3], np.asarray(l)[inner])               # one length per edge
    a0 = np.sqrt(mesh_ops._heron_q(*mesh_ops.edge_lengths(V, F).T)).sum()
    a1 = np.sqrt(mesh_ops._heron_q(*np.asarray(l).T)).sum()
    assert abs(a1 - a0) <= 1e-12 * a0                              # flips conserve the total area
    edges = lambda GG: int((GG < 0).sum() + (GG >= 0).sum() // 2)
    assert edges(G) == edges(mesh_ops.mesh_glue(F, V.shape[0]))    # nV - nE + nF unchanged (nV and nF are)
    assert np.array_equal(np.sort(np.unique(Fp)), np.sort(np.unique(F)))


@pytest.mark.parametrize("name", ic.NAMES)
def test_order_independence_and_spread(name):
    """fifo, lifo and three random seeds: the same edge multiset (vertex pair, multiplicity, self-edges included); the spread
    of the lengths and of the fp64 Laplacian between the orders stays below the constants the device bounds divide by."""
    e0, l0 = ic.sorted_sides(*ic.host_state(name)[:2])
    L0 = ic.host_laplacian(name).toarray()
    rowmax = np.abs(L0).max(axis=1, keepdims=True)
    spread_l = spread_lap = 0.0
    counts = []
    for order, seed in ic.ORDERS:
        Fp, l, _, flips = ic.host_state(name, order, seed)
        counts.append(flips)
        e, ll = ic.sorted_sides(Fp, l)
        assert np.array_equal(e, e0), (name, order, seed)
        spread_l = max(spread_l, float((np.abs(ll - l0) / l0).max()))
        spread_lap = max(spread_lap, float((np.abs(ic.host_laplacian(name, order, seed).toarray() - L0) / rowmax).max()))
    print(f"{name}: flips {counts}, spread of l' {spread_l:.2e}, of L {spread_lap:.2e} of the row maximum")
    assert spread_l < ic.SPREAD_L and spread_lap < ic.SPREAD_LAP


def test_laplacian_equals_the_extrinsic_one_where_nothing_flipped():
    """The flat disc has no flip: the whole matrix.  The disc as generated has two: every row away from them.  Dense, because
    the patterns may differ by explicit zeros."""
    V, F = ic.flat_disc()
    Fp, l, flips = mesh_ops.intrinsic_delaunay(V, F)
    assert flips == 0 and np.array_equal(Fp, F) and np.array_equal(l, mesh_ops.edge_lengths(V, F))
    L, E = mesh_ops.intrinsic_laplacian(V, F).toarray(), mesh_ops.laplacian(V, F).toarray()
    assert (np.abs(L - E) <= 1e-12 * np.abs(E).max(axis=1, keepdims=True)).all()
    V, F = mesh_ops.delaunay_disc(150, np.random.default_rng(5))
    V = ic._f32(V)
    Fp, _, flips = mesh_ops.intrinsic_delaunay(V, F)
    touched = np.unique(np.concatenate([F[(Fp != F).any(axis=1)].ravel(), Fp[(Fp != F).any(axis=1)].ravel()]))
    keep = np.setdiff1d(np.arange(V.shape[0]), touched)
    assert flips == 2 and 0 < touched.size <= 8
    L, E = mesh_ops.intrinsic_laplacian(V, F).toarray(), mesh_ops.laplacian(V, F).toarray()
    assert (np.abs(L - E)[keep] <= 1e-12 * np.abs(E).max(axis=1, keepdims=True)[keep]).all()
    assert np.abs(L - E)[touched].max() > 1e-4 * np.abs(E).max()


@pytest.mark.parametrize("name", ic.NAMES)
def test_laplacian_properties(name):
    V, F = ic.meshes()[name]
    L = ic.host_laplacian(name)
    D = L.toarray()
    assert L.has_sorted_indices and (L.diagonal() != 0).all() and L.shape == (V.shape[0],) * 2
    assert (np.diff(L.indptr) >= 2).all()                          # the diagonal and a neighbour (mesh D has a vertex of degree 1)
    assert (np.abs(D.sum(axis=1)) <= 1e-10 * np.abs(D).max(axis=1)).all()      # rows of D - W sum to zero
    off = D - np.diag(np.diag(D))
    Fp, l, G, _ = ic.host_state(name)
    if (G >= 0).all():                                             # closed: every weight is >= 0, every off-diagonal <= 0
        assert name in ("C", "F_torus") and off.max() <= 0
    ext = mesh_ops.laplacian(V, F).toarray()
    print(f"{name}: off-diagonal entries > 0: extrinsic {(ext - np.diag(np.diag(ext)) > 0).sum()}, intrinsic {(off > 0).sum()}")
    # only boundary edges keep a negative cotangent: an off-diagonal entry > 0 joins two boundary vertices
    bnd = np.zeros(V.shape[0], bool)
    bnd[np.asarray(Fp)[np.asarray(G) < 0]] = True
    i, j = np.nonzero(off > 0)
    assert bnd[i].all() and bnd[j].all()


def test_refusals():
    with pytest.raises(ValueError, match="more than two faces"):
        mesh_ops.intrinsic_delaunay(np.zeros((5, 3)), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]]))
    with pytest.raises(ValueError, match="same direction"):
        mesh_ops.intrinsic_delaunay(np.zeros((4, 3)), np.array([[0, 1, 2], [0, 1, 3]]))
    with pytest.raises(ValueError, match="outside"):
        mesh_ops.intrinsic_delaunay(np.zeros((4, 3)), np.array([[0, 1, 2], [1, 0, 4]]))
    with pytest.raises(ValueError, match="outside"):
        mesh_ops.intrinsic_laplacian(np.zeros((4, 3)), np.array([[0, 1, 2], [1, 0, -1]]))
    with pytest.raises(ValueError, match="repeated"):
        mesh_ops.intrinsic_delaunay(np.zeros((4, 3)), np.array([[0, 1, 2], [1, 0, 0]]))


def test_header_ctypes_and_plan_table_agree_on_the_new_symbols():
    from surfacenetworks_amd import _lib, kernels

    text = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    ctype = {"size_t": C.c_size_t, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}
    lib = _lib.load()
    for name in LAUNCHERS + QUERIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in the header"
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)], name
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in m.group(2).split(",")]
        assert list(args) == want, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
        if name in LAUNCHERS:
            assert f"SN_PLAN_FN({name})\n" in table and lib.sn_plan_lookup(name.encode()) >= 0
        else:
            assert name not in table
    bits = {k: int(re.search(r"#define\s+SN_IDT_" + k + r"\s+(\d+)", src).group(1))
            for k in ("BAD_FACE", "NOT_CONVERGED", "DEGENERATE", "NON_MANIFOLD", "ORIENTATION")}
    assert bits == {"BAD_FACE": kernels.IDT_BAD_FACE, "NOT_CONVERGED": kernels.IDT_NOT_CONVERGED, "DEGENERATE": kernels.IDT_DEGENERATE,
                    "NON_MANIFOLD": kernels.IDT_NON_MANIFOLD, "ORIENTATION": kernels.IDT_ORIENTATION}
    assert bits["NOT_CONVERGED"] == 2 and bits["DEGENERATE"] == 4
    assert float(re.search(r"#define\s+SN_IDT_THRESHOLD\s+\((-?[0-9.e-]+)\)", src).group(1)) == mesh_ops.IDT_THRESHOLD == -1e-12
    assert "NOT a reproduction" in text and "scaling and sign" in text.lower()
    assert lib.sn_mesh_idt_laplacian_items(6890, 13776) == 12 * 13776 + 6890 and lib.sn_mesh_idt_workspace_bytes(-1) == 0


def test_argument_checks_return_status_codes_without_a_device():
    """Every refusal of an argument happens before any launch (the pointers are never followed)."""
    from surfacenetworks_amd import _lib

    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    wg = lib.sn_mesh_glue_workspace_bytes(4, 2)
    assert lib.sn_mesh_glue_i32(p, p, -1, 2, p, p, p, p, wg, None) == -2                        # SN_E_SHAPE
    assert lib.sn_mesh_glue_i32(p, p, 4, 2 ** 30, p, p, p, p, wg, None) == -3                   # SN_E_RANGE
    assert lib.sn_mesh_glue_i32(p, p, 4, 2, p, p, None, p, wg, None) == -1                      # SN_E_NULL: no status word
    assert lib.sn_mesh_glue_i32(p, None, 4, 2, p, p, p, p, wg, None) == -1
    assert lib.sn_mesh_glue_i32(p, p, 4, 2, p, None, p, p, wg, None) == -1                      # V without l
    assert lib.sn_mesh_glue_i32(p, p, 4, 2, p, p, p, p, wg - 1, None) == -6                     # SN_E_WORKSPACE
    wr = lib.sn_mesh_idt_workspace_bytes(2)
    assert wr >= 16
    assert lib.sn_mesh_idt_rounds_f64(p, p, p, 2, 0, 9, 8, p, p, p, wr, None) == -2             # rounds past max_rounds
    assert lib.sn_mesh_idt_rounds_f64(p, p, p, 2, -1, 1, 8, p, p, p, wr, None) == -2
    assert lib.sn_mesh_idt_rounds_f64(p, p, p, 2, 0, 1, 8, None, p, p, wr, None) == -1
    assert lib.sn_mesh_idt_rounds_f64(p, p, p, 2, 0, 1, 8, p, None, p, wr, None) == -1
    assert lib.sn_mesh_idt_rounds_f64(None, p, p, 2, 0, 1, 8, p, p, p, wr, None) == -1
    assert lib.sn_mesh_idt_rounds_f64(p, p, p, 2, 0, 1, 8, p, p, p, wr - 1, None) == -6
    assert lib.sn_mesh_idt_rounds_f64(p, p, p, 2, 3, 0, 8, p, p, p, wr, None) == 0              # nothing to do
    wl = lib.sn_mesh_idt_laplacian_workspace_bytes(4, 2)
    assert lib.sn_mesh_idt_laplacian_f32(p, p, 4, 2, 3, p, p, p, p, p, None, p, wl, None) == -2
    assert lib.sn_mesh_idt_laplacian_f32(p, p, 4, 2, 0, None, None, None, None, None, None, p, wl, None) == -1
    assert lib.sn_mesh_idt_laplacian_f32(p, p, 4, 2, 1, p, None, p, None, None, None, p, wl, None) == -1
    assert lib.sn_mesh_idt_laplacian_f32(p, p, 4, 2, 0, p, None, None, None, None, None, p, wl - 1, None) == -6
    assert lib.sn_mesh_idt_laplacian_f32(p, p, 2 ** 30, 2 ** 20, 0, p, None, None, None, None, None, p, 2 ** 40, None) == -3


def test_cpu_tensors_and_unknown_keywords_are_rejected():
    import torch

    from surfacenetworks_amd import datasets, kernels, operators
    from surfacenetworks_amd import dense_correspondence as dc

    V, F = ic.meshes()["A"]
    Vt, Ft = torch.from_numpy(V.astype(np.float32)), torch.from_numpy(F.astype(np.int32))
    for call in (lambda: kernels.mesh_glue(Ft, Vt.shape[0]), lambda: kernels.intrinsic_delaunay(Vt, Ft),
                 lambda: kernels.intrinsic_laplacian_from_mesh(Vt, Ft), lambda: operators.laplacian_operator_from_mesh(Vt, Ft, intrinsic=True)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
    with pytest.raises(ValueError, match="laplacian"):
        datasets.faust_frame_from_mesh(V, F, device="cpu", laplacian="seism")
    with pytest.raises(ValueError, match="laplacian"):
        dc.TorusBodies(1, n=9, m=14, pad_to=128, device="cpu", laplacian="seism")
