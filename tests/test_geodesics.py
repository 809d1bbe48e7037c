"""Host part of the geodesic distance matrices: the definition the device kernel relies on (the fixed point of the relaxation
does not depend on the order and is what an fp32 Dijkstra returns), the oracle against scipy's float64 Dijkstra, the new C
entry points in the header, the ctypes table and the launch-plan table, and the refusal of CPU tensors.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import geodesic_oracle as go
from surfacenetworks_amd import mesh_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAUNCHERS = ("sn_edge_lengths_csr_f32", "sn_graph_apsp_f32", "sn_graph_apsp_sweeps_f32", "sn_symmetrize_min_f32")
QUERIES = ("sn_graph_apsp_max_vertices", "sn_graph_apsp_group", "sn_graph_apsp_threads")


def meshes():
    """The three meshes of the geodesic tests: 150, 126 and 108 vertices — no multiple of 8 or of a wave."""
    rng = np.random.default_rng(7)
    return {"disc": mesh_ops.delaunay_disc(150, rng), "torus": mesh_ops.torus_grid(9, 14, rng),
            "cloth": mesh_ops.grid_cloth(12, 9, rng, permute=True)}


@pytest.fixture(scope="module")
def graphs():
    return {k: go.mesh_graph(V, F) for k, (V, F) in meshes().items()}


@pytest.fixture(scope="module")
def oracle_D(graphs):
    return {k: go.apsp_f32(*g) for k, g in graphs.items()}


@pytest.mark.parametrize("name", ["disc", "torus", "cloth"])
def test_sweeps_reach_the_dijkstra_values_in_any_vertex_order(name, graphs, oracle_D):
    """Ascending, descending and random sweeps to the fixed point == fp32 heap Dijkstra, bit for bit: the value is a property
    of the graph, not of the relaxation order — which is what lets the device kernel race its lanes."""
    rowptr, colind, w = graphs[name]
    n = len(rowptr) - 1
    rng = np.random.default_rng(1)
    for s in (0, n // 3, n - 1):
        for order in (range(n), range(n - 1, -1, -1), rng.permutation(n).tolist()):
            d, sweeps = go.sweep_fixed_point(rowptr, colind, w, s, order)
            assert np.array_equal(d, oracle_D[name][s]), (name, s)
            assert sweeps <= n


def test_direction_of_a_stored_entry():
    """Row v lists the edges into v: with one-way weights the sweep and the Dijkstra still agree, and D[s][v] walks s -> v."""
    rowptr, colind, w = np.array([0, 1, 2, 3], np.int32), np.array([2, 0, 1], np.int32), np.array([4, 1, 2], np.float32)
    D = go.apsp_f32(rowptr, colind, w)                       # the cycle 0 -> 1 -> 2 -> 0 with lengths 1, 2, 4
    assert D.tolist() == [[0, 1, 3], [6, 0, 2], [4, 5, 0]]
    for s in range(3):
        for order in ((0, 1, 2), (2, 1, 0)):
            assert np.array_equal(go.sweep_fixed_point(rowptr, colind, w, s, order)[0], D[s])


@pytest.mark.parametrize("name", ["disc", "torus", "cloth"])
def test_oracle_against_scipy_float64_dijkstra(name, graphs, oracle_D):
    """Same fp32 weights, float64 path sums.  A path has at most n - 1 edges, each fp32 addition rounds by at most 2^-24 of a
    partial sum that never exceeds the result, and a factor 2 covers the second-order terms: |D32 - D64| <= n 2^-23 D64."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra

    rowptr, colind, w = graphs[name]
    n = len(rowptr) - 1
    rows = go.csr_rows(rowptr)
    off = rows != colind                                    # (csgraph reads explicit zeros as "no edge": drop the self-loops)
    A = sp.csr_matrix((w[off].astype(np.float64), (colind[off], rows[off])), shape=(n, n))     # entry (v, u): the edge u -> v
    D64 = dijkstra(A, directed=True)
    D32 = oracle_D[name].astype(np.float64)
    assert np.isfinite(D64).all() and np.isfinite(D32).all()
    err = np.abs(D32 - D64)
    print(f"geodesic oracle vs float64 {name}: max {err.max() / D64.max():.2e} of the largest distance")
    assert (err <= n * 2.0 ** -23 * D64).all()
    assert not np.array_equal(oracle_D[name], oracle_D[name].T)       # D is not symmetric: the package defines min(D, D^T)


def test_edge_weight_formula_is_the_laplacian_builders_distance():
    """The oracle's weights are mesh_ops.edge_lengths' (the reference's mesh.dist) on fp32 coordinates, rounded to fp32."""
    V, F = meshes()["cloth"]
    V32 = V.astype(np.float32)
    l = mesh_ops.edge_lengths(V32.astype(np.float64), F)
    for c, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
        assert np.array_equal(go.edge_weights(V32, F[:, a], F[:, b]), l[:, c].astype(np.float32))


def test_header_ctypes_and_plan_table_agree_on_the_new_symbols():
    from surfacenetworks_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sn_spmm.h")).read(), flags=re.S)
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    ctype = {"size_t": C.c_size_t, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}
    lib = _lib.load()
    for name in LAUNCHERS + QUERIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in the header"
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)], name
        decl = [] if m.group(2).strip() == "void" else m.group(2).split(",")
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in decl]
        assert list(args) == want, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
        if name in LAUNCHERS:
            assert f"SN_PLAN_FN({name})\n" in table and lib.sn_plan_lookup(name.encode()) >= 0
        else:
            assert name not in table
    # the documented dispatch rule: S = the largest of 8, 4, 2, 1 with S * n <= max; 0 (unsupported) above max
    nmax = lib.sn_graph_apsp_max_vertices()
    assert nmax * 4 + 16 == 160 * 1024
    for n in (1, 150, nmax // 8, nmax // 8 + 1, nmax // 4, nmax // 4 + 1, nmax // 2, nmax // 2 + 1, nmax, nmax + 1):
        want = next((S for S in (8, 4, 2, 1) if S * n <= nmax), 0)
        assert lib.sn_graph_apsp_group(n) == want, n
        per_cu = 160 * 1024 // (16 + 4 * want * n) if want else 0
        assert lib.sn_graph_apsp_threads(n) == (0 if not want else 1024 if per_cu <= 1 else 512 if per_cu == 2 else 256), n


def test_argument_checks_return_status_codes_without_a_device():
    """Every refusal happens before any launch, so it can be seen on a box without a GPU (the pointers are never followed)."""
    from surfacenetworks_amd import _lib

    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    nmax = lib.sn_graph_apsp_max_vertices()
    assert lib.sn_graph_apsp_f32(p, p, p, nmax + 1, 0, 1, p, nmax + 1, None, None) == -7       # SN_E_UNSUPPORTED
    assert lib.sn_graph_apsp_f32(p, p, p, -1, 0, 0, p, 4, None, None) == -2                     # SN_E_SHAPE
    assert lib.sn_graph_apsp_f32(p, p, p, 4, 0, -1, p, 4, None, None) == -2
    assert lib.sn_graph_apsp_f32(p, p, p, 4, 2, 3, p, 4, None, None) == -2                      # sources past the last vertex
    assert lib.sn_graph_apsp_f32(None, p, p, 4, 0, 4, p, 4, None, None) == -1                   # SN_E_NULL
    assert lib.sn_graph_apsp_f32(p, p, p, 4, 0, 4, None, 4, None, None) == -1
    assert lib.sn_graph_apsp_f32(p, None, p, 4, 0, 4, p, 4, None, None) == -1
    assert lib.sn_graph_apsp_f32(p, p, p, 4, 0, 4, p, 3, None, None) == -4                      # SN_E_LD
    assert lib.sn_graph_apsp_f32(p, p, p, 4, 0, 0, p, 4, None, None) == 0                       # nothing to do
    assert lib.sn_edge_lengths_csr_f32(None, p, p, 4, p, None) == -1
    assert lib.sn_edge_lengths_csr_f32(p, p, p, -1, p, None) == -2
    assert lib.sn_edge_lengths_csr_f32(p, p, p, 0, p, None) == 0
    assert lib.sn_symmetrize_min_f32(None, 4, 4, None) == -1
    assert lib.sn_symmetrize_min_f32(p, -1, 4, None) == -2
    assert lib.sn_symmetrize_min_f32(p, 4, 3, None) == -4
    assert lib.sn_symmetrize_min_f32(p, 0, 0, None) == 0


def test_cpu_tensors_are_rejected_not_computed():
    from surfacenetworks_amd import datasets, kernels, operators
    from surfacenetworks_amd import dense_correspondence as dc

    V, F = meshes()["torus"]
    rowptr, colind, w = (torch.from_numpy(x) for x in go.mesh_graph(V, F))
    Vt, Ft = torch.from_numpy(V.astype(np.float32)), torch.from_numpy(F)
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.edge_lengths_csr(Vt, rowptr, colind)
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.graph_apsp(rowptr, colind, w, Vt.shape[0])
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.symmetrize_min_(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="no CPU"):
        operators.geodesic_matrix_from_mesh(Vt, Ft)
    with pytest.raises(RuntimeError, match="no CPU"):
        datasets.faust_frame_from_mesh(V, F, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU"):
        dc.TorusBodies(1, n=9, m=14, pad_to=128, device="cpu", geodesics="graph")
    with pytest.raises(ValueError, match="geodesics"):
        dc.TorusBodies(1, n=9, m=14, pad_to=128, device="cpu", geodesics="exact")
