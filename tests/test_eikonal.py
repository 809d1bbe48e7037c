"""Host part of the geodesic matrices that cross triangles (method="triangles"): the closed form of the corner update against
brute force, the numpy oracle against the edge-path oracle and against the chord on flat meshes, two hand cases, the new C
entry points in the header, the ctypes table and the launch-plan table, and the refusals.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eikonal_oracle as eo
import geodesic_oracle as go
from test_geodesics import meshes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAUNCHERS = ("sn_mesh_corners_f32", "sn_mesh_geodesics_f32", "sn_mesh_geodesics_sweeps_f32")
QUERIES = ("sn_mesh_corners_workspace_bytes",)


def test_closed_form_against_the_objective_and_a_grid():
    """4000 random planar triangles — a quarter thin (height 1e-6..1e-2 of the base), obtuse ones included — with random fp32
    d_a, d_b.  Everything in float64 storage with exact edge lengths, so that the endpoints of the objective are the edge
    candidates themselves."""
    rng = np.random.default_rng(0)
    k = 4000
    P = np.zeros((3, k, 3))
    P[:, :, :2] = rng.uniform(-1, 1, (3, k, 2))
    thin = np.arange(k) < k // 4                                   # v close to the line through a and b, inside or outside ab
    lam = rng.uniform(-1.5, 2.5, k)
    e = P[1] - P[2]
    normal = np.stack([-e[:, 1], e[:, 0], np.zeros(k)], 1)
    P[0][thin] = (P[2] + lam[:, None] * e + 10.0 ** rng.uniform(-6, -2, k)[:, None] * normal)[thin]
    Pv, Pa, Pb = P
    c, sb, h = eo.corner_constants(Pv, Pa, Pb)
    assert (c > 0).all() and (h > 0).all()
    la, lb = np.linalg.norm(Pa - Pv, axis=1), np.linalg.norm(Pb - Pv, axis=1)
    obtuse = (sb > 0) | (sb + c < 0)                               # v's foot outside the edge: the angle at a or b is obtuse
    assert obtuse.sum() > k // 10 and (h < 1e-3 * c).sum() > k // 10
    db = rng.uniform(0, 2, k).astype(np.float32).astype(np.float64)
    da = (db + rng.uniform(-1.2, 1.2, k) * c).astype(np.float32).astype(np.float64)      # |delta| >= c in a sixth of the cases
    delta = da - db

    def objective(lmb):
        return db + lmb * delta + np.linalg.norm(Pb + lmb[..., None] * (Pa - Pb) - Pv, axis=-1)

    taken, t = eo.triangle_candidate(da, db, c, sb, h)
    assert 0.2 * k < taken.sum() < 0.8 * k
    r = np.sqrt(((c - delta) * (c + delta))[taken])
    lam_star = (-(h * delta)[taken] / r - sb[taken]) / c[taken]
    at_star = db[taken] + lam_star * delta[taken] + np.linalg.norm(Pb[taken] + lam_star[:, None] * (Pa - Pb)[taken] - Pv[taken], axis=1)
    print(f"closed form vs objective at its own lambda: max {np.abs(t[taken] - at_star).max():.2e}")
    assert (np.abs(t[taken] - at_star) <= 1e-12).all()
    cand = eo.corner_candidate(da, db, la, lb, c, sb, h, store=np.float64)
    grid = np.stack([objective(np.full(k, x)) for x in np.linspace(0.0, 1.0, 2001)])
    print(f"candidate minus the grid minimum: max {(cand - grid.min(0)).max():.2e}")
    assert (cand[None] <= grid + 1e-12).all()
    assert np.array_equal(cand[~taken], np.minimum(da + la, db + lb)[~taken])


@pytest.fixture(scope="module")
def oracle_D():
    out = {k: eo.mesh_apsp(V, F) for k, (V, F) in meshes().items()}
    for D in out.values():
        D.setflags(write=False)
    return out


@pytest.mark.parametrize("name", ["disc", "torus", "cloth"])
def test_oracle_lies_below_the_edge_oracle(name, oracle_D):
    """The edge candidates are the edge relaxation's own fp32 sums and fp32 addition is monotone: D_triangles <= D_edges
    exactly, and a path across a face is strictly shorter for most pairs."""
    V, F = meshes()[name]
    E = go.mesh_apsp(V, F)
    D = oracle_D[name]
    assert np.isfinite(D).all() and (D <= E).all()
    print(f"{name}: {100 * (D < E).mean():.1f} % of the entries strictly below the edge path")
    assert (D < E).any()
    assert (D.diagonal() == 0).all()


@pytest.mark.parametrize("name,factor", [("grid", 0.5), ("disc", 0.75)])
def test_oracle_against_the_chord_on_flat_meshes(name, factor):
    """Flat and convex: the true geodesic is the chord.  No value undercuts it by more than the fp32 roundings of a chain of
    at most n updates (n 2^-23, as for the edge paths), and the mean relative error of min(D, D^T) is at most `factor` times
    the edge path's."""
    V, F = eo.flat_fixtures()[name]
    n = V.shape[0]
    Cd = eo.chord(V)
    D = eo.mesh_apsp(V, F)
    assert (D >= Cd * (1 - n * 2.0 ** -23)).all()
    err = eo.mean_rel_error(np.minimum(D, D.T), Cd)
    err_edges = eo.mean_rel_error(go.mesh_apsp(V, F, symmetric=True), Cd)
    print(f"flat {name}: mean relative error across triangles {err:.4f}, along edges {err_edges:.4f}")
    assert err <= factor * err_edges


def test_hand_cases():
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    D = eo.mesh_apsp(sq, np.array([[0, 1, 3], [1, 2, 3]]))         # the unit square with the 1-3 diagonal
    assert D[0][2] == np.float32(1 + np.sqrt(0.5)) and D[0].tolist() == [0, 1, float(np.float32(1 + np.sqrt(0.5))), 1]
    D64 = eo.mesh_apsp(sq, np.array([[0, 1, 3], [1, 2, 3]]), store=np.float64)
    assert D64.dtype == np.float64 and abs(D64[0][2] - (1 + np.sqrt(0.5))) < 1e-15
    tri = np.array([[0, 0, 0], [3, 4, 0], [6, 0, 0]], np.float64)  # one triangle, sides 5, 5, 6: nothing to cross
    assert eo.mesh_apsp(tri, np.array([[0, 1, 2]])).tolist() == [[0, 5, 6], [5, 0, 5], [6, 5, 0]]
    assert np.array_equal(eo.mesh_apsp(tri, np.array([[0, 1, 2]]), sources=[2, 0]), np.array([[6, 5, 0], [0, 5, 6]], np.float32))
    cptr, v, rec, dropped = eo.corner_table(tri, np.array([[0, 1, 2], [0, 0, 1], [0, 1, 3]]))
    assert dropped and cptr.tolist() == [0, 1, 2, 3] and list(zip(v.tolist(), rec["a"].tolist(), rec["b"].tolist())) == [
        (0, 1, 2), (1, 2, 0), (2, 0, 1)]


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
    assert int(re.search(r"#define\s+SN_MESH_CORNER_BYTES\s+(\d+)", src).group(1)) == eo.RECORD.itemsize == kernels.MESH_CORNER_BYTES
    assert "D_triangles <= D_edges" in text and "First order" in text
    assert lib.sn_mesh_corners_workspace_bytes(6890) >= 4 * 6891 and lib.sn_mesh_corners_workspace_bytes(-1) > 0


def test_argument_checks_return_status_codes_without_a_device():
    """Every refusal happens before any launch, so it can be seen on a box without a GPU (the pointers are never followed)."""
    from surfacenetworks_amd import _lib

    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    nmax = lib.sn_graph_apsp_max_vertices()
    assert lib.sn_mesh_geodesics_f32(p, p, nmax + 1, 0, 1, p, nmax + 1, None, None) == -7      # SN_E_UNSUPPORTED
    assert lib.sn_mesh_geodesics_sweeps_f32(p, p, nmax + 1, 0, 1, p, nmax + 1, None, None, None) == -7
    assert lib.sn_mesh_geodesics_f32(p, p, -1, 0, 0, p, 4, None, None) == -2                   # SN_E_SHAPE
    assert lib.sn_mesh_geodesics_f32(p, p, 4, 0, -1, p, 4, None, None) == -2
    assert lib.sn_mesh_geodesics_f32(p, p, 4, 2, 3, p, 4, None, None) == -2                    # sources past the last vertex
    assert lib.sn_mesh_geodesics_f32(None, p, 4, 0, 4, p, 4, None, None) == -1                 # SN_E_NULL
    assert lib.sn_mesh_geodesics_f32(p, p, 4, 0, 4, None, 4, None, None) == -1
    assert lib.sn_mesh_geodesics_f32(p, p, 4, 0, 4, p, 3, None, None) == -4                    # SN_E_LD
    assert lib.sn_mesh_geodesics_f32(p, p, 4, 0, 0, p, 4, None, None) == 0                     # nothing to do
    ws = lib.sn_mesh_corners_workspace_bytes(4)
    assert lib.sn_mesh_corners_f32(p, p, -1, 1, p, p, None, p, ws, None) == -2
    assert lib.sn_mesh_corners_f32(p, p, 4, -1, p, p, None, p, ws, None) == -2
    assert lib.sn_mesh_corners_f32(p, p, 4, 2 ** 30, p, p, None, p, ws, None) == -3            # SN_E_RANGE
    assert lib.sn_mesh_corners_f32(p, p, 4, 1, None, p, None, p, ws, None) == -1
    assert lib.sn_mesh_corners_f32(None, p, 4, 1, p, p, None, p, ws, None) == -1
    assert lib.sn_mesh_corners_f32(p, None, 4, 1, p, p, None, p, ws, None) == -1
    assert lib.sn_mesh_corners_f32(p, p, 4, 1, p, None, None, p, ws, None) == -1
    assert lib.sn_mesh_corners_f32(p, p, 4, 1, p, p, None, p, ws - 1, None) == -6              # SN_E_WORKSPACE
    assert lib.sn_mesh_corners_f32(p, p, 4, 1, p, p, None, None, ws, None) == -6


def test_cpu_tensors_and_unknown_methods_are_rejected():
    from surfacenetworks_amd import datasets, kernels, operators
    from surfacenetworks_amd import dense_correspondence as dc

    V, F = meshes()["torus"]
    Vt, Ft = torch.from_numpy(V.astype(np.float32)), torch.from_numpy(F.astype(np.int32))
    n = Vt.shape[0]
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.mesh_corners(Vt, Ft)
    table = kernels.MeshCorners(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(3, kernels.MESH_CORNER_BYTES, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.mesh_geodesics(table, n)
    with pytest.raises(RuntimeError, match="no CPU"):
        operators.geodesic_matrix_from_mesh(Vt, Ft, method="triangles")
    with pytest.raises(RuntimeError, match="no CPU"):
        datasets.faust_frame_from_mesh(V, F, device="cpu", geodesics="triangles")
    with pytest.raises(RuntimeError, match="no CPU"):
        dc.TorusBodies(1, n=9, m=14, pad_to=128, device="cpu", geodesics="triangles")
    for bad in ("exact", "graph", None):
        with pytest.raises(ValueError, match="method"):
            operators.geodesic_matrix_from_mesh(Vt, Ft, method=bad)
        with pytest.raises(ValueError, match="geodesics"):
            datasets.faust_frame_from_mesh(V, F, device="cpu", geodesics=bad)
    with pytest.raises(ValueError, match="geodesics"):
        dc.TorusBodies(1, n=9, m=14, pad_to=128, device="cpu", geodesics="exact")
