"""Geodesic matrices that cross triangles on the device — sn_mesh_corners_f32, sn_mesh_geodesics_f32 and what is built on them
(operators.geodesic_matrix_from_mesh(method="triangles"), datasets.faust_frame_from_mesh(geodesics="triangles"),
TorusBodies(geodesics="triangles")) — against tests/eikonal_oracle.py (numpy Jacobi sweeps of the same update).

Unlike the edge paths the value is not bit-reproducible across relaxation orders, so the comparison with the oracle has a
bound — derived, not fitted: |device - oracle| <= k ulp32(the row's largest oracle value), k = the largest sweep count the kernel
reports for the call.  Every stored value is one rounding of a quantity no larger than the row's maximum, the update is
non-expansive in its distance arguments, and a dependency chain is no longer than the sweeps that ran.  What is exact is tested
exactly: the corner table's indices and edge lengths, D_triangles <= D_edges, the hand cases, +inf and the flags."""
import numpy as np
import pytest
import torch

import eikonal_oracle as eo
import geodesic_oracle as go
from test_geodesics import meshes

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import _lib, datasets, kernels, mesh_ops, operators  # noqa: E402
from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402

NAMES = ["disc", "torus", "cloth"]


def dev_mesh(V, F):
    return torch.from_numpy(np.asarray(V).astype(np.float32)).to(DEV), torch.from_numpy(np.asarray(F).astype(np.int32)).to(DEV)


def device_rows(V, F, sources=None, out=None):
    """(D, flags, k): rows of the device matrix through the kernels' own entry, the flag word and the largest sweep count."""
    n = np.asarray(V).shape[0]
    corners = kernels.mesh_corners(*dev_mesh(V, F))
    count = n if sources is None else len(sources)
    sweeps = torch.zeros(max(count, 1), dtype=torch.int32, device=DEV)
    D, flags = kernels.mesh_geodesics(corners, n, sources=sources, out=out, sweeps=sweeps)
    return D, int(flags.item()), int(sweeps.max().item())


def ulps_off(got, want):
    """max over the entries of |got - want| in ulp32 of the row's largest finite oracle value; +inf must sit where the oracle
    has it."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and not np.isnan(got).any()
    top = np.where(inf, 0, want).max(axis=1).astype(np.float32)
    ulp = np.spacing(np.maximum(top, np.float32(1e-30)))[:, None].astype(np.float64)
    diff = np.where(inf, 0.0, np.abs(np.where(inf, 0, got).astype(np.float64) - np.where(inf, 0, want).astype(np.float64)))
    return float((diff / ulp).max())


@pytest.fixture(scope="module")
def oracle_D():
    """Full oracle matrices of the three small meshes, computed once and only read."""
    out = {k: eo.mesh_apsp(V, F) for k, (V, F) in meshes().items()}
    for D in out.values():
        D.setflags(write=False)
    return out


def host_table(corners):
    """(cptr, records) of a device corner table as numpy, the records as eo.RECORD."""
    cptr = corners.cptr.cpu().numpy()
    rec = corners.records.cpu().numpy().reshape(-1).view(eo.RECORD)[: cptr[-1]]
    return cptr, rec


def sorted_by_corner(v, rec):
    order = np.lexsort((rec["b"], rec["a"], v))
    return v[order], rec[order]


@pytest.mark.parametrize("name", NAMES)
def test_corner_table_equals_numpy(name):
    V, F = meshes()[name]
    corners = kernels.mesh_corners(*dev_mesh(V, F))
    cptr, rec = host_table(corners)
    o_cptr, o_v, o_rec, dropped = eo.corner_table(V, F)
    assert not dropped and corners.n == V.shape[0] and corners.records.shape == (3 * F.shape[0], kernels.MESH_CORNER_BYTES)
    assert np.array_equal(cptr, o_cptr) and cptr[-1] == 3 * F.shape[0]
    v, rec = sorted_by_corner(go.csr_rows(cptr), rec)               # the order within a vertex is not fixed: compare as multisets
    o_v, o_rec = sorted_by_corner(o_v, o_rec)
    for f in ("a", "b", "la", "lb"):
        assert np.array_equal(rec[f], o_rec[f]), f                 # indices and fp32 edge lengths bit for bit
    for f in ("c", "sb", "h"):
        np.testing.assert_allclose(rec[f], o_rec[f], rtol=1e-12, atol=0, err_msg=f)


def test_corner_table_drops_bad_faces_and_raises_the_flag():
    V, F = meshes()["cloth"]
    n = V.shape[0]
    bad = np.array([[3, 3, 7], [5, 9, 5], [8, 2, 2], [1, 2, n], [-1, 4, 6], [0, 1, 2 ** 31 - 1]], np.int64)
    Fb = np.concatenate([F[:40], bad[:3], F[40:], bad[3:]])
    Vd, Fd = dev_mesh(V, Fb)
    corners, flag = kernels._mesh_corner_table(Vd, Fd)
    assert int(flag.item()) == 1
    cptr, rec = host_table(corners)
    o_cptr, o_v, o_rec, dropped = eo.corner_table(V, F)             # the table of the good faces alone
    assert np.array_equal(cptr, o_cptr)
    v, rec = sorted_by_corner(go.csr_rows(cptr), rec)
    o_v, o_rec = sorted_by_corner(o_v, o_rec)
    for f in ("a", "b", "la", "lb"):
        assert np.array_equal(rec[f], o_rec[f]), f
    with pytest.raises(_lib.SnError, match="index"):
        kernels.mesh_corners(Vd, Fd)
    with pytest.raises(_lib.SnError, match="index"):
        operators.geodesic_matrix_from_mesh(Vd, Fd, method="triangles")
    _, flag = kernels._mesh_corner_table(*dev_mesh(V, F))           # the builder clears the flag itself
    assert int(flag.item()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_full_matrix_against_the_oracle(name, oracle_D):
    """n = 150, 126, 108: the last source group is partial for every group size."""
    V, F = meshes()[name]
    D, flags, k = device_rows(V, F)
    assert D.shape == (V.shape[0],) * 2 and D.dtype == torch.float32 and flags == 0
    off = ulps_off(D.cpu().numpy(), oracle_D[name])
    print(f"triangles {name}: device vs oracle {off:.2f} ulp32 of the row maximum, bound {k} (sweeps)")
    assert 1 <= k <= V.shape[0] and off <= k
    D2 = operators.geodesic_matrix_from_mesh(*dev_mesh(V, F), symmetric=False, method="triangles")
    assert ulps_off(D2.cpu().numpy(), oracle_D[name]) <= k
    Gs = operators.geodesic_matrix_from_mesh(*dev_mesh(V, F), method="triangles")
    assert torch.equal(Gs, Gs.T)
    Dk = D.clone()
    assert torch.equal(kernels.symmetrize_min_(Dk), torch.minimum(D, D.T))         # min(D, D^T) of the device's own D
    assert ulps_off(Gs.cpu().numpy(), np.minimum(oracle_D[name], oracle_D[name].T)) <= k


@pytest.mark.parametrize("name", NAMES)
def test_triangles_never_exceed_edges(name):
    """Exact: the edge candidates are the edge kernel's own fp32 sums (and every mesh edge is in some corner, while the edge
    method walks the Laplacian's pattern, a subset)."""
    Vd, Fd = dev_mesh(*meshes()[name])
    for symmetric in (False, True):
        T = operators.geodesic_matrix_from_mesh(Vd, Fd, symmetric=symmetric, method="triangles")
        E = operators.geodesic_matrix_from_mesh(Vd, Fd, symmetric=symmetric, method="edges")
        assert torch.equal(E, operators.geodesic_matrix_from_mesh(Vd, Fd, symmetric=symmetric))       # the default is "edges"
        assert bool((T <= E).all()) and bool((T < E).any())


@pytest.mark.parametrize("name", ["grid", "disc"])
def test_flat_meshes_against_the_chord(name):
    V, F = eo.flat_fixtures()[name]
    n = V.shape[0]
    Cd = eo.chord(V)
    D = operators.geodesic_matrix_from_mesh(*dev_mesh(V, F), symmetric=False, method="triangles").cpu().numpy()
    assert (D >= Cd * (1 - n * 2.0 ** -23)).all()
    Do = eo.mesh_apsp(V, F)
    err, err_o = eo.mean_rel_error(np.minimum(D, D.T), Cd), eo.mean_rel_error(np.minimum(Do, Do.T), Cd)
    print(f"flat {name}: mean relative error device {err:.6f}, oracle {err_o:.6f}")
    assert err <= err_o + 1e-6


def test_hand_cases():
    sq = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    Fq = np.array([[0, 1, 3], [1, 2, 3]])
    D = operators.geodesic_matrix_from_mesh(*dev_mesh(sq, Fq), symmetric=False, method="triangles").cpu().numpy()
    want = np.float32(1 + np.sqrt(0.5))
    assert D[0][2] == want and D[2][0] == want and D[0].tolist() == [0, 1, float(want), 1]
    assert D[1][3] == np.float32(np.sqrt(2.0))                     # along the diagonal, an edge
    tri = np.array([[0, 0, 0], [3, 4, 0], [6, 0, 0]], np.float64)  # one triangle, sides 5, 5, 6
    G = operators.geodesic_matrix_from_mesh(*dev_mesh(tri, [[0, 1, 2]]), method="triangles")
    assert G.cpu().tolist() == [[0.0, 5.0, 6.0], [5.0, 0.0, 5.0], [6.0, 5.0, 0.0]]
    one = operators.geodesic_matrix_from_mesh(torch.zeros(1, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV),
                                              method="triangles")
    assert one.cpu().tolist() == [[0.0]]                            # one vertex, no face
    # a zero-area face (three collinear vertices) next to a proper one, and two coincident vertices 1 and 4
    V = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 0], [1, 0, 0], [0.5, -1, 0]], np.float64)
    F = np.array([[0, 1, 2], [0, 2, 3], [0, 5, 4], [4, 5, 2], [1, 4, 3]])
    D, flags, k = device_rows(V, F)
    want = eo.mesh_apsp(V, F)
    assert flags == 0 and np.isfinite(want).all() and want[1][4] == 0
    assert ulps_off(D.cpu().numpy(), want) <= k


def test_unreachable_vertices_keep_inf_and_are_reported():
    """An isolated vertex, and two disjoint components."""
    V, F = meshes()["cloth"]
    V2, F2 = meshes()["torus"]
    cases = {"isolated": (np.concatenate([V, [[9.0, 9.0, 9.0]]]), F),
             "components": (np.concatenate([V, V2 + 5.0]), np.concatenate([F, F2 + V.shape[0]]))}
    for name, (Vc, Fc) in cases.items():
        want = eo.mesh_apsp(Vc, Fc)
        assert np.isinf(want).any()
        D, flags, k = device_rows(Vc, Fc)
        assert flags == 1, name                                    # bit 1: +inf left; bit 2 (not converged) clear
        assert ulps_off(D.cpu().numpy(), want) <= k, name          # (ulps_off also wants +inf exactly where the oracle has it)
        Vd, Fd = dev_mesh(Vc, Fc)
        Gs = operators.geodesic_matrix_from_mesh(Vd, Fd, require_connected=False, method="triangles")
        assert ulps_off(Gs.cpu().numpy(), np.minimum(want, want.T)) <= k and torch.equal(Gs, Gs.T)
        with pytest.raises(ValueError, match="disconnected"):
            operators.geodesic_matrix_from_mesh(Vd, Fd, method="triangles")


def test_source_window_into_a_wider_matrix(oracle_D):
    V, F = meshes()["disc"]
    n = V.shape[0]
    out = torch.full((20, n + 5), float("nan"), device=DEV)
    D, flags, k = device_rows(V, F, sources=range(37, 50), out=out)
    assert D is out and flags == 0
    got = out.cpu().numpy()
    assert ulps_off(np.ascontiguousarray(got[:13, :n]), oracle_D["disc"][37:50]) <= k
    assert np.isnan(got[13:]).all() and np.isnan(got[:, n:]).all()


def _grid_for(lo, hi, exact=False):
    """(a, b) with lo < a * b <= hi, a * b as large as possible and the grid as square as its factors allow."""
    for n in range(hi, lo, -1):
        divs = [a for a in range(2 if exact else 8, int(n ** 0.5) + 1) if n % a == 0]
        if divs:
            return divs[-1], n // divs[-1]
        assert not exact, f"{n} has no factor pair"
    raise AssertionError((lo, hi))


@pytest.mark.parametrize("S", [8, 4, 2, 1])
def test_every_dispatch_leg(S):
    """One grid_cloth per group size the dispatcher can choose, at the upper end of its range; S = 1 at the largest supported
    n itself (a 12 x 3413 strip: thousands of sweeps).  The last three sources (a partial group) for S = 8, 4, 2, the last
    one for S = 1."""
    lib = _lib.load()
    nmax = int(lib.sn_graph_apsp_max_vertices())
    a, b = _grid_for(nmax // (2 * S), nmax // S, exact=(S == 1))
    n = a * b
    assert int(lib.sn_graph_apsp_group(n)) == S and (S > 1 or n == nmax)
    V, F = mesh_ops.grid_cloth(a, b, np.random.default_rng(S))
    window = range(n - 3, n) if S > 1 else range(n - 1, n)
    D, flags, k = device_rows(V, F, sources=window)
    want = eo.mesh_apsp(V, F, sources=window)
    off = ulps_off(D.cpu().numpy(), want)
    print(f"S = {S}, n = {n} ({a} x {b}): {off:.2f} ulp32, {k} sweeps")
    assert flags == 0 and 1 <= k <= n and off <= k


def test_strip_that_needs_hundreds_of_sweeps():
    """300 quads in a row, 602 vertices, sources at both ends: the Jacobi oracle needs 302 sweeps."""
    m = 301
    V = np.zeros((2 * m, 3))
    V[:m, 0] = V[m:, 0] = np.arange(m) * 0.75
    V[m:, 1] = 1.0
    i = np.arange(m - 1)
    F = np.concatenate([np.stack([i, i + 1, m + i], 1), np.stack([i + 1, m + i + 1, m + i], 1)])
    n = 2 * m
    for window, first in ((range(0, 3), 0), (range(n - 3, n), n - 1)):
        want, o_sweeps = eo.mesh_apsp(V, F, sources=window, with_sweeps=True)
        D, flags, k = device_rows(V, F, sources=window)
        print(f"strip {window}: device {k} sweeps, Jacobi oracle {o_sweeps}")
        assert o_sweeps == 302 and 1 <= k <= n and flags == 0       # converged: bit 2 clear, nothing unreached
        assert ulps_off(D.cpu().numpy(), want) <= k


def test_more_vertices_than_the_lds_holds_are_refused_before_any_launch():
    lib = _lib.load()
    n = int(lib.sn_graph_apsp_max_vertices()) + 1
    table = kernels.MeshCorners(torch.zeros(n + 1, dtype=torch.int32, device=DEV),
                                torch.zeros(3, kernels.MESH_CORNER_BYTES, dtype=torch.uint8, device=DEV))
    out = torch.full((1, n), -1.0, device=DEV)
    st = lib.sn_mesh_geodesics_f32(table.cptr.data_ptr(), table.records.data_ptr(), n, 0, 1, out.data_ptr(), n, None, None)
    assert st == -7                                                              # SN_E_UNSUPPORTED
    with pytest.raises(_lib.SnError, match="at most"):
        kernels.mesh_geodesics(table, n, sources=range(1), out=out)
    with pytest.raises(ValueError, match="at most"):
        operators.geodesic_matrix_from_mesh(torch.zeros(n, 3, device=DEV), torch.zeros(1, 3, dtype=torch.int32, device=DEV),
                                            method="triangles")
    torch.cuda.synchronize()
    assert (out == -1).all()


def test_frames_from_raw_meshes_train_and_evaluate():
    """faust_frame_from_mesh(geodesics="triangles") -> FaustFrames -> PairBatch / forward_loss / evaluate_pair; G of every
    stored frame is the device matrix in the stored numbering."""
    from helpers import deterministic_init

    rng = np.random.default_rng(11)
    raw, frames = [], []
    for _ in range(2):
        V, F = mesh_ops.torus_grid(9, 14, rng)
        label = rng.permutation(V.shape[0])
        raw.append((V, F, label))
        frames.append(datasets.faust_frame_from_mesh(V, F, label, device=DEV, geodesics="triangles"))
    ds = dc.FaustFrames(frames, model="lap", pad_to=128, device=DEV)
    for i, (V, F, label) in enumerate(raw):
        G = operators.geodesic_matrix_from_mesh(*dev_mesh(V, F), method="triangles")
        edges = datasets.faust_frame_from_mesh(V, F, label, device=DEV)["G"]
        assert bool((G <= edges).all()) and bool((G < edges).any())
        want = eo.mesh_apsp(V, F, symmetric=True)
        assert ulps_off(G.cpu().numpy(), want) <= V.shape[0]
        # two runs may differ by the ulps the bound allows, so the stored G is compared with a device matrix the same way
        vo = np.arange(V.shape[0]) if ds.orders[i].identity else ds.orders[i].vorder
        assert torch.equal(frames[i]["G"], frames[i]["G"].T)
        assert torch.equal(ds.frames[i]["G"], frames[i]["G"][torch.from_numpy(vo).to(DEV)][:, torch.from_numpy(vo).to(DEV)])
        assert ulps_off(frames[i]["G"].cpu().numpy(), want) <= V.shape[0]
    model = deterministic_init(dc.SiameseModel("lap", 2), 5).to(DEV).train()
    for name in ("dcel", "sl1"):
        model.zero_grad()
        loss = dc.forward_loss(model, dc.PairBatch(ds, 0, 1, loss=name))
        assert torch.isfinite(loss).all()
        loss.sum().backward()
        assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    ev = dc.evaluate_pair(model, ds, 0, 1)
    assert torch.isfinite(ev["mean_error"]) and float(ev["mean_error"]) >= 0


def test_torus_bodies_with_triangle_geodesics():
    ds = dc.TorusBodies(2, n=9, m=14, pad_to=128, device=DEV, geodesics="triangles")
    graph = dc.TorusBodies(2, n=9, m=14, pad_to=128, device=DEV, geodesics="graph")
    for i in range(2):
        assert torch.equal(ds.frames[i]["V"], graph.frames[i]["V"]) and torch.equal(ds.frames[i]["label"], graph.frames[i]["label"])
        T, E = ds.frames[i]["G"], graph.frames[i]["G"]
        assert T.shape == E.shape and bool((T <= E).all()) and bool((T < E).any()) and torch.equal(T, T.T)
