"""Geodesic (edge-path) distance matrices on the device — sn_edge_lengths_csr_f32, sn_graph_apsp_f32, sn_symmetrize_min_f32
and what is built on them (operators.geodesic_matrix_from_mesh, datasets.faust_frame_from_mesh, TorusBodies(geodesics="graph"))
— against tests/geodesic_oracle.py (fp32 heap Dijkstra).

The value is a property of the graph, not of the relaxation order (tests/test_geodesics.py pins that on the host), so every
comparison here is bit equality: np.array_equal / torch.equal, no tolerance."""
import numpy as np
import pytest
import torch

import geodesic_oracle as go
from test_geodesics import meshes

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import _lib, datasets, kernels, mesh_ops, operators  # noqa: E402
from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402


def dev_graph(rowptr, colind, w):
    return (torch.from_numpy(np.ascontiguousarray(rowptr)).to(DEV), torch.from_numpy(np.ascontiguousarray(colind)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(w)).to(DEV))


def dev_mesh(V, F):
    return torch.from_numpy(V.astype(np.float32)).to(DEV), torch.from_numpy(F.astype(np.int32)).to(DEV)


@pytest.fixture(scope="module")
def oracle_D():
    """Full oracle matrices of the three small meshes, computed once and only read."""
    out = {k: go.mesh_apsp(V, F) for k, (V, F) in meshes().items()}
    for D in out.values():
        D.setflags(write=False)
    return out


@pytest.mark.parametrize("name", ["disc", "torus", "cloth"])
def test_edge_lengths_equal_the_numpy_formula(name):
    V, F = meshes()[name]
    Vd, Fd = dev_mesh(V, F)
    rowptr, colind, _ = kernels.laplacian_from_mesh(Vd, Fd)
    w = kernels.edge_lengths_csr(Vd, rowptr, colind)
    rp, ci = rowptr.cpu().numpy(), colind.cpu().numpy()
    rows = go.csr_rows(rp)
    assert np.array_equal(w.cpu().numpy(), go.edge_weights(V, rows, ci))
    assert (w[torch.from_numpy(rows == ci).to(DEV)] == 0).all()                 # the Laplacian's diagonal: a zero self-loop
    # and the pattern is the mesh's vertex adjacency plus the diagonal, as the oracle builds it
    o_rp, o_ci, o_w = go.mesh_graph(V, F)
    order = np.lexsort((ci, rows))
    assert np.array_equal(rp, o_rp) and np.array_equal(ci[order], o_ci) and np.array_equal(w.cpu().numpy()[order], o_w)


@pytest.mark.parametrize("name", ["disc", "torus", "cloth"])
def test_full_matrix_equals_the_oracle(name, oracle_D):
    """n = 150, 126, 108: the last source group is partial for every group size."""
    V, F = meshes()[name]
    D = operators.geodesic_matrix_from_mesh(*dev_mesh(V, F), symmetric=False)
    assert D.shape == (V.shape[0],) * 2 and D.dtype == torch.float32
    assert np.array_equal(D.cpu().numpy(), oracle_D[name])
    Gs = operators.geodesic_matrix_from_mesh(*dev_mesh(V, F))
    assert np.array_equal(Gs.cpu().numpy(), np.minimum(oracle_D[name], oracle_D[name].T))
    assert torch.equal(Gs, Gs.T)


def test_one_and_two_vertices():
    rp, ci, w = dev_graph(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    D, unreached = kernels.graph_apsp(rp, ci, w, 1)
    assert D.cpu().tolist() == [[0.0]] and int(unreached.item()) == 0
    rp, ci, w = dev_graph(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([0.75, 0.5], np.float32))
    D, unreached = kernels.graph_apsp(rp, ci, w, 2)
    assert D.cpu().tolist() == [[0.0, 0.5], [0.75, 0.0]] and int(unreached.item()) == 0      # entry (v, u): the edge u -> v
    rp, ci, w = dev_graph(np.zeros(3, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))      # two vertices, no edge
    D, unreached = kernels.graph_apsp(rp, ci, w, 2)
    assert D.cpu().tolist() == [[0.0, np.inf], [np.inf, 0.0]] and int(unreached.item()) == 1
    V = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [6.0, 0.0, 0.0]], device=DEV)            # one triangle, sides 5, 5, 6
    G = operators.geodesic_matrix_from_mesh(V, torch.tensor([[0, 1, 2]], device=DEV))
    assert G.cpu().tolist() == [[0.0, 5.0, 6.0], [5.0, 0.0, 5.0], [6.0, 5.0, 0.0]]


def test_unreachable_vertices_keep_inf_and_are_reported():
    """An isolated vertex, and two disjoint components."""
    V, F = meshes()["cloth"]
    V2, F2 = meshes()["torus"]
    cases = {"isolated": (np.concatenate([V, [[9.0, 9.0, 9.0]]]), F),
             "components": (np.concatenate([V, V2 + 5.0]), np.concatenate([F, F2 + V.shape[0]]))}
    for name, (Vc, Fc) in cases.items():
        want = go.mesh_apsp(Vc, Fc)
        assert np.isinf(want).any()
        Vd, Fd = dev_mesh(Vc, Fc)
        D = operators.geodesic_matrix_from_mesh(Vd, Fd, symmetric=False, require_connected=False)
        assert np.array_equal(D.cpu().numpy(), want), name
        Gs = operators.geodesic_matrix_from_mesh(Vd, Fd, require_connected=False)
        assert np.array_equal(Gs.cpu().numpy(), np.minimum(want, want.T)), name
        rowptr, colind, _ = kernels.laplacian_from_mesh(Vd, Fd)
        _, unreached = kernels.graph_apsp(rowptr, colind, kernels.edge_lengths_csr(Vd, rowptr, colind), Vc.shape[0])
        assert int(unreached.item()) == 1
        with pytest.raises(ValueError, match="disconnected"):
            operators.geodesic_matrix_from_mesh(Vd, Fd)


def test_source_window_into_a_wider_matrix(oracle_D):
    V, F = meshes()["disc"]
    n = V.shape[0]
    rp, ci, w = dev_graph(*go.mesh_graph(V, F))
    out = torch.full((20, n + 5), float("nan"), device=DEV)
    D, unreached = kernels.graph_apsp(rp, ci, w, n, sources=range(37, 50), out=out)
    assert D is out and int(unreached.item()) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:13, :n], oracle_D["disc"][37:50])
    assert np.isnan(got[13:]).all() and np.isnan(got[:, n:]).all()


def test_chain_numbered_against_the_sweep():
    """600 vertices in a row: a pull sweep carries a distance one hop, so a source at one end needs ~600 sweeps to reach the
    other — in one of the two directions whatever order the lanes run in.  A loop bound below n would leave inf behind."""
    n = 600
    rng = np.random.default_rng(3)
    rows = np.concatenate([np.arange(n - 1), np.arange(1, n)])
    cols = np.concatenate([np.arange(1, n), np.arange(n - 1)])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    w = (rng.random(rows.size) + 0.01).astype(np.float32)
    g = (rowptr, cols.astype(np.int32), w)
    rp, ci, wd = dev_graph(*g)
    for window in (range(0, 5), range(n - 5, n)):
        sweeps = torch.zeros(8, dtype=torch.int32, device=DEV)
        D, unreached = kernels.graph_apsp(rp, ci, wd, n, sources=window, sweeps=sweeps)
        assert np.array_equal(D.cpu().numpy(), go.apsp_f32(*g, sources=window))
        assert int(unreached.item()) == 0 and 1 <= int(sweeps[0].item()) <= n
        print(f"chain {window}: {int(sweeps[0].item())} sweeps")


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
    """One grid_cloth per group size the dispatcher can choose (S = the largest of 8, 4, 2, 1 with S * n <= max), at the upper
    end of its range; S = 1 at the largest supported n itself.  Three sources at the end of the vertex range: a partial group."""
    lib = _lib.load()
    nmax = int(lib.sn_graph_apsp_max_vertices())
    a, b = _grid_for(nmax // (2 * S), nmax // S, exact=(S == 1))
    n = a * b
    assert int(lib.sn_graph_apsp_group(n)) == S and (S > 1 or n == nmax)
    V, F = mesh_ops.grid_cloth(a, b, np.random.default_rng(S))
    g = go.mesh_graph(V, F)
    rp, ci, w = dev_graph(*g)
    window = range(n - 3, n)
    D, unreached = kernels.graph_apsp(rp, ci, w, n, sources=window)
    assert np.array_equal(D.cpu().numpy(), go.apsp_f32(*g, sources=window))
    assert int(unreached.item()) == 0


def test_more_vertices_than_the_lds_holds_are_refused_before_any_launch():
    lib = _lib.load()
    n = int(lib.sn_graph_apsp_max_vertices()) + 1
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    colind = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = torch.zeros(1, device=DEV)
    out = torch.full((1, n), -1.0, device=DEV)
    st = lib.sn_graph_apsp_f32(rowptr.data_ptr(), colind.data_ptr(), w.data_ptr(), n, 0, 1, out.data_ptr(), n, None, None)
    assert st == -7                                                              # SN_E_UNSUPPORTED
    with pytest.raises(_lib.SnError, match="at most"):
        kernels.graph_apsp(rowptr, colind, w, n, sources=range(1), out=out)
    with pytest.raises(ValueError, match="at most"):
        operators.geodesic_matrix_from_mesh(torch.zeros(n, 3, device=DEV), torch.zeros(1, 3, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert (out == -1).all()


@pytest.mark.parametrize("n", [1, 63, 150])
def test_symmetrize_min_in_place(n):
    g = torch.Generator().manual_seed(n)
    full = torch.rand(n, n + 3, generator=g)
    G = full.to(DEV)
    got = kernels.symmetrize_min_(G[:, :n])
    assert got.data_ptr() == G.data_ptr()
    D = full[:, :n].numpy()
    want = np.minimum(D, D.T)
    res = G.cpu().numpy()
    assert np.array_equal(res[:, :n], want) and np.array_equal(res[:, :n], res[:, :n].T)
    assert np.array_equal(res[:, n:], full[:, n:].numpy())


def test_frames_from_raw_meshes_train_and_evaluate():
    """datasets.faust_frame_from_mesh -> FaustFrames -> PairBatch / forward_loss / evaluate_pair, with no file and no host
    geodesics: G of every stored frame is the oracle's symmetric matrix in the stored numbering."""
    from helpers import deterministic_init

    rng = np.random.default_rng(11)
    raw, frames = [], []
    for _ in range(2):
        V, F = mesh_ops.torus_grid(9, 14, rng)
        label = rng.permutation(V.shape[0])
        raw.append((V, F, label))
        frames.append(datasets.faust_frame_from_mesh(V, F, label, device=DEV))
    ident = datasets.faust_frame_from_mesh(*raw[0][:2], device=DEV)
    assert torch.equal(ident["label"], torch.arange(126, device=DEV)) and torch.equal(ident["label_inv"], ident["label"])
    assert set(frames[0]) == {"V", "F", "L", "Di", "DiA", "label", "label_inv", "G"}
    ds = dc.FaustFrames(frames, model="lap", pad_to=128, device=DEV)
    for i, (V, F, label) in enumerate(raw):
        D = go.mesh_apsp(V, F)
        want = np.minimum(D, D.T)
        assert np.array_equal(frames[i]["G"].cpu().numpy(), want)
        vo = np.arange(V.shape[0]) if ds.orders[i].identity else ds.orders[i].vorder
        assert np.array_equal(ds.frames[i]["G"].cpu().numpy(), want[vo][:, vo])
        assert torch.equal(ds.frames[i]["label_inv"][ds.frames[i]["label"]], torch.arange(V.shape[0], device=DEV))
    model = deterministic_init(dc.SiameseModel("lap", 2), 5).to(DEV).train()
    for name in ("dcel", "sl1"):
        model.zero_grad()
        loss = dc.forward_loss(model, dc.PairBatch(ds, 0, 1, loss=name))
        assert torch.isfinite(loss).all()
        loss.sum().backward()
        assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    ev = dc.evaluate_pair(model, ds, 0, 1)
    assert torch.isfinite(ev["mean_error"]) and float(ev["mean_error"]) >= 0


def test_torus_bodies_with_graph_geodesics():
    ds = dc.TorusBodies(2, n=9, m=14, pad_to=128, device=DEV, geodesics="graph")
    plain = dc.TorusBodies(2, n=9, m=14, pad_to=128, device=DEV)
    rng = np.random.default_rng(4)                                   # TorusBodies' default seed and draw order
    for i in range(2):
        V, F = mesh_ops.torus_grid(9, 14, rng)
        rng.permutation(V.shape[0])
        D = go.mesh_apsp(V, F)
        assert np.array_equal(ds.frames[i]["G"].cpu().numpy(), np.minimum(D, D.T))
        Vd = torch.from_numpy(V.astype(np.float32)).to(DEV)
        assert torch.equal(ds.frames[i]["V"], Vd) and torch.equal(ds.frames[i]["label"], plain.frames[i]["label"])
        assert torch.equal(plain.frames[i]["G"], torch.cdist(Vd, Vd))
        V64 = V.astype(np.float32).astype(np.float64)                # no edge path is shorter than the chord, up to the
        chord = np.sqrt(((V64[:, None] - V64[None]) ** 2).sum(-1))   # n 2^-23 of the fp32 path sums (tests/test_geodesics.py)
        assert (ds.frames[i]["G"].cpu().numpy() >= chord * (1 - V.shape[0] * 2.0 ** -23)).all()
