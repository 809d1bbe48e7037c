"""Device builder of the intrinsic Delaunay Laplacian (sn_mesh_glue_i32, sn_mesh_idt_rounds_f64, sn_mesh_idt_laplacian_f32)
against the host function mesh_ops.intrinsic_delaunay / intrinsic_laplacian on the named meshes of tests/intrinsic_cases.py:
the edge multiset exactly, lengths and values within bounds that come from the HOST function's own spread between flip orders
(never from the device): intrinsic_cases.SPREAD_L = 1e-13 (measured 1.8e-14, mesh D) and SPREAD_LAP = 1e-12 of the row maximum
(measured 1.1e-13, mesh F_disc), times 64 for the device — a different schedule and other roundings; both products stay below
1e-9, five orders under the 1e-4-and-up error of a wrong or missed flip.  Measured on an MI355X: lengths at most 7.9e-15
relative from the host's fifo run (mesh B), every fp32 value of every mesh equal to the host's bit for bit.  Also: bit-identical reruns, the batch form, the
unchanged default path, the refusals and the dataset keyword end to end.

The 0-flip mesh is the disc with z = 0 (intrinsic_cases.flat_disc): delaunay_disc(150, default_rng(5)) as generated has two
genuinely non-Delaunay edges (cot sums -5.5e-2 and -1.2e-3), tests/test_intrinsic.py covers it."""
import numpy as np
import pytest
import torch

import intrinsic_cases as ic

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import datasets, kernels, mesh_ops  # noqa: E402
from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402
from surfacenetworks_amd.operators import laplacian_operator_from_mesh  # noqa: E402


def dev_mesh(V, F):
    return torch.from_numpy(np.asarray(V, np.float32)).to(DEV), torch.from_numpy(np.asarray(F, np.int32)).to(DEV)


_runs = {}


def device_run(name):
    """(state, (rowptr, colind, vals)) of the device builder, once per mesh."""
    if name not in _runs:
        V, F = ic.meshes()[name] if name != "flat" else ic.flat_disc()
        Vd, Fd = dev_mesh(V, F)
        state = kernels.intrinsic_delaunay(Vd, Fd)
        _runs[name] = (state, kernels.intrinsic_laplacian_from_mesh(Vd, Fd, state=state))
    return _runs[name]


@pytest.mark.parametrize("name", ic.NAMES)
def test_device_against_host(name):
    V, F = ic.meshes()[name]
    (Fp, l, G, status, rounds, flips), (rowptr, colind, vals) = device_run(name)
    hF, hl, hG, hflips = ic.host_state(name)
    print(f"{name}: device {flips} flips in {rounds} rounds (status {status}), host {hflips} flips")
    assert status == 0 and flips > 0 and 1 < rounds < 1024
    Fp, l, G = Fp.cpu().numpy(), l.cpu().numpy(), G.cpu().numpy()
    e, ll = ic.sorted_sides(Fp, l)
    he, hll = ic.sorted_sides(hF, hl)
    assert np.array_equal(e, he)                                   # the edge multiset, exactly
    err_l = float((np.abs(ll - hll) / hll).max())
    inner = G >= 0
    assert np.array_equal(G[G[inner] // 3, G[inner] % 3], np.arange(G.size).reshape(G.shape)[inner])
    margin, degenerate = mesh_ops.delaunay_margin(l, G)
    assert degenerate == 0 and margin > 1e-6
    L = ic.host_laplacian(name)
    assert np.array_equal(rowptr.cpu().numpy(), L.indptr) and np.array_equal(colind.cpu().numpy(), L.indices)
    h32 = L.data.astype(np.float32)
    rowmax = np.repeat(np.abs(L).max(axis=1).toarray().ravel(), np.diff(L.indptr))
    diff = np.abs(vals.cpu().numpy().astype(np.float64) - h32.astype(np.float64))
    bound = np.spacing(np.abs(h32)).astype(np.float64) + ic.DEVICE_FACTOR * ic.SPREAD_LAP * rowmax
    print(f"{name}: max |l'_dev - l'_host| / l'_host = {err_l:.2e} (bound {ic.DEVICE_FACTOR * ic.SPREAD_L:.1e}); "
          f"max |vals_dev - vals_host32| / bound = {float((diff / bound).max()):.3f}; {int((diff > 0).sum())} of {diff.size} values differ")
    assert (np.abs(ll - hll) <= ic.DEVICE_FACTOR * ic.SPREAD_L * hll).all()
    assert (diff <= bound).all()


def test_zero_flip_mesh_runs_one_round_and_keeps_the_faces():
    V, F = ic.flat_disc()
    (Fp, l, G, status, rounds, flips), (rowptr, colind, vals) = device_run("flat")
    assert (status, rounds, flips) == (0, 1, 0)
    assert np.array_equal(Fp.cpu().numpy(), F)
    assert np.array_equal(l.cpu().numpy(), mesh_ops.edge_lengths(V, F))          # the start lengths: numpy's values bit for bit
    assert np.array_equal(G.cpu().numpy(), mesh_ops.mesh_glue(F, V.shape[0]))
    L = ic.host_laplacian("flat")
    assert np.array_equal(rowptr.cpu().numpy(), L.indptr) and np.array_equal(colind.cpu().numpy(), L.indices)
    h32 = L.data.astype(np.float32)
    print(f"flat: {int((vals.cpu().numpy() != h32).sum())} of {h32.size} values differ from the host's")
    rowmax = np.repeat(np.abs(L).max(axis=1).toarray().ravel(), np.diff(L.indptr))
    assert (np.abs(vals.cpu().numpy().astype(np.float64) - h32) <= np.spacing(np.abs(h32)) + ic.DEVICE_FACTOR * ic.SPREAD_LAP * rowmax).all()
    Gonly, st = kernels.mesh_glue(dev_mesh(V, F)[1], V.shape[0])
    assert torch.equal(Gonly, G) and int(st.item()) == 0


@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_two_device_runs_are_bit_identical(name):
    V, F = ic.meshes()[name]
    Vd, Fd = dev_mesh(V, F)
    (Fp, l, G, status, rounds, flips), (_, _, vals) = device_run(name)
    again = kernels.intrinsic_delaunay(Vd, Fd)
    assert torch.equal(again[0], Fp) and torch.equal(again[1], l) and torch.equal(again[2], G)
    assert again[3:] == (status, rounds, flips)
    assert torch.equal(kernels.intrinsic_laplacian_from_mesh(Vd, Fd)[2], vals)


def test_batch_is_block_diagonal_of_the_single_meshes():
    V, F = ic.meshes()["A"]
    Vb = np.stack([V * np.array([1.0, 1.0, z]) for z in (1.0, 2.5, 6.0)])
    Fd = dev_mesh(V, F)[1]
    Lb = laplacian_operator_from_mesh(torch.from_numpy(Vb.astype(np.float32)).to(DEV), Fd, intrinsic=True)
    nV = V.shape[0]
    assert Lb.shape == (3 * nV, 3 * nV)
    rp, ci, va, base = [], [], [], 0
    for b in range(3):
        op = laplacian_operator_from_mesh(dev_mesh(Vb[b], F)[0], Fd, intrinsic=True)
        rp.append(op.rowptr[:-1] + base)
        ci.append(op.colind + b * nV)
        va.append(op.vals)
        base += int(op.rowptr[-1])
    rp.append(torch.tensor([base], dtype=torch.int32, device=DEV))
    assert torch.equal(Lb.rowptr, torch.cat(rp)) and torch.equal(Lb.colind, torch.cat(ci)) and torch.equal(Lb.vals, torch.cat(va))
    assert int(Lb.rowptr[nV]) != int(Lb.rowptr[3 * nV]) - int(Lb.rowptr[2 * nV])      # the three blocks are different triangulations


def test_default_path_is_unchanged():
    V, F = ic.meshes()["A"]
    Vd, Fd = dev_mesh(V, F)
    op = laplacian_operator_from_mesh(Vd, Fd)
    rowptr, colind, vals = kernels.laplacian_from_mesh(Vd, Fd)
    assert torch.equal(op.rowptr, rowptr) and torch.equal(op.colind, colind) and torch.equal(op.vals, vals)
    ref = mesh_ops.laplacian(V, F).astype(np.float32)
    ref.sort_indices()
    assert np.array_equal(op.to_scipy().toarray(), ref.toarray())


@pytest.mark.parametrize("faces,nv,what,bit", [
    ([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 5, "more than two faces", kernels.IDT_NON_MANIFOLD),
    ([[0, 1, 2], [0, 1, 3]], 4, "same direction", kernels.IDT_ORIENTATION),
    ([[0, 1, 2], [1, 0, 4]], 4, "outside", kernels.IDT_BAD_FACE),
    ([[0, 1, 2], [1, 0, 0]], 4, "repeated", kernels.IDT_BAD_FACE)], ids=["three_faces", "orientation", "range", "repeated"])
def test_refusals_raise_value_error(faces, nv, what, bit):
    V = torch.from_numpy(np.random.default_rng(0).random((nv, 3)).astype(np.float32)).to(DEV)
    F = torch.tensor(faces, dtype=torch.int32, device=DEV)
    Fp, l, G, status, rounds, flips = kernels.intrinsic_delaunay(V, F)
    assert status & bit and flips == 0 and torch.equal(Fp, F)      # nothing is flipped on such input
    with pytest.raises(ValueError, match=what):
        laplacian_operator_from_mesh(V, F, intrinsic=True)


def test_max_rounds_exhausted_raises_runtime_error():
    Vd, Fd = dev_mesh(*ic.meshes()["C"])
    state = kernels.intrinsic_delaunay(Vd, Fd, max_rounds=1)
    assert state[3] == kernels.IDT_NOT_CONVERGED and state[4] == 1 and state[5] > 0
    with pytest.raises(RuntimeError, match="non-Delaunay"):
        laplacian_operator_from_mesh(Vd, Fd, intrinsic=True, max_rounds=1)


def test_faust_frame_with_the_intrinsic_laplacian_end_to_end():
    V, F = ic.meshes()["A"]
    fr = datasets.faust_frame_from_mesh(V, F, device=DEV, laplacian="intrinsic")
    L = ic.host_laplacian("A")
    assert fr["L"].dtype == np.float32 and np.array_equal(fr["L"].indptr, L.indptr) and np.array_equal(fr["L"].indices, L.indices)
    ext = datasets.faust_frame_from_mesh(V, F, device=DEV)["L"]
    assert ext.shape == fr["L"].shape and not np.array_equal(ext.indices, fr["L"].indices)      # (flips keep the number of edges)
    off = fr["L"].tocoo()
    assert ((ext.tocoo().data > 0) & (ext.tocoo().row != ext.tocoo().col)).sum() == 186 and not ((off.data > 0) & (off.row != off.col)).any()
    for model in ("lap", "amp"):
        ds = dc.FaustFrames([fr], model=model, pad_to=256, device=DEV)
        inputs, target, mask, ops = ds.sample(0)
        assert inputs.shape == (1, 256, 3) and int(mask.sum()) == V.shape[0]
        for op in (ops if model == "amp" else [ops]):
            assert op.shape == (256, 256) and bool(torch.isfinite(op.vals).all())
    tb = dc.TorusBodies(1, n=9, m=14, pad_to=128, device=DEV, laplacian="intrinsic")
    assert tb.sample(0)[3].shape == (128, 128)
