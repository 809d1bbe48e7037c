"""Sparse x sparse CSR products on the device (sn_csr_spgemm_f32, sn_csr_scale_sym_f32, sn_csr_inv_sqrt_degree_f32) against the
plain-numpy emulation of their written definition (tests/amplify_cases.py) — bit for bit, pattern included — and against the
host function dense_correspondence.amplify_sequence: matrices 0 and 1 bit for bit, matrix 2 within the derived bound
2 gamma_n T (scipy sums its own unsorted rows there: tests/test_amplify.py).  Also rectangular products with empty rows, explicit
zeros and an exactly cancelling sum, the block-diagonal batch, the refusals and the dataset keyword end to end."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import amplify_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import _lib, datasets, kernels, operators  # noqa: E402
from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402
from surfacenetworks_amd.operators import SparseOperator, amplify_sequence_operators, laplacian_operator_from_mesh  # noqa: E402


def arrays(op):
    return op.rowptr.cpu().numpy(), op.colind.cpu().numpy(), op.vals.cpu().numpy()


def upload(A):
    """A csr_matrix as it is (explicit zeros kept, nothing re-sorted)."""
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(DEV)
    return SparseOperator(t(A.indptr, np.int32), t(A.indices, np.int32), t(A.data, np.float32), A.shape)


@pytest.mark.parametrize("kind,name", ac.GPU_CASES)
def test_sequence_against_emulation_and_host(kind, name):
    L = ac.laplacian(kind, name)
    ops = amplify_sequence_operators(upload(L))
    emu, scaled, dropped = ac.emulated_sequence(kind, name)
    host = dc.amplify_sequence(L)
    assert len(ops) == 3
    for t in range(3):
        assert ops[t].shape == L.shape and ops[t].batch == 1
        assert ac.same_csr(emu[t], *arrays(ops[t])), f"{kind}/{name}: matrix {t} differs from the definition"
    for t in range(2):
        H = host[t].copy()
        H.sort_indices()
        assert ac.same_csr(H, *arrays(ops[t])), f"{kind}/{name}: matrix {t} differs from scipy's"
    ratio, one_sided = ac.compare_within_bound(ops[2].to_scipy(), host[2], ac.product_bound(scaled[1], scaled[1]))
    print(f"{kind}/{name}: longest rows {[int(np.diff(arrays(o)[0]).max()) for o in ops]}, dropped zero sums {dropped}, matrix 2 "
          f"against scipy: worst {ratio:.3f} of the bound, {one_sided} one-sided entries")
    assert ratio <= 1.0 and one_sided <= 0.01 * emu[2].nnz
    if name == "flat":
        assert sum(dropped) >= 1                      # (the compaction phase ran)
    again = amplify_sequence_operators(upload(L))
    assert all(np.array_equal(a, b) for o, p in zip(ops, again) for a, b in zip(arrays(o), arrays(p)))


def _random_pair(seed, M, K, N, density):
    """A (M x K), B (K x N) with: empty rows in A (3) and in B (7, 8), an empty result row (A's row 9 meets only B's empty
    rows), a single-entry row (A's row 5), explicit zeros in both, and a sum that cancels exactly (A's row 11: x and -x against
    two rows of B holding the same y in column 2)."""
    rng = np.random.default_rng(seed)
    A = (rng.random((M, K)) < density) * rng.standard_normal((M, K))
    B = (rng.random((K, N)) < density) * rng.standard_normal((K, N))
    pa, pb = A != 0, B != 0
    A[3], pa[3] = 0, False
    B[7], pb[7] = 0, False
    B[8], pb[8] = 0, False
    A[9], pa[9] = 0, False
    A[9, [7, 8]], pa[9, [7, 8]] = [1.5, -2.0], True
    A[5], pa[5] = 0, False
    A[5, K - 1], pa[5, K - 1] = 0.75, True
    A[11], pa[11] = 0, False
    A[11, [4, 13]], pa[11, [4, 13]] = [1.2345, -1.2345], True
    B[4, 2] = B[13, 2] = 0.321
    pb[4, 2] = pb[13, 2] = True
    for X, P in ((A, pa), (B, pb)):                   # explicit zeros: stored entries whose value is 0
        r, c = np.nonzero(P)
        pick = rng.choice(r.size, 5, replace=False)
        pick = pick[~((X is A) & np.isin(r[pick], [5, 9, 11])) & ~((X is B) & np.isin(r[pick], [4, 13]) & (c[pick] == 2))]
        X[r[pick], c[pick]] = 0
    mk = lambda X, P: sp.csr_matrix((X[P].astype(np.float32), np.nonzero(P)[1].astype(np.int32),
                                     np.concatenate([[0], np.cumsum(P.sum(1))]).astype(np.int32)), shape=X.shape)
    return mk(A, pa), mk(B, pb)


def _wide_pair():
    """3 x 40 times 40 x 20011: one result row whose window covers 626 bitmap words, more than one per thread."""
    rng = np.random.default_rng(8)
    A = sp.random(3, 40, 0.4, random_state=rng, dtype=np.float32).tocsr()
    B = sp.random(40, 20011, 0.004, random_state=rng, dtype=np.float32).tolil()
    B[int(A[1].indices[0]), 0] = 1.0
    B[int(A[1].indices[0]), 20010] = -1.0
    A, B = A.tocsr(), B.tocsr().astype(np.float32)
    for X in (A, B):
        X.sort_indices()
    return A, B


PAIRS = {"37x53x29": lambda: _random_pair(1, 37, 53, 29, 0.15), "64x70x300": lambda: _random_pair(2, 64, 70, 300, 0.5),
         "3x40x20011": _wide_pair}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_rectangular_products_against_emulation(pair):
    A, B = PAIRS[pair]()
    full = ac.emulate_spgemm(A, B, keep_zeros=True)
    want = ac.drop_zeros(full)
    if pair != "3x40x20011":
        assert (A.data == 0).any() and (B.data == 0).any() and full.nnz > want.nnz
        assert full[11, 2] == 0 and 2 in full.indices[full.indptr[11]:full.indptr[12]] and np.diff(full.indptr)[[3, 9]].tolist() == [0, 0]
        assert np.diff(A.indptr)[5] == 1
    dA, dB = upload(A), upload(B)
    got = operators.spgemm(dA, dB)
    kept = operators.spgemm(dA, dB, keep_zeros=True)
    print(f"{pair}: {full.nnz} structural entries, {full.nnz - want.nnz} exact zeros, longest row {int(np.diff(full.indptr).max())}")
    assert got.shape == (A.shape[0], B.shape[1])
    assert ac.same_csr(want, *arrays(got)) and ac.same_csr(full, *arrays(kept))
    for other in (dA @ dB, dA.matmul(dB)):
        assert all(np.array_equal(a, b) for a, b in zip(arrays(got), arrays(other)))
    with pytest.raises(TypeError):
        dA.matmul(torch.zeros(B.shape[0], 4, device=DEV))
    with pytest.raises(ValueError, match="chain"):
        operators.spgemm(dA, dA)


def test_batch_equals_block_diagonal_of_single_meshes():
    V, F = ac.mesh("A")
    Vb = np.stack([V * np.array([1.0, 1.0, s]) for s in (1.0, 0.5, 2.0)]).astype(np.float32)
    Fd = torch.from_numpy(F.astype(np.int32)).to(DEV)
    Vd = torch.from_numpy(Vb).to(DEV)
    batch = amplify_sequence_operators(laplacian_operator_from_mesh(Vd, Fd))
    single = [amplify_sequence_operators(laplacian_operator_from_mesh(Vd[b], Fd)) for b in range(3)]
    nV = V.shape[0]
    for t in range(3):
        assert batch[t].batch == 3 and batch[t].shape == (3 * nV, 3 * nV)
        parts = [arrays(s[t]) for s in single]
        base = np.concatenate([[0], np.cumsum([p[0][-1] for p in parts])])
        rowptr = np.concatenate([[0]] + [p[0][1:] + base[b] for b, p in enumerate(parts)])
        colind = np.concatenate([p[1] + b * nV for b, p in enumerate(parts)])
        vals = np.concatenate([p[2] for p in parts])
        got = arrays(batch[t])
        assert np.array_equal(got[0], rowptr) and np.array_equal(got[1], colind)
        assert np.array_equal(got[2].view(np.int32), vals.view(np.int32))


def test_out_of_range_column_is_a_value_error():
    A, B = PAIRS["37x53x29"]()
    bad = A.copy()
    bad.indices[-1] = 53                              # one past A's last column: it would read B's row pointers out of bounds
    with pytest.raises(ValueError, match="column"):
        operators.spgemm(upload(bad), upload(B))
    badB = B.copy()
    badB.indices[badB.indptr[4]] = -1                 # (row 4 of B is read by A's row 11)
    with pytest.raises(ValueError, match="column"):
        operators.spgemm(upload(A), upload(badB))
    torch.cuda.synchronize()


def test_row_with_only_its_diagonal_is_a_value_error():
    L = ac.laplacian("ext", "A").tolil()
    L[5, :] = 0
    L[5, 5] = 1.0
    L = L.tocsr().astype(np.float32)
    L.eliminate_zeros()
    with pytest.raises(ValueError, match="off-diagonal"):
        amplify_sequence_operators(upload(L))


def test_row_wider_than_the_window_is_refused_and_nothing_is_written():
    W = kernels.spgemm_max_window()
    assert W == 131072
    A = sp.csr_matrix((np.ones(3, np.float32), np.array([0, 1, 0], np.int32), np.array([0, 2, 3], np.int32)), shape=(2, 2))
    B = sp.csr_matrix((np.ones(2, np.float32), np.array([0, W], np.int32), np.array([0, 1, 2], np.int32)), shape=(2, W + 1))
    dA, dB = upload(A), upload(B)
    with pytest.raises(RuntimeError, match="window"):
        operators.spgemm(dA, dB)
    # the same call through the C-ABI: the status bit is set and the row pointers keep the caller's bytes
    s_rowptr = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws_bytes = int(_lib.load().sn_csr_spgemm_workspace_bytes(2))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.call("sn_csr_spgemm_f32", p(dA.rowptr), p(dA.colind), p(dA.vals), p(dB.rowptr), p(dB.colind), p(dB.vals), 2, 2, W + 1, 0,
              p(s_rowptr), None, None, None, None, None, p(status), p(ws), ws_bytes, kernels._stream())
    assert int(status.item()) == kernels.SPGEMM_TOO_WIDE and s_rowptr.tolist() == [-7, -7, -7]
    # one column fewer fits: the widest row the kernels take
    B2 = sp.csr_matrix((np.ones(2, np.float32), np.array([0, W - 1], np.int32), np.array([0, 1, 2], np.int32)), shape=(2, W))
    got = operators.spgemm(dA, upload(B2))
    assert ac.same_csr(ac.emulate_spgemm(A, B2), *arrays(got))


def test_faust_frames_amplify_on_the_device_end_to_end():
    from helpers import deterministic_init

    V, F = ac.mesh("A")
    fr = datasets.faust_frame_from_mesh(V, F, device=DEV)
    with pytest.raises(ValueError, match="amplify"):
        dc.FaustFrames([fr], model="amp", pad_to=256, device=DEV, amplify="nonsense")
    host = dc.FaustFrames([fr], model="amp", pad_to=256, device=DEV)
    dev = dc.FaustFrames([fr], model="amp", pad_to=256, device=DEV, amplify="device")
    oh, od = host.sample(0)[3], dev.sample(0)[3]
    assert isinstance(od, dc.LSequence) and len(od) == 3
    for t in range(2):
        assert od[t].shape == (256, 256) and all(np.array_equal(a, b) for a, b in zip(arrays(oh[t]), arrays(od[t])))
    L = host.frames[0]["L"].astype(np.float32).tocsr()
    L.sort_indices()
    d = ac.inv_sqrt_degree(L)
    S2 = ac.emulate_scale(ac.emulate_spgemm(*(2 * [ac.emulate_scale(ac.emulate_scale(L, d), d)])), d)
    n = L.shape[0]
    ratio, one_sided = ac.compare_within_bound(od[2].to_scipy()[:n, :n], oh[2].to_scipy()[:n, :n], ac.product_bound(S2, S2))
    print(f"FaustFrames amp: operator 2 device against host: worst {ratio:.3f} of the bound, {one_sided} one-sided entries")
    assert ratio <= 1.0 and one_sided == 0 and od[2].nnz == oh[2].nnz
    model = deterministic_init(dc.SiameseModel("amp", 3), 7).to(DEV).train()
    inputs, _, mask, ops = dev.sample(0)
    out = model(dc._operation(ops, mask), dc._operation(ops, mask), inputs, inputs)
    assert out.shape == (1, 256, 256) and bool(torch.isfinite(out).all())
