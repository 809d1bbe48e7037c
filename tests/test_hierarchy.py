"""The mesh hierarchy, host side (no GPU): the numpy statement mesh_ops.mesh_hierarchy on the cases of tests/hierarchy_cases.py.

Invariants of every coarsening: the matching is an involution on adjacent vertices and maximal; the coarse operator equals a dense
evaluation of the written formula bit for bit; positions and order are inverse, real[k-1] is the pairwise OR of real[k], fake rows
and columns are empty, the operators in position order are the level operators renumbered.  Row sums: a coarse row's sum is
bounded by (fine entries merged into it) x 2^-24 x (sum of their magnitudes) plus the fine rows' own sums scaled by r.  And two
conditions that keep "equal bit for bit" from being vacuous: per level at most a quarter of the nodes stay singletons, and at most
64 rounds are needed."""
import numpy as np
import pytest
import scipy.sparse as sp

import hierarchy_cases as hc
from surfacenetworks_amd import mesh_ops

NAMES = tuple(hc.cases())
DENSE_MAX = 400          # the dense evaluation of the formula is run where the operator has at most this many rows


def _chain(case, levels, mass_choice):
    """[(L_k, mate_k, parent_k, m_k, rounds_k)] for k = levels-1 .. 1 in LEVEL numbering, from the public pieces."""
    L = case["L"]
    m = np.ones(L.shape[0], np.float32) if mass_choice is None else case["mass"]
    out = []
    for _ in range(levels - 1):
        mate, rounds = mesh_ops.handshake_matching(L)
        Lc, mc, parent = mesh_ops.coarsen_operator(L, mate, m)
        out.append((L, mate, parent, m, rounds, Lc))
        L, m = Lc, mc
    return out


def _dense_formula(L, mate, parent, m):
    """L_c of the written definition on dense fp32 arrays (absent entries are +0: adding them changes no stored sum)."""
    n, nc = L.shape[0], int(parent.max()) + 1
    A = L.toarray().astype(np.float32)
    idx = np.arange(n)
    first = np.zeros(nc, np.int64)
    second = np.full(nc, -1, np.int64)
    reps = idx[(mate < 0) | (idx < mate)]
    first[parent[reps]] = reps
    second[parent[reps]] = mate[reps]
    two = second >= 0
    T = A[:, first].copy()
    T[:, two] = (A[:, first[two]] + A[:, second[two]]).astype(np.float32)                 # ascending j: first member, then second
    r = np.ones(n, np.float32)
    pr = mate >= 0
    r[pr] = (m[pr] / (m[pr] + m[mate[pr]]).astype(np.float32)).astype(np.float32)
    C = (r[first][:, None] * T[first]).astype(np.float32)
    C[two] = (C[two] + (r[second[two]][:, None] * T[second[two]]).astype(np.float32)).astype(np.float32)
    return C


@pytest.mark.parametrize("mass_choice", hc.MASSES)
@pytest.mark.parametrize("name", NAMES)
def test_matching_and_coarse_operator(name, mass_choice):
    case = hc.cases()[name]
    for L, mate, parent, m, rounds, Lc in _chain(case, 4, mass_choice):
        n = L.shape[0]
        idx = np.arange(n)
        s = mesh_ops.hierarchy_scores(L)
        row = np.repeat(idx, np.diff(L.indptr))
        col = L.indices
        S = sp.csr_matrix((s, (row, col)), shape=L.shape)
        assert abs(S - S.T).max() == 0                                        # s_ij and s_ji: the same bits
        p = np.flatnonzero(mate >= 0)
        assert np.array_equal(mate[mate[p]], p) and (mate[p] != p).all()      # an involution ...
        assert (np.asarray(S[p, mate[p]]).ravel() > 0).all()                  # ... on adjacent vertices with a positive score
        free = mate < 0
        assert not ((s > 0) & free[row] & free[col]).any()                    # maximal
        # clusters numbered by the rank of their smallest member
        rep = np.where((mate >= 0) & (mate < idx), mate, idx)
        assert np.array_equal(parent, np.searchsorted(np.unique(rep), rep))
        assert Lc.shape == (parent.max() + 1,) * 2 and Lc.dtype == np.float32 and Lc.has_sorted_indices and (Lc.data != 0).all()
        if n <= DENSE_MAX:
            want = _dense_formula(L, mate, parent, m)
            assert np.array_equal(Lc.toarray().view(np.uint32) & 0x7fffffff != 0, want != 0)
            assert np.array_equal(Lc.toarray()[want != 0].view(np.uint32), want[want != 0].view(np.uint32))
        # row sums: rounding of the merged entries plus the fine rows' own sums, scaled
        fine_sum = np.asarray(L.astype(np.float64).sum(1)).ravel()
        fine_abs = np.asarray(abs(L.astype(np.float64)).sum(1)).ravel()
        cnt = np.diff(L.indptr)
        r = np.ones(n)
        pr = mate >= 0
        r[pr] = m[pr].astype(np.float64) / (m[pr].astype(np.float64) + m[mate[pr]])
        nc = Lc.shape[0]
        bound = np.bincount(parent, cnt, nc) * 2.0 ** -24 * np.bincount(parent, fine_abs, nc) + np.bincount(parent, r * np.abs(fine_sum), nc)
        got = np.abs(np.asarray(Lc.astype(np.float64).sum(1)).ravel())
        assert (got <= bound + 1e-300).all(), float((got / (bound + 1e-300)).max())


@pytest.mark.parametrize("levels", hc.LEVELS)
@pytest.mark.parametrize("mass_choice", hc.MASSES)
@pytest.mark.parametrize("name", NAMES)
def test_positions_masks_and_operators_in_position_order(name, mass_choice, levels):
    case = hc.cases()[name]
    h = hc.statement(name, levels, mass_choice)
    n = case["L"].shape[0]
    B = 1 if case["blocks"] is None or levels == 1 else len(case["blocks"])
    assert len(h.L) == len(h.real) == levels and h.sizes[-1] == n
    n0 = h.L[0].shape[0]
    assert [M.shape[0] for M in h.L] == [n0 << k for k in range(levels)] and n0 % B == 0
    # order and position are inverse; the finest operator is the given one renumbered
    assert np.array_equal(h.order[h.position], np.arange(n)) and (h.order >= 0).sum() == n
    assert np.array_equal(h.real[-1], h.order >= 0)
    back = h.L[-1][h.position][:, h.position]
    assert abs(back - case["L"]).max() == 0 and back.nnz == case["L"].nnz
    for k in range(levels):
        M = h.L[k]
        assert M.dtype == np.float32 and M.has_sorted_indices and int(h.real[k].sum()) == h.sizes[k]
        fake = ~h.real[k]
        assert np.diff(M.indptr)[fake].sum() == 0 and not fake[M.indices].any()                # empty rows and columns
        if k > 0:
            assert np.array_equal(h.real[k - 1], h.real[k].reshape(-1, 2).any(1))
            assert not (h.real[k].reshape(-1, 2)[:, 1] & ~h.real[k].reshape(-1, 2)[:, 0]).any()      # a singleton takes slot 0
    if levels == 1:
        assert abs(h.L[0] - case["L"]).max() == 0 and np.array_equal(h.order, np.arange(n))
    # the level operators are those of the chain, renumbered: children of one parent are siblings in position order
    chain = _chain(case, levels, mass_choice)
    for k, (_, mate, parent, _, rounds, Lc) in zip(range(levels - 1, 0, -1), chain):
        assert h.rounds[k] == rounds and h.singletons[k] == int((mate < 0).sum())
        assert np.array_equal(h.mate[k], mate) and np.array_equal(h.parent[k], parent)
        at = h.positions[k - 1]
        assert np.array_equal(np.sort(at), np.flatnonzero(h.real[k - 1]))
        assert np.array_equal(h.positions[k], 2 * at[parent] + ((mate >= 0) & (mate < np.arange(len(mate)))))
        sub = h.L[k - 1][at][:, at]                                            # back in level numbering
        assert sub.shape == Lc.shape and abs(sub - Lc).max() == 0 and sub.nnz == Lc.nnz


@pytest.mark.parametrize("mass_choice", hc.MASSES)
@pytest.mark.parametrize("name", NAMES)
def test_few_singletons_and_few_rounds(name, mass_choice):
    """Per level: singletons <= 0.25 of the nodes, rounds <= 64.  (A prototype with a reciprocal multiply in the score gave
    singleton shares 0.018-0.122 and 2-8 rounds on these families.)"""
    h = hc.statement(name, 4, mass_choice)
    for k in range(3, 0, -1):
        share = h.singletons[k] / h.sizes[k]
        print(f"{name} mass={mass_choice} level {k}: {h.sizes[k]} nodes, singleton share {share:.3f}, rounds {h.rounds[k]}")
        assert share <= 0.25 and h.rounds[k] <= 64, (name, k, share, h.rounds[k])


def test_a_batch_equals_its_meshes_one_by_one():
    case = hc.cases()["batch_two_grids"]
    for mass_choice in hc.MASSES:
        h = hc.statement("batch_two_grids", 4, mass_choice)
        per = h.L[0].shape[0] // 2
        off = 0
        for b, part in enumerate(case["parts"]):
            hb = mesh_ops.mesh_hierarchy(part["L"], levels=4, mass=hc.mass_of(part, mass_choice))
            nb = part["L"].shape[0]
            for k in range(4):
                lo, hi = b * per << k, (b + 1) * per << k
                real = lo + np.flatnonzero(h.real[k][lo:hi])
                mine = np.flatnonzero(hb.real[k])
                assert len(real) == len(mine)
                assert np.array_equal((real - lo)[: len(mine)], mine)                      # the same positions inside the mesh
                a, c = h.L[k][real][:, real], hb.L[k][mine][:, mine]
                assert abs(a - c).max() == 0 and a.nnz == c.nnz
            assert np.array_equal(h.position[off:off + nb] - (b * per << 3), hb.position)
            off += nb
        # nothing crosses meshes on any level
        for k in range(4):
            M = h.L[k].tocoo()
            assert np.array_equal(M.row // (per << k), M.col // (per << k))


def test_pad_coarsest_to_and_refusals():
    case = hc.cases()["grid12"]
    h = mesh_ops.mesh_hierarchy(case["L"], levels=3, pad_coarsest_to=16)
    plain = hc.statement("grid12", 3, None)
    assert h.L[0].shape[0] % 16 == 0 and h.L[0].shape[0] >= plain.L[0].shape[0] and h.sizes == plain.sizes
    for k in range(3):
        real = np.flatnonzero(h.real[k])
        assert abs(h.L[k][real][:, real] - plain.L[k][np.flatnonzero(plain.real[k])][:, np.flatnonzero(plain.real[k])]).max() == 0
    assert plain.rounds[2] > 1
    with pytest.raises(RuntimeError, match="max_rounds"):
        mesh_ops.mesh_hierarchy(case["L"], levels=2, max_rounds=1)
    with pytest.raises(ValueError):
        mesh_ops.mesh_hierarchy(case["L"][:5], levels=2)
    with pytest.raises(ValueError):
        mesh_ops.mesh_hierarchy(case["L"], levels=2, blocks=[3, 4])


def test_isolated_vertex_and_zero_scores():
    """A vertex without a diagonal entry never proposes and is never chosen: it stays a singleton on every level."""
    case = hc.cases()["grid_isolated"]
    n = case["L"].shape[0]
    s = mesh_ops.hierarchy_scores(case["L"])
    assert s.dtype == np.float32 and (s >= 0).all()
    mate, _ = mesh_ops.handshake_matching(case["L"])
    assert mate[n - 1] == -1
    h = hc.statement("grid_isolated", 4, None)
    p = h.position[n - 1]
    assert all(np.diff(h.L[k].indptr)[p >> (3 - k)] == 0 for k in range(4))


def test_new_names_are_declared_bound_and_mirrored():
    import os
    import re

    from surfacenetworks_amd import _lib, constants, kernels

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = open(os.path.join(root, "include", "sn_spmm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    lib = _lib.load()
    for name in ("sn_mesh_match_workspace_bytes", "sn_mesh_match_f32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name in open(os.path.join(root, "INTEGRATION.md")).read(), name
    assert "Mesh hierarchy" in full
    for name, value in (("HIER_NOT_FINISHED", 1), ("HIER_BAD_COLUMN", 2), ("HIER_THREADS", 1024)):
        assert re.search(rf"#define SN_{name}\s+{value}\b", full) and getattr(constants, name) == value == getattr(kernels, name)
        assert getattr(mesh_ops, name) == value
    assert constants.status_names("hierarchy", 3) == ["NOT_FINISHED", "BAD_COLUMN"]
    assert int(lib.sn_mesh_match_workspace_bytes(10, 40)) >= 10 * 4 + 40 * 4 + 10 * 4
    assert lib.sn_mesh_match_f32(None, None, None, None, -1, 0, 4, None, None, None, None, None, 0, None) == -2      # SN_E_SHAPE
    assert lib.sn_mesh_match_f32(None, None, None, None, 3, 0, 4, None, None, None, None, None, 0, None) == -1       # SN_E_NULL
