"""Mesh clean-up, host side (no GPU): mesh_ops.components against scipy's connected components on graphs built here,
mesh_ops.largest_component against a literal numpy rendering of the reference's script
(src/dense_correspondence/largest_component.py:28-47), the invariants of compact, and what the cases are meant to hold.
Every comparison is an exact integer or bitwise one."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import components_cases as cases
from surfacenetworks_amd import mesh_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _good(F, nV):
    F = F.astype(np.int64)
    return ((F >= 0) & (F < nV)).all(1) & (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])


def _to_minima(lab):
    """scipy's component numbers -> the smallest member of every component."""
    mins = np.full(lab.max() + 1 if lab.size else 0, np.iinfo(np.int64).max)
    np.minimum.at(mins, lab, np.arange(lab.size))
    return mins[lab]


def oracle_vertex(F, nV):
    """vlabel by scipy on the vertex graph of the good faces."""
    Fg = F[_good(F, nV)].astype(np.int64)
    a = np.concatenate([Fg[:, 0], Fg[:, 1], Fg[:, 2]])
    b = np.concatenate([Fg[:, 1], Fg[:, 2], Fg[:, 0]])
    A = sp.coo_matrix((np.ones(a.size), (a, b)), shape=(nV, nV)).tocsr()
    return _to_minima(connected_components(A, directed=False)[1])


def oracle_edge(F, nV):
    """flabel by scipy on the face graph: faces x edges incidence B from the sorted edge keys, components of B B^T."""
    good = _good(F, nV)
    fid = np.nonzero(good)[0]
    Fg = F[good].astype(np.int64)
    ends = np.sort(np.stack([Fg, np.roll(Fg, -1, axis=1)], axis=2).reshape(-1, 2), axis=1)       # (3 nFg, 2), face-major
    _, edge = np.unique(ends[:, 0] * max(nV, 1) + ends[:, 1], return_inverse=True)
    B = sp.coo_matrix((np.ones(edge.size), (np.repeat(fid, 3), edge.ravel())), shape=(F.shape[0], int(edge.max()) + 1 if edge.size else 1))
    lab = _to_minima(connected_components((B @ B.T).tocsr(), directed=False)[1])
    lab[~good] = -1
    return lab


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_components_match_scipy(name, mode):
    c = cases.case(name)
    nV, nF = c.V.shape[0], c.F.shape[0]
    cc = cases.host_components(name, mode)
    good = _good(c.F, nV)
    if mode == "vertex":
        vl = oracle_vertex(c.F, nV)
        assert cc.vlabel.dtype == np.int32 and np.array_equal(cc.vlabel, vl)
        fl = np.where(good, vl[np.clip(c.F[:, 0], 0, nV - 1)], -1)      # (clipped: a bad face's index is never looked at)
        n = nV
    else:
        assert cc.vlabel is None
        fl = oracle_edge(c.F, nV)
        n = nF
    assert cc.flabel.dtype == np.int32 and np.array_equal(cc.flabel, fl)
    count = np.bincount(fl[good], minlength=n)
    assert cc.count.dtype == np.int32 and np.array_equal(cc.count, count)
    if good.any():
        best = count.max()
        want = [np.count_nonzero(count), int(np.nonzero(count == best)[0].min()), best]
    else:
        want = [0, -1, 0]
    assert cc.summary.tolist() == want
    assert cc.status == (0 if good.all() else mesh_ops.CC_BAD_FACE)


def reference_largest_component(V, F):
    """largest_component.py:28-47 step by step on a mesh without bad faces: component ids in the order of their first face
    (facet_components), the smallest id among the most frequent (stats.mode), the kept faces sliced out (igl.slice), the
    vertices in use renumbered ascending (igl.remove_unreferenced)."""
    lab = oracle_edge(F, V.shape[0])
    _, first = np.unique(lab, return_index=True)
    ids = np.empty(lab.max() + 1, np.int64)
    ids[lab[np.sort(first)]] = np.arange(first.size)
    C = ids[lab]
    modeC = int(np.bincount(C).argmax())
    Fid = np.where(C == modeC)[0]
    Fk = F[Fid]
    J = np.unique(Fk)
    return V[J], np.searchsorted(J, Fk), J, Fid


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in cases.NO_FACE])
def test_largest_component_is_the_reference_script(name):
    c = cases.case(name)
    good = _good(c.F, c.V.shape[0])
    src = np.nonzero(good)[0]                              # the script knows no bad faces: it sees the good ones, in order
    Vw, Fw, Jw, Fidw = reference_largest_component(c.V, c.F[good])
    Vg, Fg, Jg, Fsrcg = mesh_ops.largest_component(c.V, c.F, "edge")
    assert Vg.dtype == np.float32 and Vg.tobytes() == Vw.tobytes()
    assert np.array_equal(Fg, Fw) and np.array_equal(Jg, Jw) and np.array_equal(Fsrcg, src[Fidw])


@pytest.mark.parametrize("name", cases.NO_FACE)
def test_largest_component_without_faces_raises(name):
    c = cases.case(name)
    with pytest.raises(ValueError, match="no face"):
        mesh_ops.largest_component(c.V, c.F)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_compact_invariants(name, mode):
    c = cases.case(name)
    nV = c.V.shape[0]
    keep = cases.winner_mask(name, mode)
    out = mesh_ops.compact(c.V, c.F, keep)
    I, J, Fsrc = out.I.astype(np.int64), out.J.astype(np.int64), out.Fsrc.astype(np.int64)
    assert out.sizes.tolist() == [len(J), len(Fsrc)] and I.shape == (nV,)
    assert (np.diff(J) > 0).all() and (np.diff(Fsrc) > 0).all()
    kept = np.nonzero(I >= 0)[0]
    assert np.array_equal(kept, J) and np.array_equal(I[J], np.arange(len(J)))
    assert out.Vnew[I[kept]].tobytes() == c.V[kept].tobytes()
    assert np.array_equal(Fsrc, np.nonzero(keep.astype(bool) & _good(c.F, nV))[0])
    assert np.array_equal(out.Fnew, I[c.F[Fsrc].astype(np.int64)])
    assert out.Fnew.size == 0 or (out.Fnew.min() >= 0 and np.array_equal(np.unique(out.Fnew), np.arange(len(J))))
    nov = mesh_ops.compact(None, c.F, keep, num_vertices=nV)
    assert nov.Vnew is None and all(np.array_equal(a, b) for a, b in zip(nov[:4], out[:4]))


def test_cases_hold_what_they_are_meant_to():
    comps = {(n, m): cases.host_components(n, m) for n in cases.NAMES for m in cases.MODES}
    ncomp = {k: int(v.summary[0]) for k, v in comps.items()}
    assert cases.case("strip").V.shape[0] == 6002 and cases.case("strip").F.shape[0] == 6000
    for n in ("strip", "strip_reversed", "strip_permuted", "fin"):
        assert ncomp[n, "edge"] == ncomp[n, "vertex"] == 1
    for n in ("bowtie", "bowtie_tets"):
        assert ncomp[n, "vertex"] == 1 and ncomp[n, "edge"] == 2
    assert ncomp["two_grids", "edge"] == 2 and ncomp["junk", "edge"] == 3 and ncomp["soup", "edge"] == ncomp["soup", "vertex"] == 5000
    # tie: the same count twice; the vertex-mode winner is block 0, the edge-mode winner block 1
    tie = cases.case("tie")
    for mode, block in (("vertex", 0), ("edge", 1)):
        cc = comps["tie", mode]
        assert sorted(cc.count[cc.count > 0].tolist()) == [128, 128]
        assert set(tie.face_block[cc.flabel == cc.summary[1]].tolist()) == {block}
    # junk: unused vertices at both ends, all three kinds of bad face
    junk = cases.case("junk")
    nV = junk.V.shape[0]
    used = np.zeros(nV, bool)
    used[junk.F[_good(junk.F, nV)].ravel()] = True
    assert not used[0] and not used[-1]
    bad = junk.F[~_good(junk.F, nV)]
    assert (bad == -1).any() and (bad == nV).any() and ((bad[:, 0] == bad[:, 1]) | (bad[:, 0] == bad[:, 2])).any()
    # the scans: soup passes one tile, big passes the top level's 256 tiles in both scans of the compaction
    assert cases.case("soup").F.shape[0] + 1 > cases.SCAN_TILE
    big = cases.case("big")
    assert min(big.V.shape[0], big.F.shape[0]) + 1 > cases.SCAN_TOP
    assert (cases.BIG_TORUS - 1) ** 2 + 1 <= cases.SCAN_TOP < cases.BIG_TORUS ** 2      # no smaller square torus does on its own
    out = mesh_ops.compact(big.V, big.F, cases.winner_mask("big", "edge"))
    assert out.sizes[0] > cases.SCAN_TOP and out.sizes[0] < big.V.shape[0]


@pytest.mark.parametrize("name", ["two_grids", "junk"])
def test_largest_component_is_the_block_it_was_built_from(name):
    c = cases.case(name)
    Vw, Fw, Jw, Fsrcw = cases.expected_part(name, 0)
    assert len(Jw) == 144 and len(Fsrcw) == 242                        # the grid_cloth(12, 12)
    Vg, Fg, Jg, Fsrcg = mesh_ops.largest_component(c.V, c.F)
    assert Vg.tobytes() == Vw.tobytes() and np.array_equal(Fg, Fw) and np.array_equal(Jg, Jw) and np.array_equal(Fsrcg, Fsrcw)


def test_header_ctypes_and_plan_table_agree_on_the_new_symbols():
    from surfacenetworks_amd import _lib

    header = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    for name in ("sn_mesh_components_workspace_bytes", "sn_mesh_components_i32", "sn_mesh_label_mask_i32",
                 "sn_mesh_compact_workspace_bytes", "sn_mesh_compact_i32"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
        assert (f"SN_PLAN_FN({name})" in table) == (not name.endswith("_bytes"))
    for macro, value in (("SN_CC_EDGE", 0), ("SN_CC_VERTEX", 1), ("SN_CC_BAD_FACE", mesh_ops.CC_BAD_FACE),
                         ("SN_CC_INTERNAL", mesh_ops.CC_INTERNAL)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", header)
