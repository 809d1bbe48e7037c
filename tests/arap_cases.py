"""The ARAP cases shared by tests/test_arap_deform.py (host) and tests/test_arap_deform_gpu.py (device), and their host results,
computed once per process by the numpy statement (mesh_ops.arap_*) and handed out read-only."""
import collections
import functools

import numpy as np

from surfacenetworks_amd import mesh_ops

Case = collections.namedtuple("Case", "name V F handles H voff hoff iters tol max_cg")

NAMES = ("cloth5x5", "cloth9x7", "flat_inplane", "octahedron", "cloth34x33", "ragged_pair", "no_handle_component", "capped")
ORACLE_NAMES = ("cloth5x5", "cloth9x7", "octahedron")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _cloth(n, m, seed, frames):
    V, F = mesh_ops.grid_cloth(n, m, np.random.default_rng(seed))
    V = V.astype(np.float32)
    handles, H = mesh_ops.arap_handle_motion(V, frames, np.random.default_rng(seed + 100))
    return V, F.astype(np.int32), handles, H


def _single(name, V, F, handles, H, iters=2, tol=1e-10, max_cg=4096):
    voff = np.array([0, V.shape[0]], np.int32)
    hoff = np.array([0, handles.size], np.int32)
    return Case(name, *_frozen(V, F, handles, H, voff, hoff), iters, tol, max_cg)


def _union(name, parts, **kw):
    V = np.concatenate([p[0] for p in parts])
    voff = np.cumsum([0] + [p[0].shape[0] for p in parts]).astype(np.int32)
    hoff = np.cumsum([0] + [p[2].size for p in parts]).astype(np.int32)
    F = np.concatenate([p[1] + voff[b] for b, p in enumerate(parts)]).astype(np.int32)
    handles = np.concatenate([p[2] + voff[b] for b, p in enumerate(parts)]).astype(np.int32)
    H = np.concatenate([p[3] for p in parts], axis=1)
    c = _single(name, V, F, handles, H, **kw)
    return c._replace(voff=_frozen(voff)[0], hoff=_frozen(hoff)[0])


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name == "cloth5x5":
        return _single(name, *_cloth(5, 5, 11, 6))
    if name == "cloth9x7":
        return _single(name, *_cloth(9, 7, 12, 6))
    if name == "capped":
        return _single(name, *_cloth(9, 7, 12, 6), max_cg=3)
    if name == "cloth34x33":
        return _single(name, *_cloth(34, 33, 13, 3))
    if name == "flat_inplane":
        V, F, handles, _ = _cloth(5, 5, 11, 6)
        V = V.copy()
        V[:, 2] = 0.0
        held = handles[V[handles, 0] < 0.5 * V[:, 0].max()]
        c = V[np.setdiff1d(handles, held)].astype(np.float64).mean(axis=0)
        H = np.zeros((6, handles.size, 3))
        for t in range(6):
            a = 0.05 * t
            Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
            moved = c + (V[handles].astype(np.float64) - c) @ Rz.T + np.array([0.01, -0.004, 0.0]) * t
            H[t] = np.where(np.isin(handles, held)[:, None], V[handles], moved)
        H = H.astype(np.float32)
        assert not H[:, :, 2].any()
        return _single(name, V, F, handles, H)
    if name == "octahedron":
        V = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
        V = V + 0.05 * np.random.default_rng(14).standard_normal(V.shape).astype(np.float32)
        F = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [5, 2, 1], [5, 3, 2], [5, 4, 3], [5, 1, 4]], np.int32)
        handles = np.array([2], np.int32)
        H = (V[2][None, None, :] + np.arange(4, dtype=np.float32)[:, None, None] * np.array([0.03, -0.02, 0.05], np.float32))
        return _single(name, V, F, handles, H.astype(np.float32))
    if name == "ragged_pair":
        return _union(name, [_cloth(5, 5, 11, 6), _cloth(9, 7, 12, 6)])
    if name == "no_handle_component":      # two disjoint cloths as ONE mesh, handles on the first only
        a, b = _cloth(5, 5, 11, 2), _cloth(5, 5, 15, 2)
        V = np.concatenate([a[0], b[0] + np.float32(2.0)])
        F = np.concatenate([a[1], b[1] + 25]).astype(np.int32)
        return _single(name, V, F, a[2], a[3], max_cg=48)
    raise KeyError(name)


def meshes(c: Case):
    """The meshes of a case as single-mesh cases: (V, F, handles, H) with local indices."""
    out = []
    for b in range(c.voff.size - 1):
        v0, v1, h0, h1 = c.voff[b], c.voff[b + 1], c.hoff[b], c.hoff[b + 1]
        sel = (c.F[:, 0] >= v0) & (c.F[:, 0] < v1)
        out.append((c.V[v0:v1], c.F[sel] - v0, c.handles[h0:h1] - v0, c.H[:, h0:h1]))
    return out


@functools.lru_cache(maxsize=None)
def host_weights(name: str):
    c = case(name)
    return mesh_ops.arap_weights(c.V, c.F)


@functools.lru_cache(maxsize=None)
def host_result(name: str):
    """One mesh_ops.ArapResult per mesh of the case."""
    c = case(name)
    return tuple(mesh_ops.arap_deform(V, F, h, H, c.iters, c.tol, c.max_cg) for V, F, h, H in meshes(c))
