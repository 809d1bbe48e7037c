"""Shared by tests/test_intrinsic.py (host) and tests/test_intrinsic_gpu.py (device): the named meshes, the edge multiset of a
Delta-complex, and the two spread constants the device bounds are built from."""
import functools

import numpy as np

from surfacenetworks_amd import mesh_ops

# The host function's own spread between flip orders (fifo, lifo, three random seeds), the largest over the meshes below as
# tests/test_intrinsic.py measures and asserts it: 1.8e-14 relative in the lengths (mesh D), 1.1e-13 of the row maximum in
# the fp64 Laplacian (mesh F_disc).  The constants are the next power of ten above; the device gets 64 x that, and both products
# stay below 1e-9 — five orders under the 1e-4-and-up error of a wrong or missed flip.
SPREAD_L = 1e-13
SPREAD_LAP = 1e-12
DEVICE_FACTOR = 64
assert DEVICE_FACTOR * SPREAD_L < 1e-9 and DEVICE_FACTOR * SPREAD_LAP < 1e-9

ORDERS = (("fifo", 0), ("lifo", 0), ("random", 0), ("random", 1), ("random", 2))


def _f32(V):
    return np.asarray(V, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (V, F): V already rounded to fp32 (what the device reads), every mesh under 500 faces."""
    rng = np.random.default_rng
    out = {}
    VA, FA = mesh_ops.grid_cloth(13, 17, rng(5))
    out["A"] = (VA, FA)                                            # 384 faces, 93 flips
    out["B"] = (VA * np.array([1.0, 1.0, 6.0]), FA)                # 300 flips; one vertex pair carrying two edges
    out["C"] = mesh_ops.torus_grid(12, 20, rng(5), jitter=0.8)     # closed; the flip count depends on the schedule
    VD, FD = mesh_ops.grid_cloth(9, 9, rng(3))
    VD = VD.copy()
    VD[40, 2] += 2.0
    out["D"] = (VD, FD)                                            # a self-edge and a double edge
    VE, FE = mesh_ops.delaunay_disc(150, rng(5))
    out["E"] = (VE * np.array([1.0, 1.0, 8.0]), FE)                # 288 faces, not a multiple of 64
    r7 = rng(7)                                                    # the three meshes() of tests/test_geodesics.py
    out["F_disc"] = mesh_ops.delaunay_disc(150, r7)
    out["F_torus"] = mesh_ops.torus_grid(9, 14, r7)
    out["F_cloth"] = mesh_ops.grid_cloth(12, 9, r7, permute=True)
    out = {k: (_f32(V), np.asarray(F, np.int64)) for k, (V, F) in out.items()}
    for V, F in out.values():
        V.setflags(write=False)
        F.setflags(write=False)
    return out


NAMES = ("A", "B", "C", "D", "E", "F_disc", "F_torus", "F_cloth")


def flat_disc():
    """delaunay_disc(150, default_rng(5)) with z = 0: a planar Delaunay triangulation, so nothing flips.  (As generated the
    disc carries a height field and two of its edges are non-Delaunay in 3-D, cot sums -5.5e-2 and -1.2e-3.)"""
    V, F = mesh_ops.delaunay_disc(150, np.random.default_rng(5))
    return _f32(V * np.array([1.0, 1.0, 0.0])), np.asarray(F, np.int64)


def sorted_sides(Fp, l):
    """Every face side as (smaller vertex, larger vertex, length), sorted: the edge multiset of a Delta-complex (an interior
    edge appears twice, once per side; self-edges and multiple edges included) with the lengths matched by sorted edge."""
    Fp, l = np.asarray(Fp, np.int64), np.asarray(l, np.float64)
    a = np.concatenate([Fp[:, 0], Fp[:, 1], Fp[:, 2]])
    b = np.concatenate([Fp[:, 1], Fp[:, 2], Fp[:, 0]])
    ln = np.concatenate([l[:, 0], l[:, 1], l[:, 2]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    o = np.lexsort((ln, hi, lo))
    return np.stack([lo[o], hi[o]], 1), ln[o]


@functools.lru_cache(maxsize=None)
def host_state(name, order="fifo", seed=0):
    """(F', l', G, flips) of the host function, computed once per (mesh, order) and shared read-only."""
    V, F = meshes()[name] if name != "flat" else flat_disc()
    Fp, l, G, flips = mesh_ops._intrinsic_state(V, F, order, seed)
    for x in (Fp, l, G):
        x.setflags(write=False)
    return Fp, l, G, flips


@functools.lru_cache(maxsize=None)
def host_laplacian(name, order="fifo", seed=0):
    Fp, l, _, _ = host_state(name, order, seed)
    V, _ = meshes()[name] if name != "flat" else flat_disc()
    return mesh_ops.intrinsic_laplacian_from_lengths(Fp, l, V.shape[0])
