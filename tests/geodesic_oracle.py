"""Host oracle of the geodesic (edge-path) distance matrices — test infrastructure, numpy + heapq only.

The definition (include/sn_spmm.h, "Geodesic distance matrices"): edge weight w = (float) sqrt((dx*dx + dy*dy) + dz*dz) in
fp64 from the fp32 coordinates; D[s][v] = the minimum over all edge paths of the length accumulated in fp32 from the source
outward, +inf without a path.  `dijkstra_f32` is the textbook algorithm with np.float32 additions; `sweep_fixed_point` is the
relaxation the device kernel runs, in a vertex order of the caller's choice."""
import heapq

import numpy as np


def edge_weights(V, rows, cols):
    """The edge-weight formula on index arrays: numpy rounds every product and sum on its own."""
    V32 = np.asarray(V).astype(np.float32)
    d = V32[rows].astype(np.float64) - V32[cols].astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def csr_rows(rowptr):
    rowptr = np.asarray(rowptr)
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def mesh_graph(V, F):
    """(rowptr, colind, w) of the vertex adjacency of a triangle mesh plus a zero self-loop per vertex, columns ascending:
    the pattern of the mass-normalised cotangent Laplacian when no cotangent weight cancels."""
    n = np.asarray(V).shape[0]
    F = np.asarray(F).astype(np.int64)
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2], F[:, 1], F[:, 2], F[:, 0], np.arange(n)])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0], F[:, 0], F[:, 1], F[:, 2], np.arange(n)])
    key = np.unique(a * n + b)
    rows, cols = key // n, key % n
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), edge_weights(V, rows, cols)


def out_edges(rowptr, colind, w):
    """Row v of the CSR lists the edges INTO v (an entry (v, u) is the edge u -> v: the device sweep pulls along its row).
    Returns, per vertex u, the list of (v, np.float32 weight) it reaches."""
    n = len(rowptr) - 1
    out = [[] for _ in range(n)]
    for v, u, x in zip(csr_rows(rowptr).tolist(), np.asarray(colind).tolist(), list(np.asarray(w, np.float32))):
        out[u].append((v, x))
    return out


def dijkstra_f32(out, s):
    """One row of D from the lists of out_edges: heap Dijkstra whose path lengths are np.float32 sums."""
    n = len(out)
    inf = np.float32(np.inf)
    d = [inf] * n
    d[s] = np.float32(0)
    done = [False] * n
    heap = [(d[s], s)]
    while heap:
        du, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v, x in out[u]:
            t = du + x                          # np.float32 + np.float32
            if t < d[v]:
                d[v] = t
                heapq.heappush(heap, (t, v))
    return np.array(d, np.float32)


def apsp_f32(rowptr, colind, w, sources=None):
    n = len(rowptr) - 1
    sources = range(n) if sources is None else sources
    edges = out_edges(rowptr, colind, w)
    out = np.empty((len(sources), n), np.float32)
    for k, s in enumerate(sources):
        out[k] = dijkstra_f32(edges, s)
    return out


def mesh_apsp(V, F, symmetric=False):
    D = apsp_f32(*mesh_graph(V, F))
    return np.minimum(D, D.T) if symmetric else D


def sweep_fixed_point(rowptr, colind, w, s, order):
    """d[v] = min(d[v], min_u fl(d[u] + w_uv)) over the vertices in `order`, in place, swept until nothing changes.
    Returns (d, number of sweeps including the last, unchanged one)."""
    n = len(rowptr) - 1
    inf = np.float32(np.inf)
    d = [inf] * n
    d[s] = np.float32(0)
    ws, ci, rp = list(np.asarray(w, np.float32)), np.asarray(colind).tolist(), np.asarray(rowptr).tolist()
    sweeps = 0
    while True:
        sweeps += 1
        changed = False
        for v in order:
            best = d[v]
            for e in range(rp[v], rp[v + 1]):
                t = d[ci[e]] + ws[e]
                if t < best:
                    best = t
            if best < d[v]:
                d[v] = best
                changed = True
        if not changed or sweeps > n:
            return np.array(d, np.float32), sweeps
