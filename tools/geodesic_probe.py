"""Times the geodesic distance matrix of one FAUST-sized shape (torus_grid(65, 106): 6890 vertices, 41 340 directed edges / corners):
(a) `device`: the symmetric matrix on the GPU from resident (V, F) — operators.geodesic_matrix_from_mesh end to end, a host clock
    around calls that end in the read of the flag word, after --warmup calls; and the kernels alone between device events.
    --method edges: Laplacian pattern, edge lengths, sn_graph_apsp_f32, sn_symmetrize_min_f32;  --method triangles: corner table
    (sn_mesh_corners_f32), Eikonal sweeps (sn_mesh_geodesics_f32), sn_symmetrize_min_f32;  --method both: one after the other in
    the same run, plus how the two matrices compare.
(b) `host` (with the edges method): scipy.sparse.csgraph.dijkstra (float64, one core) on the same box for --host-sources evenly
    spaced sources, SCALED to all n sources by n / host_sources (every source costs the same on this graph: the scaling is
    stated in the output).
Also: the sources per workgroup (S) and workgroup size the dispatcher chose, and the sweeps per workgroup (min / median / max).
Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def measure(method, Vd, Fd, S, a):
    """End-to-end call times and per-kernel device times of one method; returns (result dict, G, the edge graph or None)."""
    from surfacenetworks_amd import kernels, operators

    nv = Vd.shape[0]
    for _ in range(a.warmup):
        G = operators.geodesic_matrix_from_mesh(Vd, Fd, method=method)
    torch.cuda.synchronize()
    whole = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        G = operators.geodesic_matrix_from_mesh(Vd, Fd, method=method)       # ends in the flag's .item(): the device has finished
        whole.append((time.perf_counter() - t0) * 1e3)
    out = torch.empty(nv, nv, device=Vd.device)
    sweeps = torch.zeros(-(-nv // S), dtype=torch.int32, device=Vd.device)
    graph = None
    if method == "edges":
        rowptr, colind, _ = kernels.laplacian_from_mesh(Vd, Fd)
        names = ("edge_lengths", "apsp", "symmetrize")
    else:
        names = ("corners", "sweeps", "symmetrize")
    parts = {k: [] for k in names}
    for _ in range(a.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        if method == "edges":
            w = kernels.edge_lengths_csr(Vd, rowptr, colind)
            ev[1].record()
            kernels.graph_apsp(rowptr, colind, w, nv, out=out, sweeps=sweeps)
            graph = (rowptr, colind, w)
        else:
            corners, _ = kernels._mesh_corner_table(Vd, Fd)                   # (no flag read between the events)
            ev[1].record()
            kernels.mesh_geodesics(corners, nv, out=out, sweeps=sweeps)
        ev[2].record()
        kernels.symmetrize_min_(out)
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(names):
            parts[name].append(ev[k].elapsed_time(ev[k + 1]))
    if method == "edges":
        assert torch.equal(out, G)                                            # bit-reproducible; the triangles method is not
    sw = sweeps.cpu().numpy()
    res = {"workgroups": int(sw.size), "sweeps_min": int(sw.min()), "sweeps_median": float(np.median(sw)), "sweeps_max": int(sw.max()),
           "device_ms": {"median": round(statistics.median(whole), 3), "min": round(min(whole), 3), "max": round(max(whole), 3),
                         "reps": a.reps},
           "kernel_ms": {k: round(statistics.median(v), 3) for k, v in parts.items()}}
    return res, G, graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--m", type=int, default=106)
    ap.add_argument("--permute", action="store_true", help="random vertex numbering (what a scan looks like)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-sources", type=int, default=256)
    ap.add_argument("--method", choices=("edges", "triangles", "both"), default="edges")
    a = ap.parse_args()

    from surfacenetworks_amd import _lib, mesh_ops

    dev = "cuda"
    V, F = mesh_ops.torus_grid(a.n, a.m, np.random.default_rng(4), permute=a.permute)
    nv = V.shape[0]
    Vd = torch.from_numpy(V.astype(np.float32)).to(dev)
    Fd = torch.from_numpy(F.astype(np.int32)).to(dev)
    lib = _lib.load()
    S, threads = int(lib.sn_graph_apsp_group(nv)), int(lib.sn_graph_apsp_threads(nv))
    res = {"vertices": nv, "faces": int(F.shape[0]), "permuted": bool(a.permute), "S": S, "threads": threads,
           "device": torch.cuda.get_device_name(0), "hip": torch.version.hip}
    G = {}
    for method in (("edges", "triangles") if a.method == "both" else (a.method,)):
        res[method], G[method], graph = measure(method, Vd, Fd, S, a)
        if method == "edges":
            res[method].update(host_dijkstra(graph, G[method], nv, a.host_sources, res[method]["device_ms"]["median"]))
    if a.method == "both":
        E, T = G["edges"], G["triangles"]
        off = ~torch.eye(nv, dtype=torch.bool, device=dev)
        res["triangles_vs_edges"] = {"never_above": bool((T <= E).all()), "strictly_below": round(float((T < E)[off].float().mean()), 4),
                                     "mean_ratio": round(float((T[off].double() / E[off].double()).mean()), 4),
                                     "min_ratio": round(float((T[off] / E[off]).min()), 4),
                                     "time_ratio": round(res["triangles"]["device_ms"]["median"] / res["edges"]["device_ms"]["median"], 2)}
    print(json.dumps(res))


def host_dijkstra(graph, G, nv, host_sources, dev_ms):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra

    rowptr, colind, w = graph
    rp, ci = rowptr.cpu().numpy(), colind.cpu().numpy()
    rows = np.repeat(np.arange(nv), np.diff(rp))
    off = rows != ci
    A = sp.csr_matrix((w.cpu().numpy()[off].astype(np.float64), (ci[off], rows[off])), shape=(nv, nv))
    src = np.linspace(0, nv - 1, min(host_sources, nv)).astype(np.int64)
    t0 = time.perf_counter()
    D64 = dijkstra(A, directed=True, indices=src)
    host_part = time.perf_counter() - t0
    host_ms = host_part * 1e3 * nv / len(src)
    Gh = G[torch.from_numpy(src).to(G.device)].cpu().numpy().astype(np.float64)
    return {"directed_edges": int(off.sum()), "host_scipy_ms_scaled": round(host_ms, 1),
            "host_scaling": f"{len(src)} sources took {host_part * 1e3:.1f} ms, times {nv}/{len(src)}",
            "host_over_device": round(host_ms / dev_ms, 1),
            "max_rel_diff_to_float64": float(np.max(np.abs(Gh - D64)[D64 > 0] / D64[D64 > 0]))}


if __name__ == "__main__":
    main()
