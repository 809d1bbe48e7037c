"""Times the geodesic distance matrix of one FAUST-sized shape (torus_grid(65, 106): 6890 vertices, 41 340 directed edges):
(a) `device`: the symmetric matrix on the GPU from resident (V, F) — operators.geodesic_matrix_from_mesh end to end (Laplacian
    pattern, edge lengths, sn_graph_apsp_f32, sn_symmetrize_min_f32, one read of the `unreached` flag), a host clock around
    calls that end in that read, after --warmup calls; and the three kernels alone between device events;
(b) `host`: scipy.sparse.csgraph.dijkstra (float64, one core) on the same box for --host-sources evenly spaced sources, SCALED
    to all n sources by n / host_sources (every source costs the same on this graph: the scaling is stated in the output).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--m", type=int, default=106)
    ap.add_argument("--permute", action="store_true", help="random vertex numbering (what a scan looks like)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-sources", type=int, default=256)
    a = ap.parse_args()
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra

    from surfacenetworks_amd import _lib, kernels, mesh_ops, operators

    dev = "cuda"
    V, F = mesh_ops.torus_grid(a.n, a.m, np.random.default_rng(4), permute=a.permute)
    nv = V.shape[0]
    Vd = torch.from_numpy(V.astype(np.float32)).to(dev)
    Fd = torch.from_numpy(F.astype(np.int32)).to(dev)
    lib = _lib.load()
    S, threads = int(lib.sn_graph_apsp_group(nv)), int(lib.sn_graph_apsp_threads(nv))

    for _ in range(a.warmup):
        G = operators.geodesic_matrix_from_mesh(Vd, Fd)
    torch.cuda.synchronize()
    whole = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        G = operators.geodesic_matrix_from_mesh(Vd, Fd)       # ends in unreached.item(): the device has finished
        whole.append((time.perf_counter() - t0) * 1e3)

    rowptr, colind, _ = kernels.laplacian_from_mesh(Vd, Fd)
    out = torch.empty(nv, nv, device=dev)
    sweeps = torch.zeros(-(-nv // S), dtype=torch.int32, device=dev)
    parts = {"edge_lengths": [], "apsp": [], "symmetrize": []}
    for _ in range(a.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        w = kernels.edge_lengths_csr(Vd, rowptr, colind)
        ev[1].record()
        kernels.graph_apsp(rowptr, colind, w, nv, out=out, sweeps=sweeps)
        ev[2].record()
        kernels.symmetrize_min_(out)
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(parts):
            parts[name].append(ev[k].elapsed_time(ev[k + 1]))
    assert torch.equal(out, G)
    sw = sweeps.cpu().numpy()

    rp, ci = rowptr.cpu().numpy(), colind.cpu().numpy()
    rows = np.repeat(np.arange(nv), np.diff(rp))
    off = rows != ci
    A = sp.csr_matrix((w.cpu().numpy()[off].astype(np.float64), (ci[off], rows[off])), shape=(nv, nv))
    src = np.linspace(0, nv - 1, min(a.host_sources, nv)).astype(np.int64)
    t0 = time.perf_counter()
    D64 = dijkstra(A, directed=True, indices=src)
    host_part = time.perf_counter() - t0
    host_ms = host_part * 1e3 * nv / len(src)
    Gh = G[torch.from_numpy(src).to(dev)].cpu().numpy().astype(np.float64)
    dev_ms = statistics.median(whole)
    res = {"vertices": nv, "directed_edges": int(off.sum()), "permuted": bool(a.permute), "S": S, "threads": threads,
           "workgroups": int(sw.size), "sweeps_min": int(sw.min()), "sweeps_median": float(np.median(sw)), "sweeps_max": int(sw.max()),
           "device_ms": {"median": round(dev_ms, 3), "min": round(min(whole), 3), "max": round(max(whole), 3), "reps": a.reps},
           "kernel_ms": {k: round(statistics.median(v), 3) for k, v in parts.items()},
           "host_scipy_ms_scaled": round(host_ms, 1),
           "host_scaling": f"{len(src)} sources took {host_part * 1e3:.1f} ms, times {nv}/{len(src)}",
           "host_over_device": round(host_ms / dev_ms, 1),
           "max_rel_diff_to_float64": float(np.max(np.abs(Gh - D64)[D64 > 0] / D64[D64 > 0])),
           "device": torch.cuda.get_device_name(0), "hip": torch.version.hip}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
