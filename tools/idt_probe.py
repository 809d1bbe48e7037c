"""Times the intrinsic Delaunay Laplacian of one FAUST-sized shape (torus_grid(65, 106, jitter=0.8): 6890 vertices, 13 780 faces):
(a) `intrinsic`: operators.laplacian_operator_from_mesh(V, F, intrinsic=True) end to end from resident (V, F), a host clock around
    calls that end in a device synchronise, after --warmup calls; and its stages between device events: the glue builder
    (sn_mesh_glue_i32), the flip rounds (sn_mesh_idt_rounds_f64, every round that found work and the idle one that ends the run,
    enqueued without the chunk reads), then the three phases of sn_mesh_idt_laplacian_f32 and the torch.sort between them.
(b) `extrinsic`: the device builder of the extrinsic operator on the same mesh, the same way.
(c) `host`: mesh_ops.intrinsic_laplacian (Python loops, one core) on the same box, once — the only alternative there was.
Also rounds, flips, flips per round, and the negative weights before and after.  Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def clocked(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "reps": reps}


def stages(Vd, Fd, rounds, reps):
    """Median device-event time of every stage; the rounds are enqueued in one go (their number is known from the run before)."""
    from surfacenetworks_amd import _lib, kernels
    from surfacenetworks_amd.kernels import _p, _stream

    lib = _lib.load()
    nV, nF = Vd.shape[0], Fd.shape[0]
    dev = Vd.device
    names = ("glue", "rounds", "contributions", "sort", "count", "fill")
    parts = {k: [] for k in names}
    N = int(lib.sn_mesh_idt_laplacian_items(nV, nF))
    wsr_b, wsl_b = int(lib.sn_mesh_idt_workspace_bytes(nF)), int(lib.sn_mesh_idt_laplacian_workspace_bytes(nV, nF))
    wsr = torch.empty(wsr_b, dtype=torch.uint8, device=dev)
    wsl = torch.empty(wsl_b, dtype=torch.uint8, device=dev)
    counters = torch.empty(rounds, 2, dtype=torch.int32, device=dev)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    rowptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        Fp = Fd.clone()
        ev[0].record()
        G, status, l = kernels.mesh_glue(Fd, nV, Vd)
        ev[1].record()
        _lib.call("sn_mesh_idt_rounds_f64", _p(Fp), _p(l), _p(G), nF, 0, rounds, rounds + 1, counters.data_ptr(), status.data_ptr(), _p(wsr),
                  wsr_b, _stream())
        ev[2].record()
        args = (_p(Fp), _p(l), nV, nF)
        _lib.call("sn_mesh_idt_laplacian_f32", *args, 0, _p(keys), None, None, None, None, None, _p(wsl), wsl_b, _stream())
        ev[3].record()
        skeys, order = torch.sort(keys)
        ev[4].record()
        _lib.call("sn_mesh_idt_laplacian_f32", *args, 1, _p(skeys), _p(order), rowptr.data_ptr(), None, None, None, _p(wsl), wsl_b, _stream())
        nnz = int(rowptr[-1].item())
        colind = torch.empty(nnz, dtype=torch.int32, device=dev)
        vals = torch.empty(nnz, dtype=torch.float32, device=dev)
        ev[5].record()
        _lib.call("sn_mesh_idt_laplacian_f32", *args, 2, _p(skeys), _p(order), rowptr.data_ptr(), _p(colind), _p(vals), None, _p(wsl), wsl_b,
                  _stream())
        ev[6].record()
        ev[6].synchronize()
        for k, name in enumerate(names):
            parts[name].append(ev[k].elapsed_time(ev[k + 1]))
    c = counters.cpu().numpy()
    out = {k: round(statistics.median(v), 3) for k, v in parts.items()}
    out["rounds_per_round"] = round(out["rounds"] / rounds, 4)
    return out, c, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--m", type=int, default=106)
    ap.add_argument("--jitter", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    from surfacenetworks_amd import kernels, mesh_ops, operators

    dev = "cuda"
    V, F = mesh_ops.torus_grid(a.n, a.m, np.random.default_rng(4), jitter=a.jitter)
    V = V.astype(np.float32)
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F.astype(np.int32)).to(dev)
    res = {"vertices": int(V.shape[0]), "faces": int(F.shape[0]), "jitter": a.jitter, "device": torch.cuda.get_device_name(0),
           "hip": torch.version.hip}
    L, res["intrinsic_ms"] = clocked(lambda: operators.laplacian_operator_from_mesh(Vd, Fd, intrinsic=True), a.warmup, a.reps)
    E, res["extrinsic_ms"] = clocked(lambda: operators.laplacian_operator_from_mesh(Vd, Fd), a.warmup, a.reps)
    state = kernels.intrinsic_delaunay(Vd, Fd)
    res.update({"status": state[3], "rounds": state[4], "flips": state[5], "chunk": kernels.IDT_CHUNK})
    res["stage_ms"], counters, vals = stages(Vd, Fd, state[4], a.reps)
    assert torch.equal(vals, L.vals)                                           # the staged run is the same run, bit for bit
    res["non_delaunay_per_round"] = counters[:, 0].tolist()
    res["flips_per_round"] = counters[:, 1].tolist()

    def positives(op):
        m = op.to_scipy().tocoo()
        return int(((m.row != m.col) & (m.data > 0)).sum())
    res["offdiag_positive"] = {"extrinsic": positives(E), "intrinsic": positives(L)}
    res["nnz"] = {"extrinsic": int(E.vals.numel()), "intrinsic": int(L.vals.numel())}
    res["max_row_entries"] = int((L.rowptr[1:] - L.rowptr[:-1]).max())
    if not a.no_host:
        t0 = time.perf_counter()
        H = mesh_ops.intrinsic_laplacian(V, F)
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["host_over_device"] = round(res["host_ms"] / res["intrinsic_ms"]["median"], 1)
        res["pattern_equal_host"] = bool(np.array_equal(H.indptr, L.rowptr.cpu().numpy()) and np.array_equal(H.indices, L.colind.cpu().numpy()))
        h32 = H.data.astype(np.float32)
        res["values_differing_from_host"] = int((h32 != L.vals.cpu().numpy()).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
