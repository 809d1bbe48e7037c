"""Times of the 'amp' tower's operator sequence (LABNOTES.md#spgemm): operators.amplify_sequence_operators on the device against
dense_correspondence.amplify_sequence (scipy) on the same machine's host, for one 65 x 106 torus (6890 vertices) and for a
block-diagonal batch of 8.  The device call ends in a device synchronise (it reads sizes back between phases anyway), the host
call is timed by the same clock; both alternate inside one loop after a warm-up, and the median and the spread of `--reps`
repetitions are printed.  Also prints the longest row and the widest column window of every result, and checks that the first
two device matrices equal the host's bit for bit.

    python tools/spgemm_probe.py [--reps 20] [--batch 8] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402
from surfacenetworks_amd import kernels, mesh_ops  # noqa: E402
from surfacenetworks_amd.operators import SparseOperator, amplify_sequence_operators  # noqa: E402


def shape_of(M):
    M = M.tocsr()
    M.sort_indices()
    rows = np.diff(M.indptr)
    first, last = M.indices[M.indptr[:-1][rows > 0]], M.indices[M.indptr[1:][rows > 0] - 1]
    return {"nnz": int(M.nnz), "longest_row": int(rows.max()), "widest_window": int((last - first + 1).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spgemm_probe needs the GPU: there is no other path to time")
    rng = np.random.default_rng(4)
    meshes = [mesh_ops.torus_grid(65, 106, rng) for _ in range(args.batch)]
    Ls = [mesh_ops.laplacian(V, F).astype(np.float32).tocsr() for V, F in meshes]
    cases = {"one torus": Ls[0], f"batch of {args.batch}": sp.block_diag(Ls, format="csr").astype(np.float32)}
    result = {"max_window": kernels.spgemm_max_window(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": {}}
    for name, L in cases.items():
        L.sort_indices()
        op = SparseOperator.from_scipy(L, "cuda")
        host = dc.amplify_sequence(L)
        dev = amplify_sequence_operators(op)                       # warm-up of both sides
        torch.cuda.synchronize()
        same = []
        for t in range(2):
            H = host[t].copy()
            H.sort_indices()
            D = dev[t].to_scipy()
            same.append(bool(np.array_equal(H.indptr, D.indptr) and np.array_equal(H.indices, D.indices)
                             and np.array_equal(H.data.view(np.int32), D.data.view(np.int32))))
        th, td, tu = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            dc.amplify_sequence(L)
            t1 = time.perf_counter()
            amplify_sequence_operators(op)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            up = SparseOperator.from_scipy(L, "cuda")
            seq = amplify_sequence_operators(up)
            back = [o.to_scipy() for o in seq]                     # what FaustFrames(amplify="device") does per frame
            t3 = time.perf_counter()
            th.append(t1 - t0)
            td.append(t2 - t1)
            tu.append(t3 - t2)
        ms = lambda x: {"median_ms": round(1e3 * float(np.median(x)), 3), "min_ms": round(1e3 * float(np.min(x)), 3),
                        "max_ms": round(1e3 * float(np.max(x)), 3)}
        result["cases"][name] = {"rows": int(L.shape[0]), "host_scipy": ms(th), "device_resident": ms(td),
                                 "device_upload_and_download": ms(tu), "matrices_0_1_bit_identical_to_host": same,
                                 "shapes": [shape_of(o.to_scipy()) for o in dev]}
        del back
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
