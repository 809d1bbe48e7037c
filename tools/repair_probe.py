"""Times of the mesh repair (LABNOTES.md#repair): operators.repair_mesh on the device against mesh_ops.repair_mesh (numpy) on
the same machine's host, at two sizes: the 65 x 106 torus of TorusBodies (6890 vertices) and a 224 x 224 torus (100352 faces),
each as a triangle soup — every face on three vertices of its own — with half its faces turned and vertex ids and face order
shuffled.  The mesh is resident on the device before the clock starts; a device call ends in its own read-back (a device
synchronise); host and device alternate inside one loop after a warm-up, the device side as `--inner` consecutive calls per
sample, and the median and the range of `--reps` samples are printed per call.  Also checks that both sides return the same
mesh, bit for bit.

    python tools/repair_probe.py [--reps 20] [--inner 10] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfacenetworks_amd import mesh_ops  # noqa: E402
from surfacenetworks_amd.operators import repair_mesh  # noqa: E402


def soup(V, F, seed):
    """Every face on its own three vertices, half of the faces stored as (a, c, b), ids and order under seeded permutations."""
    rng = np.random.default_rng(seed)
    Vs = V.astype(np.float32)[F.ravel()]
    Fs = np.arange(F.size).reshape(-1, 3)
    perm = rng.permutation(len(Vs))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    Fs = inv[Fs][rng.permutation(len(Fs))]
    turn = rng.random(len(Fs)) < 0.5
    Fs[turn] = Fs[turn][:, [0, 2, 1]]
    return Vs[perm], Fs.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("repair_probe needs the GPU: there is no other path to time")
    rng = np.random.default_rng
    cases = {
        "torus 65x106 as a soup": soup(*mesh_ops.torus_grid(65, 106, rng(1)), 2),
        "torus 224x224 as a soup": soup(*mesh_ops.torus_grid(224, 224, rng(3)), 4),
    }
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "cases": {}}
    ms = lambda x: {"median_ms": round(1e3 * float(np.median(x)), 4), "min_ms": round(1e3 * float(np.min(x)), 4),
                    "max_ms": round(1e3 * float(np.max(x)), 4)}
    fields = ("V", "F", "vertex_map", "vertex_index", "face_map", "flipped")
    for name, (V, F) in cases.items():
        Vd, Fd = torch.from_numpy(V).to("cuda"), torch.from_numpy(F).to("cuda")
        host = mesh_ops.repair_mesh(V, F)                            # warm-up of both sides, and the comparison
        dev = repair_mesh(Vd, Fd)
        same = all(getattr(dev, k).cpu().numpy().tobytes() == np.ascontiguousarray(getattr(host, k)).tobytes() for k in fields)
        same = bool(same and tuple(dev[6:]) == tuple(host[6:]))
        th, td = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mesh_ops.repair_mesh(V, F)
            t1 = time.perf_counter()
            for _ in range(args.inner):
                repair_mesh(Vd, Fd)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            th.append(t1 - t0)
            td.append((t2 - t1) / args.inner)
        result["cases"][name] = {"vertices": int(V.shape[0]), "faces": int(F.shape[0]), "kept_vertices": int(dev.V.shape[0]),
                                 "kept_faces": int(dev.F.shape[0]), "welded_vertices": dev.welded_vertices,
                                 "flipped_faces": int(dev.flipped.sum()), "classes": dev.classes, "host_numpy": ms(th),
                                 "device_resident_per_call": ms(td), "same_mesh_bit_for_bit": same}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
