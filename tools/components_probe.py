"""Times of the mesh clean-up (LABNOTES.md#components): operators.clean_mesh on the device against mesh_ops.largest_component
(numpy) on the same machine's host, at three sizes: the 65 x 106 torus of TorusBodies (6890 vertices) with a small second
component, a ~100k-face torus with one, and a soup of 5000 separate triangles; vertex ids and face order shuffled.  The mesh is
resident on the device before the clock starts; a device call ends in its own read-back (a device synchronise); host and device
alternate inside one loop after a warm-up, the device side as `--inner` consecutive calls per sample, and the median and the
spread of `--reps` samples are printed per call.  Also checks that both sides return the same mesh, bit for bit.

    python tools/components_probe.py [--reps 30] [--inner 20] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfacenetworks_amd import mesh_ops  # noqa: E402
from surfacenetworks_amd.operators import clean_mesh  # noqa: E402


def joined(parts, seed):
    """The parts as one mesh, vertex ids and face order under a seeded permutation."""
    off, Vs, Fs = 0, [], []
    for V, F in parts:
        Vs.append(V)
        Fs.append(F + off)
        off += len(V)
    V, F = np.concatenate(Vs), np.concatenate(Fs)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(V))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return V[perm].astype(np.float32), inv[F][rng.permutation(len(F))].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_probe needs the GPU: there is no other path to time")
    rng = np.random.default_rng
    cases = {
        "torus 65x106 + grid 9x9": joined([mesh_ops.torus_grid(65, 106, rng(1)), mesh_ops.grid_cloth(9, 9, rng(2))], 3),
        "torus 224x224 + grid 20x20": joined([mesh_ops.torus_grid(224, 224, rng(4)), mesh_ops.grid_cloth(20, 20, rng(5))], 6),
        "soup of 5000 triangles": joined([(rng(7).random((15000, 3)), np.arange(15000).reshape(5000, 3))], 8),
    }
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "cases": {}}
    ms = lambda x: {"median_ms": round(1e3 * float(np.median(x)), 4), "min_ms": round(1e3 * float(np.min(x)), 4),
                    "max_ms": round(1e3 * float(np.max(x)), 4)}
    for name, (V, F) in cases.items():
        Vd, Fd = torch.from_numpy(V).to("cuda"), torch.from_numpy(F).to("cuda")
        Vh, Fh, Jh, Sh = mesh_ops.largest_component(V, F)           # warm-up of both sides, and the comparison
        cm = clean_mesh(Vd, Fd)
        same = bool(cm.V.cpu().numpy().tobytes() == Vh.tobytes() and np.array_equal(cm.F.cpu().numpy(), Fh)
                    and np.array_equal(cm.vertex_map.cpu().numpy(), Jh) and np.array_equal(cm.face_map.cpu().numpy(), Sh))
        th, td = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mesh_ops.largest_component(V, F)
            t1 = time.perf_counter()
            for _ in range(args.inner):
                clean_mesh(Vd, Fd)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            th.append(t1 - t0)
            td.append((t2 - t1) / args.inner)
        result["cases"][name] = {"vertices": int(V.shape[0]), "faces": int(F.shape[0]), "components": cm.components,
                                 "kept_vertices": int(cm.V.shape[0]), "kept_faces": int(cm.F.shape[0]),
                                 "host_numpy": ms(th), "device_resident_per_call": ms(td), "same_mesh_bit_for_bit": same}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
