"""Times of the mesh descriptors (LABNOTES.md#descriptors): operators.vertex_descriptors with every output on the device against
mesh_ops.vertex_descriptors (numpy) on the same machine's host, on the 65 x 106 torus of TorusBodies (6890 vertices) and on a
(64, 5041, 3) batch of 71 x 71 cloths sharing one face list.  The mesh is resident on the device before the clock starts.  The
device call is timed with device events around the whole launch sequence (allocations included), after a warm-up, as the median
of `--reps` calls; the host statement with perf_counter as the median of `--host-reps`.  Also checks that the outputs built from
+ - * / sqrt alone are the host statement's, bit for bit.  --lib times another build of the library (a kernel variant).

    python tools/descriptor_probe.py [--reps 30] [--host-reps 3] [--lib PATH] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfacenetworks_amd import _lib, mesh_ops  # noqa: E402

EXACT = ("face_area", "face_normal", "n_area", "n_uniform", "mass_bary", "mass_voronoi", "mean")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("descriptor_probe needs the GPU: there is no other path to time")
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from surfacenetworks_amd.operators import vertex_descriptors

    rng = np.random.default_rng
    Vt, Ft = mesh_ops.torus_grid(65, 106, rng(1))
    cloths = [mesh_ops.grid_cloth(71, 71, rng(10 + b)) for b in range(64)]
    cases = {
        "torus 65x106": (Vt.astype(np.float32), Ft.astype(np.int32)),
        "cloth 71x71, batch of 64": (np.stack([V for V, _ in cloths]).astype(np.float32), cloths[0][1].astype(np.int32)),
    }
    result = {"device": torch.cuda.get_device_name(0), "library": _lib.LIB_PATH if args.lib else "in-tree", "reps": args.reps,
              "host_reps": args.host_reps, "cases": {}}
    ms = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "max_ms": round(float(np.max(x)), 4)}
    for name, (V, F) in cases.items():
        Vd, Fd = torch.from_numpy(V).to("cuda"), torch.from_numpy(F).to("cuda")
        B = V.shape[0] if V.ndim == 3 else 1
        nV, nF = V.shape[-2], F.shape[0]
        Vh = V.reshape(-1, 3)                                       # the batch as one disjoint mesh, as the device lays it out
        Fh = (F[None].astype(np.int64) + nV * np.arange(B)[:, None, None]).reshape(-1, 3)
        th = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = mesh_ops.vertex_descriptors(Vh, Fh)
            th.append(1e3 * (time.perf_counter() - t0))
        got = vertex_descriptors(Vd, Fd)                            # warm-up and the comparison
        same = all(getattr(got, f).cpu().numpy().tobytes() == getattr(want, f).tobytes() for f in EXACT)
        for _ in range(5):
            vertex_descriptors(Vd, Fd)
        torch.cuda.synchronize()
        td = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            vertex_descriptors(Vd, Fd)
            b.record()
            b.synchronize()
            td.append(a.elapsed_time(b))
        result["cases"][name] = {"meshes": B, "vertices": B * nV, "faces": B * nF, "host_numpy": ms(th), "device_events": ms(td),
                                 "status": int(got.status.item()), "exact_outputs_bit_for_bit": bool(same),
                                 "workspace_bytes": int(_lib.load().sn_mesh_descriptors_workspace_bytes(B * nV, B * nF))}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
