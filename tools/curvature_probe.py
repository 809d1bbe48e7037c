"""Times of the principal curvatures (LABNOTES.md#curvature): operators.principal_curvatures with every output on the device
against mesh_ops.principal_curvatures (numpy) on the same machine's host, at radius 2 and 5, on the 65 x 106 torus of TorusBodies
(6890 vertices) and on a (64, 5041, 3) batch of 71 x 71 cloths sharing one face list.  Every (case, radius) is a step of its own:
a fresh child process under its own `timeout`, and the first step that fails ends the probe — nothing more is started on the
device after it.  Inside a step the mesh is resident on the device before the clock starts; the device call is timed with device
events around the whole launch sequence (allocations included), after a warm-up, as the median of `--reps` calls; the host
statement with perf_counter (`--host-reps` calls, one for the batch).  Every step also checks that the device outputs are the
host statement's, bit for bit.

    python tools/curvature_probe.py [--reps 20] [--host-reps 2] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("torus 65x106", "cloth 71x71, batch of 64")
RADII = (2, 5)
STEP_SECONDS = {"torus 65x106": 120, "cloth 71x71, batch of 64": 300}      # the host statement of the batch takes most of it
FIELDS = ("k1", "k2", "d1", "d2", "ring_size")


def make_case(name):
    from surfacenetworks_amd import mesh_ops

    rng = np.random.default_rng
    if name == CASES[0]:
        V, F = mesh_ops.torus_grid(65, 106, rng(1))
        return V.astype(np.float32), F.astype(np.int32)
    cloths = [mesh_ops.grid_cloth(71, 71, rng(10 + b)) for b in range(64)]
    return np.stack([V for V, _ in cloths]).astype(np.float32), cloths[0][1].astype(np.int32)


def step(name, radius, reps, host_reps):
    """One (case, radius) on the device and on the host; prints one JSON line."""
    import torch

    from surfacenetworks_amd import _lib, mesh_ops
    from surfacenetworks_amd.operators import principal_curvatures

    if not torch.cuda.is_available():
        raise SystemExit("curvature_probe needs the GPU: there is no other path to time")
    V, F = make_case(name)
    B = V.shape[0] if V.ndim == 3 else 1
    nV, nF = V.shape[-2], F.shape[0]
    Vd, Fd = torch.from_numpy(V).to("cuda"), torch.from_numpy(F).to("cuda")
    got = principal_curvatures(Vd, Fd, radius)                                  # warm-up and the comparison
    for _ in range(3):
        principal_curvatures(Vd, Fd, radius)
    torch.cuda.synchronize()
    td = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        principal_curvatures(Vd, Fd, radius)
        b.record()
        b.synchronize()
        td.append(a.elapsed_time(b))
    status = int(got.status.item())
    got = {f: getattr(got, f).cpu().numpy().reshape(B * nV, -1) for f in FIELDS}
    del Vd, Fd
    Vh = V.reshape(-1, 3)                                                       # the batch as one disjoint mesh, as the device lays it out
    Fh = (F[None].astype(np.int64) + nV * np.arange(B)[:, None, None]).reshape(-1, 3)
    th = []
    for _ in range(1 if B > 1 else host_reps):
        t0 = time.perf_counter()
        want = mesh_ops.principal_curvatures(Vh, Fh, radius)
        th.append(1e3 * (time.perf_counter() - t0))
    same = all(got[f].tobytes() == getattr(want, f).tobytes() for f in FIELDS) and status == want.status
    ms = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "max_ms": round(float(np.max(x)), 4)}
    ring = want.ring_size
    print(json.dumps({"case": name, "radius": radius, "meshes": B, "vertices": B * nV, "faces": B * nF, "host_numpy": ms(th),
                      "device_events": ms(td), "status": status, "ring_size": [int(ring.min()), float(ring.mean()), int(ring.max())],
                      "failed_vertices": int(np.isnan(want.k1).sum()), "bit_for_bit": bool(same),
                      "workspace_bytes": int(_lib.load().sn_mesh_curvature_workspace_bytes(B * nV, B * nF)),
                      "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, metavar=("CASE", "RADIUS"), default=None, help="run one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(args.step[0], int(args.step[1]), args.reps, args.host_reps)
    result = {"reps": args.reps, "host_reps": args.host_reps, "steps": []}
    for name in CASES:
        for radius in RADII:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS[name]), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                   "--host-reps", str(args.host_reps), "--step", name, str(radius)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if done.returncode != 0:
                raise SystemExit(f"curvature_probe: step {name!r} radius {radius} ended with status {done.returncode}; stopping here")
            line = done.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            result["steps"].append(json.loads(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
