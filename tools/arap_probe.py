"""Times ARAP sequence generation (operators.arap_deform, arap.ClothSequences(dynamics="arap")) on one MI355X:
(a) `small`: the 34 x 33 cloth, 3 frames, one mesh — device time per CG iteration, from which the time limit of (b) was sized;
(b) `deform`: a pool of --sequences cloths of --grid x --grid vertices, --frames frames, as ONE arap_deform call (one workgroup per
    mesh), a host clock around the call (it ends in a read of the status), for every --chunk frames-per-launch value; the CG
    iterations per solve; the longest single launch between device events;
(c) `dataset`: arap.ClothSequences(...) with dynamics="arap" and with the default wave, end to end (the difference is (b) plus
    the transfers; the rest is the host's operator pools, the same for both);
(d) `host`: the scipy oracle of tests/test_arap_deform.py (SVD rotations, sparse LU) on ONE sequence of --host-frames frames on
    this box's host, SCALED to the pool — it is not run at full size.
Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=71)
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--chunk", type=int, nargs="+", default=[5])
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--skip-dataset", action="store_true")
    args = ap.parse_args()
    from surfacenetworks_amd import arap, kernels, mesh_ops, operators

    out = {"grid": args.grid, "sequences": args.sequences, "frames": args.frames}
    # (a)
    V, F = mesh_ops.grid_cloth(34, 33, np.random.default_rng(13))
    h, H = mesh_ops.arap_handle_motion(V, 3, np.random.default_rng(113))
    operators.arap_deform(V, F, h, H)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = operators.arap_deform(V, F, h, H)
    its = int(r.cg_iters.sum())
    out["small"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "cg_iterations": its,
                    "us_per_cg_iteration": round((time.perf_counter() - t0) * 1e6 / max(its, 1), 2)}
    # (b)
    rng = np.random.default_rng(3)
    meshes = []
    for _ in range(args.sequences):
        V, F = mesh_ops.grid_cloth(args.grid, args.grid, rng)
        meshes.append((V.astype(np.float32), F.astype(np.int32)) + mesh_ops.arap_handle_motion(V, args.frames, rng))
    batch = [torch.from_numpy(np.stack([m[k] for m in meshes])).cuda() for k in range(4)]
    out["deform"] = {}
    default_chunk = kernels.ARAP_FRAMES_PER_LAUNCH
    for chunk in args.chunk:
        kernels.ARAP_FRAMES_PER_LAUNCH = chunk
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = operators.arap_deform(*batch)
        sec = time.perf_counter() - t0
        it = r.cg_iters.double()
        moving = it[:, 1:]                                   # frame 0 is the rest pose: its solves start converged
        out["deform"][str(chunk)] = {"seconds": round(sec, 3), "launches": -(-args.frames // chunk),
                                     "seconds_per_launch": round(sec / -(-args.frames // chunk), 4),
                                     "cg_per_solve_mean": round(float(moving.mean()), 1), "cg_per_solve_min": int(moving.min()),
                                     "cg_per_solve_max": int(moving.max()), "status": sorted(set(r.status.tolist()))}
    kernels.ARAP_FRAMES_PER_LAUNCH = default_chunk
    # (d)
    from test_arap_deform import oracle_frames

    V, F, h, H = meshes[0]
    t0 = time.perf_counter()
    want = oracle_frames(V, F, h, H[: args.host_frames], 2)
    sec = time.perf_counter() - t0
    out["host"] = {"frames": args.host_frames, "seconds": round(sec, 2),
                   "scaled_to_pool_seconds": round(sec / args.host_frames * args.frames * args.sequences, 1),
                   "max_abs_diff_to_device_fp32": float(np.abs(want - r.frames[0, : args.host_frames].cpu().numpy()).max())}
    # (c)
    if not args.skip_dataset:
        for dyn in ("arap", "wave"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arap.ClothSequences([(args.grid, args.grid)] * args.sequences, frames=args.frames, dynamics=dyn)
            torch.cuda.synchronize()
            out.setdefault("dataset", {})[dyn] = round(time.perf_counter() - t0, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
