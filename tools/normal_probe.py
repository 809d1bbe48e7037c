"""Times the normal-prediction step (surfacenetworks_amd/normal_predict.py) on N jittered tori or cloths: ms per training step
launched eagerly without launch plans, with them, and replayed from a hipGraph; and the loss alone — forward + backward of the
squared-cosine loss with its metric — as the one-pass kernels (sn_normal_cosine_*) and as the plain-torch statement
(loss_reference + mad_reference + autograd) on the same device tensors, the two ALTERNATING inside one run.  Device events
around every repetition after --warmup; medians with min / max.  The loss kernel's bytes are what the definition moves: per row
16 of g (pitch 4) and 4 of the mask twice (the count launch and the pass); per row of the mask 16 of y, 12 of the target and 12
of the frame; both legs are rated by these bytes over their time (an effective rate: the time includes torch's autograd and
launch overhead, so it is no kernel bandwidth).  Both loss legs enter through the (B, V, 3) view of a pitch-4 tensor, so both pay torch's backward of that slice.
`python tools/normal_probe.py --meshes 4 --shape torus --n 65 --m 106 --model lap`; prints one JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(run, warmup, reps):
    times = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return times


def _stats(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=4)
    ap.add_argument("--shape", choices=["torus", "cloth"], default="torus")
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--m", type=int, default=106)
    ap.add_argument("--model", choices=["lap", "dir", "avg"], default="lap")
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normal_probe measures on the GPU; there is none here")
    from surfacenetworks_amd import mesh_ops, plans
    from surfacenetworks_amd import normal_predict as NP

    dev = "cuda"
    rng = np.random.default_rng(a.seed)
    make = mesh_ops.torus_grid if a.shape == "torus" else mesh_ops.grid_cloth
    ds = NP.NormalFrames.from_meshes([make(a.n, a.m, rng) for _ in range(a.meshes)], model="dir" if a.model == "dir" else "lap", device=dev)
    batch = ds.sample_batch(a.meshes, ids=np.arange(ds.n))
    torch.manual_seed(a.seed)
    build = {"lap": lambda: NP.LapDeepModel(3, 3, layers=a.layers), "dir": lambda: NP.DirDeepModel(3, 3, layers=a.layers),
             "avg": lambda: NP.AvgModel(3, 3, a.layers)}[a.model]
    out = {"model": a.model, "layers": a.layers, "meshes": ds.n, "rows": int(batch.inputs.shape[0] * batch.inputs.shape[1]),
           "real_rows": int(batch.mask.sum()), "steps": a.steps, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip}
    # ---- the step: eager without plans, eager with plans, graphed
    for name in ("eager", "planned", "graphed"):
        plans.set_enabled(name != "eager")
        model = build().to(dev).train()
        opt = NP.make_optimizer(model)
        if name == "graphed":
            step = NP.graphed_train_step(model, opt, batch)
            run = lambda: step(batch)
        else:
            run = lambda: NP.train_step(model, opt, batch)
        out[name] = _stats(_timed(run, a.warmup, a.steps))
    plans.set_enabled(True)
    # ---- the loss alone, kernels and torch statement alternating
    rows = out["rows"]
    g = torch.Generator().manual_seed(a.seed)
    y4 = torch.randn(batch.inputs.shape[0], batch.inputs.shape[1], 4, generator=g).to(dev).requires_grad_(True)
    frame = batch.inputs[:, :, :3]

    def kernel_leg():
        loss, _ = NP.loss_and_mad(y4[:, :, :3], batch.mask, batch.targets, frame=frame)
        torch.autograd.grad(loss, y4)

    def torch_leg():
        o = y4[:, :, :3] + frame
        loss = NP.loss_reference(o, batch.mask, batch.targets)
        with torch.no_grad():
            NP.mad_reference(o, batch.mask, batch.targets)
        torch.autograd.grad(loss, y4)

    tk, tt = [], []
    for i in range(a.warmup + a.steps):
        k_, t_ = _timed(kernel_leg, 0, 1), _timed(torch_leg, 0, 1)
        if i >= a.warmup:
            tk += k_
            tt += t_
    nbytes = rows * (16 + 4 + 4) + out["real_rows"] * (16 + 12 + 12)      # every row: g, the mask twice; rows of the mask: y, target, frame
    out["loss_kernels"] = dict(_stats(tk), bytes=nbytes, gb_per_s=round(nbytes / statistics.median(tk) / 1e6, 2))
    # (the same bytes — what the definition needs — over the torch statement's time: its own traffic is several times that)
    out["loss_torch"] = dict(_stats(tt), bytes=nbytes, gb_per_s=round(nbytes / statistics.median(tt) / 1e6, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
