"""Times what the cascade model adds (surfacenetworks_amd/cascade.py):

  pooling   the four sibling-pair kernels (sn_pool_max2_*, sn_unpool2_*) at (B, V, C) = (64, 5048, 128) against torch's
            MaxPool1d(2, 2) / F.interpolate(scale_factor=2) + add and their autograd backward on the same device tensors, the two
            ALTERNATING inside one run, every call on the next of --sets operand sets (8 x 0.25-0.33 GB read per call: an
            operand is long out of the 256 MB last-level cache when its turn comes again; the outputs are the allocator's, which
            may hand out the same block again); each rated by the bytes its definition moves (fp32: 3, 5, 5, 3 coarse-row volumes of a fine
            pair) over its time, and as a share of the 5.75 TB/s a trivial 2 : 1 kernel streams on these boxes (README);
  hierarchy operators.mesh_hierarchy of the 6890-vertex torus and the 71 x 71 cloth against the numpy statement
            mesh_ops.mesh_hierarchy on the same machine's host (wall clock; the device figure includes its read-backs);
  step      one replayed training step (graphed_train_step) of a --levels cascade on a NormalFrames(model="cas") batch of
            --meshes jittered tori against the same model with torch's pooling swapped in.

Device events around every sample (--inner calls each) after --warmup; medians of --samples with min / max.
`python tools/cascade_probe.py`; prints one JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))      # torch's pooling forms and the pair-aggregation levels: one statement, the tests'

import numpy as np  # noqa: E402
import torch  # noqa: E402

STREAM_TBS = 5.75      # what a trivial kernel streams at a 2 : 1 read : write mix on these boxes (README), the lower figure


def _sample(run, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def _alternate(legs, warmup, samples, inner):
    """{name: [ms per call]}: the legs take turns, sample by sample."""
    times = {k: [] for k in legs}
    for i in range(warmup + samples):
        for k, run in legs.items():
            t = _sample(run, inner)
            if i >= warmup:
                times[k].append(t)
    return times


def _stats(times, nbytes=None):
    med = statistics.median(times)
    out = {"median_ms": round(med, 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}
    if nbytes is not None:
        out.update(bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3), share_of_stream=round(nbytes / med / 1e9 / STREAM_TBS, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[64, 5048, 128], metavar=("B", "V", "C"))
    ap.add_argument("--meshes", type=int, default=4)
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--m", type=int, default=106)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cascade_probe measures on the GPU; there is none here")
    from surfacenetworks_amd import cascade, kernels, mesh_ops
    from surfacenetworks_amd import normal_predict as NP
    from surfacenetworks_amd.operators import SparseOperator
    from cascade_cases import torch_pool, torch_unpool_add

    dev = "cuda"
    out = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "samples": a.samples, "inner": a.inner}
    # ---- the pooling kernels against torch, alternating; every call takes the NEXT of --sets operand sets, so that an operand
    # comes round again only after sets x (its own size and its neighbours') have passed through the 256 MB last-level cache
    B, V, C = a.shape
    g = torch.Generator().manual_seed(a.seed)
    sets = []
    for _ in range(a.sets):
        fine = torch.randn(B, V, C, generator=g).to(dev).requires_grad_(True)
        coarse = torch.randn(B, V // 2, C, generator=g).to(dev).requires_grad_(True)
        sets.append(dict(fine=fine, coarse=coarse, gf=torch.randn(B, V, C, generator=g).to(dev),
                         gc=torch.randn(B, V // 2, C, generator=g).to(dev), yp=torch_pool(fine),
                         yu=torch_unpool_add(coarse, fine.detach())))
    unit = B * (V // 2) * C * 4                                     # bytes of one coarse tensor
    s0 = sets[0]
    with torch.no_grad():
        same = bool(torch.equal(kernels.pool_max2_fwd(s0["fine"]), s0["yp"]) and
                    torch.equal(kernels.unpool2_add_fwd(s0["coarse"], s0["fine"]), s0["yu"]) and
                    torch.equal(kernels.pool_max2_bwd(s0["fine"], s0["gc"]),
                                torch.autograd.grad(s0["yp"], s0["fine"], s0["gc"], retain_graph=True)[0]) and
                    torch.equal(kernels.unpool2_bwd(s0["gf"]), torch.autograd.grad(s0["yu"], s0["coarse"], s0["gf"], retain_graph=True)[0]))
    out["pooling"] = {"shape": [B, V, C], "sets": a.sets, "equal_to_torch": same}
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % len(sets)]

    legs = {
        "pool_max2_fwd": (3, lambda s: kernels.pool_max2_fwd(s["fine"].detach()), lambda s: torch_pool(s["fine"].detach())),
        "pool_max2_bwd": (5, lambda s: kernels.pool_max2_bwd(s["fine"].detach(), s["gc"]),
                          lambda s: torch.autograd.grad(s["yp"], s["fine"], s["gc"], retain_graph=True)),
        "unpool2_add_fwd": (5, lambda s: kernels.unpool2_add_fwd(s["coarse"].detach(), s["fine"].detach()),
                            lambda s: torch_unpool_add(s["coarse"].detach(), s["fine"].detach())),
        "unpool2_bwd": (3, lambda s: kernels.unpool2_bwd(s["gf"]),
                        lambda s: torch.autograd.grad(s["yu"], s["coarse"], s["gf"], retain_graph=True)),
    }
    for name, (units, mine, theirs) in legs.items():
        t = _alternate({"kernel": lambda: mine(nxt()), "torch": lambda: theirs(nxt())}, a.warmup, a.samples, a.inner)
        out["pooling"][name] = {"kernel": _stats(t["kernel"], units * unit), "torch": _stats(t["torch"], units * unit)}
    del sets, s0, fine, coarse
    # ---- hierarchy build: the device against the numpy statement on this machine's host (wall clock around a synchronise: the
    # build reads the cluster count of every level back)
    import time

    from surfacenetworks_amd import operators

    rng = np.random.default_rng(a.seed)
    out["hierarchy"] = {}
    for name, (Vv, Ff) in (("torus_65x106", mesh_ops.torus_grid(a.n, a.m, rng)), ("cloth_71x71", mesh_ops.grid_cloth(71, 71, rng))):
        Ls = mesh_ops.laplacian(Vv.astype(np.float64), Ff).astype(np.float32).tocsr()
        Ls.sort_indices()
        Ld = SparseOperator.from_scipy(Ls, dev)
        times = []
        for i in range(a.warmup + a.samples):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = operators.mesh_hierarchy(Ld, levels=a.levels)
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            hs = mesh_ops.mesh_hierarchy(Ls, levels=a.levels)
            host.append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(h.L[k].vals.cpu().numpy().view(np.uint32), hs.L[k].data.view(np.uint32)) and
                   np.array_equal(h.L[k].colind.cpu().numpy(), hs.L[k].indices) for k in range(a.levels))
        out["hierarchy"][name] = {"vertices": int(Vv.shape[0]), "sizes": h.sizes, "rounds": h.rounds, "singletons": h.singletons,
                                  "nodes_finest": int(h.real[-1].numel()), "equal_to_statement": bool(same),
                                  "device": _stats(times), "numpy_statement": _stats(host)}
    # ---- one replayed step on sampled batches (real hierarchies), kernels against torch's pooling
    rng = np.random.default_rng(a.seed)
    ds = NP.NormalFrames.from_meshes([mesh_ops.torus_grid(a.n, a.m, rng) for _ in range(a.meshes)], model="cas", device=dev,
                                     levels=a.levels)
    batch = ds.sample_batch(a.meshes, ids=np.arange(a.meshes))
    Laps = batch.Laps
    out["step"] = {"levels": a.levels, "meshes": a.meshes, "rows_per_level": [int(L.shape[0]) for L in Laps]}
    runs = {}
    for name in ("kernels", "torch_pooling"):
        torch.manual_seed(a.seed)
        model = cascade.LapCascade(3, 3, cascade_levels=a.levels).to(dev).train()
        if name == "torch_pooling":
            model.down_pool, model.up_pool_add = torch_pool, torch_unpool_add
        step = NP.graphed_train_step(model, NP.make_optimizer(model), batch)
        runs[name] = (lambda s=step: s(batch))
    t = _alternate(runs, a.warmup, a.samples, 1)
    out["step"].update({k: _stats(v) for k, v in t.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
