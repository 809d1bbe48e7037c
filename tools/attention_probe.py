"""Times what graph attention adds (surfacenetworks_amd/attention.py over csrc/sn_attention.hip):

  propagate  attn_propagate forward and backward at (B x V, C) = (64 x 5041, 128), H = 8, on the Laplacian pattern of the ARAP grid
             batch (64 cloths of 71 x 71 vertices, block-diagonal), next to functional.lap_propagate on the same operator — its
             forward moves nearly the same bytes (x in, the (rows, 2C) buffer out, the gathered rows from cache): the floor — and
             to the torch-operation statement attention.attn_propagate_reference on the same device tensors.  The legs ALTERNATE
             inside one run and every call takes the next of --sets operand sets.  Forward: the call under no_grad; backward:
             torch.autograd.grad of a kept forward, both halves of the output carrying a gradient.  Each leg is also rated by
             the bytes its definition must move (forward 3, backward 4 volumes of a (rows, C) fp32 matrix: x in and two halves out;
             two gradient halves and e in, dx out) as a share of the 5.75 TB/s a trivial 2 : 1 kernel streams on these boxes (README).
  step       one replayed training step (graphed_train_step) of attention.LapGatModel on a NormalFrames(model="lap") batch of
             --meshes jittered 6890-vertex tori next to normal_predict.LapDeepModel's on the same batch, alternating.

Device events around every sample (--inner calls each) after --warmup; medians of --samples with min / max.
`python tools/attention_probe.py`; prints one JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--grid", type=int, default=71)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--meshes", type=int, default=4)
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--m", type=int, default=106)
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_probe measures on the GPU; there is none here")
    from surfacenetworks_amd import attention, mesh_ops
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd import normal_predict as NP
    from surfacenetworks_amd.operators import OperatorPool

    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "samples": a.samples, "inner": a.inner}
    # ---- the propagate, three forms on one operator
    rng = np.random.default_rng(a.seed)
    V, F_ = mesh_ops.grid_cloth(a.grid, a.grid, rng)
    L1 = mesh_ops.mesh_operators(V, F_)["L"].tocsr()
    nv = L1.shape[0]
    op = OperatorPool([L1], dev).assemble(np.zeros(a.batch, dtype=np.int64), nv, nv)
    op.t()
    rows, C, H = a.batch * nv, a.channels, a.heads
    g = torch.Generator().manual_seed(a.seed)
    att = (0.3 * torch.randn(2, C, generator=g)).to(dev).requires_grad_(True)
    sets = []
    for _ in range(a.sets):
        x = torch.randn(rows, C, generator=g).to(dev).requires_grad_(True)
        sets.append(dict(x=x, g=torch.randn(rows, 2 * C, generator=g).to(dev), attn=attention.attn_propagate(op, x, att, H),
                         lap=snF.lap_propagate(op, x)))
    s0 = sets[0]
    want = attention.attn_propagate_reference(op, s0["x"], att, H)
    gw = torch.autograd.grad(want, (s0["x"], att), s0["g"])
    gm = torch.autograd.grad(s0["attn"], (s0["x"], att), s0["g"], retain_graph=True)
    out["propagate"] = {"rows": rows, "channels": C, "heads": H, "nnz": int(op.colind.numel()), "sets": a.sets,
                        "max_abs_diff_to_torch_statement": {"p": float((s0["attn"] - want).abs().max()),
                                                            "dx": float((gm[0] - gw[0]).abs().max()),
                                                            "da": float((gm[1] - gw[1]).abs().max())}}
    del want, gw, gm
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % len(sets)]

    unit = rows * C * 4
    with torch.no_grad():
        fwd = _alternate({"attn": lambda: attention.attn_propagate(op, nxt()["x"], att, H),
                          "lap": lambda: snF.lap_propagate(op, nxt()["x"]),
                          "torch_statement": lambda: attention.attn_propagate_reference(op, nxt()["x"], att, H)},
                         a.warmup, a.samples, a.inner)

    def grad_of(key, wrt_a):
        s = nxt()
        return torch.autograd.grad(s[key], (s["x"], att) if wrt_a else (s["x"],), s["g"], retain_graph=True)

    def torch_fwd_bwd():
        s = nxt()
        return torch.autograd.grad(attention.attn_propagate_reference(op, s["x"], att, H), (s["x"], att), s["g"])

    bwd = _alternate({"attn": lambda: grad_of("attn", True), "lap": lambda: grad_of("lap", False)}, a.warmup, a.samples, a.inner)
    both = _alternate({"torch_statement_fwd_bwd": torch_fwd_bwd}, 1, max(3, a.samples // 4), 1)
    out["propagate"]["forward"] = {k: _stats(v, 3 * unit) for k, v in fwd.items()}
    out["propagate"]["backward"] = {k: _stats(v, 4 * unit) for k, v in bwd.items()}
    out["propagate"]["forward_and_backward"] = {k: _stats(v) for k, v in both.items()}
    med = lambda v: statistics.median(v)
    out["propagate"]["attn_over_lap"] = {"forward": round(med(fwd["attn"]) / med(fwd["lap"]), 3),
                                         "backward": round(med(bwd["attn"]) / med(bwd["lap"]), 3)}
    out["propagate"]["torch_statement_over_attn"] = {
        "forward": round(med(fwd["torch_statement"]) / med(fwd["attn"]), 2),
        "forward_and_backward": round(med(both["torch_statement_fwd_bwd"]) / (med(fwd["attn"]) + med(bwd["attn"])), 2)}
    del sets, s0
    torch.cuda.empty_cache()
    # ---- one replayed step of the attention model next to the Laplacian model's, same batch
    rng = np.random.default_rng(a.seed)
    ds = NP.NormalFrames.from_meshes([mesh_ops.torus_grid(a.n, a.m, rng) for _ in range(a.meshes)], model="lap", device=dev)
    batch = ds.sample_batch(a.meshes, ids=np.arange(a.meshes))
    out["step"] = {"layers": a.layers, "meshes": a.meshes, "rows": int(batch.L.shape[0])}
    runs = {}
    for name, make in (("lap_gat", lambda: attention.LapGatModel(3, 3, layers=a.layers, heads=H)),
                       ("lap_deep", lambda: NP.LapDeepModel(3, 3, layers=a.layers))):
        torch.manual_seed(a.seed)
        model = make().to(dev).train()
        step = NP.graphed_train_step(model, NP.make_optimizer(model), batch)
        runs[name] = (lambda s=step: s(batch))
    t = _alternate(runs, a.warmup, a.samples, 1)
    out["step"].update({k: _stats(v) for k, v in t.items()})
    out["step"]["lap_gat_over_lap_deep"] = round(med(t["lap_gat"]) / med(t["lap_deep"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
