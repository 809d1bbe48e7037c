"""Times forward + backward of the `cel` / `sl1` dense-correspondence losses at the FAUST size (7000 padded / 6890 scored rows,
K = 120): (a) the plain-torch materialised composition (bmm, two gathers, soft-min / log-soft-max or smooth-L1, autograd) and
(b) the fused kernels (sn_pair_soft_* / sn_pair_sl1_*).  Median of --reps timed repetitions with device events after --warmup.
One leg per process: `python tools/pair_loss_probe.py --loss cel --leg fused`; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", choices=["cel", "sl1"], required=True)
    ap.add_argument("--leg", choices=["torch", "fused"], required=True)
    ap.add_argument("--rows", type=int, default=7000)
    ap.add_argument("--n", type=int, default=6890)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from surfacenetworks_amd import dense_correspondence as dc

    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    frames = []
    for _ in range(2):
        label = torch.randperm(a.n, generator=g).to(dev)
        frames.append(((torch.rand(a.n, a.n, generator=g) * 3).to(dev), label, torch.argsort(label)))
    tx, ty = frames
    FA = (torch.randn(1, a.rows, 120, generator=g) * 0.7).to(dev).requires_grad_(True)
    FB = (torch.randn(1, a.rows, 120, generator=g) * 0.7).to(dev).requires_grad_(True)
    if a.leg == "fused":
        HA, HB = dc.label_order_matrix(tx[0], tx[2]), dc.label_order_matrix(ty[0], ty[2])
        geo = dc.pair_geo_table(HA, HB)
        fn = dc.fused_pair_soft_cross_entropy if a.loss == "cel" else dc.fused_pair_smooth_l1
        run = lambda: fn(FA, FB, HA, HB, tx[2], ty[2], a.n, a.n, geo)
    else:
        run = lambda: dc.LOSSES[a.loss](torch.bmm(FA, FB.transpose(1, 2)), [tx], [ty])
    times = []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = run()
        torch.autograd.grad(loss.sum(), (FA, FB))
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1))
    print(json.dumps({"loss": a.loss, "leg": a.leg, "rows": a.rows, "scored": a.n, "median_ms": round(statistics.median(times), 4),
                      "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "reps": a.reps, "value": float(loss.sum()),
                      "device": torch.cuda.get_device_name(0), "hip": torch.version.hip}))


if __name__ == "__main__":
    main()
