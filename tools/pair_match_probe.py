"""Times the matching of one FAUST-sized pair (7000 padded / 6890 scored rows, K = 120) in both directions:
(a) `fused`: dense_correspondence.match_features (sn_pair_match_f32, the score matrix never written);
(b) `materialised`: torch.bmm + max(dim=1) + max(dim=0) on the (N, N) product — library code, the route a user had before;
(c) `hard_fwd`: kernels.pair_fused_fwd, the forward of the hard-target loss (pair_fwd_k<PairHard>, one direction), as the
    yardstick: the same skeleton doing more work per tile.
The legs alternate inside one process (--rounds rounds of --reps calls each, timed with device events around the whole block
after --warmup calls of every leg); the peak-allocation rise of one call of each leg is reported next to the times.
Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=7000)
    ap.add_argument("--n", type=int, default=6890)
    ap.add_argument("--k", type=int, default=120)
    ap.add_argument("--reps", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from surfacenetworks_amd import _lib, kernels
    from surfacenetworks_amd import dense_correspondence as dc

    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    FA = (torch.randn(1, a.rows, a.k, generator=g) * 0.7).to(dev)
    FB = (torch.randn(1, a.rows, a.k, generator=g) * 0.7).to(dev)
    target = torch.randint(0, a.n, (a.n,), generator=g).to(dev)
    assert dc.fused_pair_supported(FA, FB)

    def materialised():
        S = torch.bmm(FA[:, :a.n], FB[:, :a.n].transpose(1, 2))[0]
        return S.max(dim=1), S.max(dim=0)

    legs = {"fused": lambda: dc.match_features(FA, FB, a.n, a.n, both=True), "materialised": materialised,
            "hard_fwd": lambda: kernels.pair_fused_fwd(FA[0], FB[0], target, a.n, a.n)}
    peak = {}
    for name, run in legs.items():
        for _ in range(a.warmup):
            out = run()
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        del out
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.reps)
    m = dc.match_features(FA, FB, a.n, a.n)
    (_, ia), (_, ib) = materialised()
    res = {"rows": a.rows, "scored": a.n, "K": a.k, "reps": a.reps, "rounds": a.rounds,
           "workspace_bytes": int(_lib.load().sn_pair_match_workspace_bytes(a.rows, a.rows)),
           "agree_a2b": float((m.a2b == ia).double().mean()), "agree_b2a": float((m.b2a == ib).double().mean()),
           "device": torch.cuda.get_device_name(0), "hip": torch.version.hip}
    for name in legs:
        res[name] = {"median_ms": round(statistics.median(times[name]), 4), "min_ms": round(min(times[name]), 4),
                     "max_ms": round(max(times[name]), 4), "peak_rise_bytes": int(peak[name])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
