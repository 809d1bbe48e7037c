"""Times the eigen-solver and the wave kernel signature (operators.laplacian_eigenpairs / wave_kernel_signature) on one MI355X, at
the defaults (k = 300, guard 37, deg 24, tol 1e-10):
(a) `solve`: one jittered --grid x --grid cloth (71 x 71 = 5041 vertices), a host clock around the call (it ends in reads of the
    residuals): seconds per solve, outer iterations, the worst residual over tol b, and the WKS on top of it;
(b) `batch`: --batch such cloths through the batch axis, the same figures per mesh;
(c) `filter`: sn_cheb_filter_step_f64 alone at the solve's shape (n x m, the mesh's standard form), --reps launches between device
    events: microseconds per launch and the achieved bytes/s against the bytes a step must move (X and Y read, Z written once:
    3 n m 8, plus the CSR arrays; the gathered rows of Y beyond the first read are cache traffic and are not counted).  The
    solve's time is split with it: filter = launches x this, dense = the rest (QR, X^T A X, eigh, rotations, host reads);
(d) `dense_ms`: torch.linalg.qr of the n x m block, X^T (A X), the m x m eigh on the device and on the host, and one rotation, each
    alone at the same shape, in milliseconds;
(e) `eigsh`: scipy.sparse.linalg.eigsh(S, M=diag(Am), sigma=-1e-5, k=300), the reference's call (geom_utils.compute_wks:420 with
    -L = S), on this box's host for the same mesh, and the largest eigenvalue difference to (a).
Prints one JSON line.  Not part of bench.py.
--measure-bounds runs no GPU code: it prints, per case of tests/spectral_cases.py, the M-orthonormality and the WKS error of the
HOST statement against the dense oracle — the figures behind ORTH_MEASURED and WKS_MEASURED there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def measure_bounds():
    import spectral_cases as cases
    from surfacenetworks_amd import mesh_ops

    out = {}
    for name in cases.NAMES:
        k, st = cases.case(name).k, cases.statement(name)
        wks = np.concatenate([mesh_ops.wave_kernel_signature(None, None, cases.N_WKS, k, ep, np.float64) for ep in st])
        out[name] = {"k": k, "outer": [ep.outer_iterations for ep in st],
                     "orthonormality": max(cases.orthonormality(ep.vectors, ep.mass) for ep in st),
                     "wks_error": cases.wks_error(wks, name)}
    out["worst"] = {q: max(v[q] for v in out.values()) for q in ("orthonormality", "wks_error")}
    print(json.dumps(out))


def cloth(grid, seed):
    from surfacenetworks_amd import mesh_ops

    V, F = mesh_ops.grid_cloth(grid, grid, np.random.default_rng(seed))
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=71)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--skip-eigsh", action="store_true")
    ap.add_argument("--measure-bounds", action="store_true")
    args = ap.parse_args()
    if args.measure_bounds:
        return measure_bounds()
    import torch

    from surfacenetworks_amd import kernels, mesh_ops, operators

    assert torch.cuda.is_available(), "spectral_probe times the MI355X; --measure-bounds is the part without one"
    dev = torch.device("cuda")
    out = {"grid": args.grid, "k": args.k, "eigh_on_host": operators._EIGH_ON_HOST}

    def solve(V, F):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep = operators.laplacian_eigenpairs(V, F, k=args.k)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        t0 = time.perf_counter()
        wks = operators.wave_kernel_signature(V, F, eigenpairs=ep)
        torch.cuda.synchronize()
        return ep, wks, sec, time.perf_counter() - t0

    # (a)
    V, F = cloth(args.grid, 3)
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    solve(Vd, Fd)                                        # warm-up: code objects, library handles
    ep, wks, sec, wsec = solve(Vd, Fd)
    outer = int(ep.outer_iterations.max())
    out["solve"] = {"vertices": int(V.shape[0]), "seconds": round(sec, 4), "outer_iterations": ep.outer_iterations.tolist(),
                    "status": ep.status, "worst_residual_over_tol_b": float((ep.residuals / (1e-10 * ep.bound[:, None])).max()),
                    "wks_seconds": round(wsec, 5), "wks_finite": bool(torch.isfinite(wks).all())}
    # (c)
    n, m = V.shape[0], min(V.shape[0], args.k + mesh_ops.eig_guard(args.k))
    rowptr, colind, S, mass, _ = kernels.cot_pencil_from_mesh(Vd, Fd)
    voff = torch.tensor([0, n], dtype=torch.int32, device=dev)
    sc = [torch.full((1,), v, dtype=torch.float64, device=dev) for v in (1e-3, 0.5, 100.0)]
    X, Y = torch.randn(n, m, dtype=torch.float64, device=dev), torch.randn(n, m, dtype=torch.float64, device=dev)
    Z = torch.empty_like(X)
    for _ in range(10):
        kernels.cheb_filter_step(rowptr, colind, S, voff, *sc, X, Y, out=Z)
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(args.reps):
        kernels.cheb_filter_step(rowptr, colind, S, voff, *sc, X, Y, out=Z)
    end.record()
    torch.cuda.synchronize()
    us = beg.elapsed_time(end) * 1e3 / args.reps
    must = 3 * n * m * 8 + int(colind.numel()) * 12 + (n + 1) * 4
    launches = outer + (outer - 1) * 24
    out["filter"] = {"n": n, "m": m, "nnz": int(colind.numel()), "us_per_launch": round(us, 2), "bytes_must_move": must,
                     "achieved_TB_per_s": round(must / us * 1e-6, 3), "launches_per_solve": launches,
                     "filter_seconds_per_solve": round(launches * us * 1e-6, 4),
                     "dense_and_host_seconds_per_solve": round(sec - launches * us * 1e-6, 4)}
    # (d) the dense steps of one outer iteration at the same shape, each between device events (the host eigh: a host clock
    # around the copy down, numpy's eigh and the copy back)
    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / reps * 1e3, 3)

    Q0 = torch.linalg.qr(X)[0]
    H = Q0.T @ (Q0 * torch.linspace(1.0, 2.0, m, dtype=torch.float64, device=dev))
    H = (H + H.T) / 2
    Qm = torch.linalg.eigh(H)[1]
    out["dense_ms"] = {"qr_n_by_m": timed(lambda: torch.linalg.qr(X)), "xt_ax": timed(lambda: Q0.T @ Y),
                       "eigh_m_device": timed(lambda: torch.linalg.eigh(H)),
                       "eigh_m_host": timed(lambda: torch.from_numpy(np.linalg.eigh(H.cpu().numpy())[1]).to(dev)),
                       "rotate_n_by_m": timed(lambda: Q0 @ Qm)}
    # (b)
    if args.batch > 1:
        Vb = torch.from_numpy(np.stack([cloth(args.grid, 100 + b)[0] for b in range(args.batch)])).to(dev)
        ep_b, _, sec_b, wsec_b = solve(Vb, Fd)
        out["batch"] = {"meshes": args.batch, "seconds": round(sec_b, 4), "seconds_per_mesh": round(sec_b / args.batch, 4),
                        "outer_iterations": ep_b.outer_iterations.tolist(), "status": ep_b.status, "wks_seconds": round(wsec_b, 5)}
    # (e)
    if not args.skip_eigsh:
        import scipy.sparse
        import scipy.sparse.linalg

        Sh, mh, _ = mesh_ops.cot_pencil(V, F)
        Am, _ = mesh_ops.eig_normalised_mass(mh, [0, n])
        t0 = time.perf_counter()
        E, _ = scipy.sparse.linalg.eigsh(Sh, M=scipy.sparse.diags(Am), sigma=-1e-5, k=args.k)
        out["eigsh"] = {"seconds": round(time.perf_counter() - t0, 3),
                        "max_abs_value_difference": float(np.abs(np.sort(E) - ep.values[0].cpu().numpy()).max()),
                        "tol_b": 1e-10 * float(ep.bound[0])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
