"""Checks of the PRODUCT modules against the reference-generated golden fixtures, parametrised by device so that the
CPU suite (oracle-backed kernels) and the GPU suite (real HIP kernels) run the very same assertions."""
import os

import numpy as np
import scipy.sparse as sp
import torch

from helpers import deterministic_init, det_tensor, grad_signature, load_golden, rel_err, sigs_close
from oracle import ref_blocks as OB

# Model-level criterion.  The deep fixtures are ill-conditioned in fp32 (the reference's OWN fp32 gradients of the FAUST fixture
# are off by 3x their norm against float64, its Mesh-MNIST gradients by 6 %: tests/golden/make_golden.py prints them), so a
# fixed tolerance against the reference's fp32 numbers would be either vacuous or flaky.  Two complementary checks instead:
#   * per layer (check_model_layers): every block of the product model, fed the REFERENCE's stored input of that block,
#     reproduces the reference's stored output to 1e-5 relative — conditioning cannot compound, a defect in one block shows;
#   * end to end (check_model): against the float64 oracle the product must be as close as the reference itself is,
#         err(product, fp64) <= SLACK * err(reference_fp32, fp64) + spread + FLOOR,    SLACK = 3,
#     where `spread` is MEASURED ON THE REFERENCE and stored in the fixture ({tag}_spread_*): the largest deviation from
#     float64 of eight fp32 runs of the imported reference whose inputs carry one-ulp relative noise — what any other valid
#     fp32 evaluation order may show.  No hand-picked constants.
SLACK, FLOOR = 3.0, 1e-6


def _sig_err(sigs, ref64):
    """Largest deviation of any gradient signature from the fp64 one, relative to the largest gradient norm."""
    top = max(abs(float(ref64[k][0])) for k in ref64)
    return max(float(np.abs(np.asarray(sigs[k]) - ref64[k]).max()) for k in ref64) / top


def _as_close_as_reference(name, prod, ref32, truth64, spread=0.0):
    e_prod, e_ref = rel_err(prod, truth64), rel_err(ref32, truth64)
    assert e_prod <= SLACK * e_ref + spread + FLOOR, (name, "product err", e_prod, "reference fp32 err", e_ref, "spread", spread)
    return e_prod, e_ref


BLOCKS = [("LapResNet2", 64), ("LapResNet2", 128), ("DirResNet2", 64), ("DirResNet2", 128), ("AvgResNet2", 128),
          ("MlpResNet2", 128)]


def load(golden_dir, name):
    return load_golden(golden_dir, name)


def csr_of(z, k):
    return sp.csr_matrix((z[f"{k}_data"], z[f"{k}_indices"], z[f"{k}_indptr"]), shape=tuple(z[f"{k}_shape"]))


def batch_operators(golden_dir, opkind, dev):
    """The ragged fixture batch (cube, delaunay150, delaunay60) as operators of the requested kind on `dev`."""
    from surfacenetworks_amd.operators import OperatorPool

    rb = load(golden_dir, "ragged_batch.npz")
    order = [str(s) for s in rb["order"]]
    nv, nf = int(rb["nv"]), int(rb["nf"])
    ops = {}
    for k, (s0, s1) in {"L": (nv, nv), "Di": (4 * nf, 4 * nv), "DiA": (4 * nv, 4 * nf)}.items():
        if opkind == "pool":
            mats = [csr_of(load(golden_dir, f"ops_{m}.npz"), k) for m in order]
            ops[k] = OperatorPool(mats, dev, want_bsr4=(k != "L")).assemble(np.arange(len(order)), s0, s1)
        else:
            key = "bd" if opkind == "coo2d" else "3d"
            ops[k] = torch.sparse_coo_tensor(torch.from_numpy(rb[f"{k}_{key}_indices"]), torch.from_numpy(rb[f"{k}_{key}_values"]),
                                             tuple(rb[f"{k}_{key}_shape"])).coalesce().to(dev)
    return rb, ops


def check_block(golden_dir, cname, C, opkind, dev, tol=1e-5):
    import surfacenetworks_amd.utils_pt as U

    rb, ops = batch_operators(golden_dir, opkind, dev)
    g = load(golden_dir, "blocks_reference.npz")
    B, nv, nf = rb["mask"].shape[0], int(rb["nv"]), int(rb["nf"])
    mask = torch.from_numpy(rb["mask"]).to(dev)
    tag = f"{cname}{C}"
    mod = deterministic_init(getattr(U, cname)(C), seed=C + len(cname)).train().to(dev)
    v = torch.from_numpy(det_tensor((B, nv, C), 11 + C, 1.0) * rb["mask"]).to(dev).requires_grad_(True)
    if cname == "DirResNet2":
        f = torch.from_numpy(det_tensor((B, nf, C), 12 + C, 1.0)).to(dev).requires_grad_(True)
        outs, gin = mod(ops["Di"], ops["DiA"], v, f), [v, f]
    else:
        outs, gin = (mod(ops["L"], mask, v),), [v]
    loss = sum((o * torch.from_numpy(det_tensor(tuple(o.shape), s)).to(dev)).sum() for o, s in zip(outs, [21, 22]))
    loss.backward()
    for i, o in enumerate(outs):
        assert rel_err(o.detach().cpu().numpy(), g[f"{tag}_out{i}"]) <= tol, (tag, i, rel_err(o.detach().cpu().numpy(), g[f"{tag}_out{i}"]))
    for i, t in enumerate(gin):
        assert rel_err(t.grad.cpu().numpy(), g[f"{tag}_gin{i}"]) <= tol, (tag, "gin", i, rel_err(t.grad.cpu().numpy(), g[f"{tag}_gin{i}"]))
    assert not sigs_close(grad_signature(mod), lambda k: g[f"{tag}_psig_{k}"])
    for k, t in mod.state_dict().items():
        if "running" in k:
            assert rel_err(t.cpu().numpy(), g[f"{tag}_{k}"]) <= 1e-5, (k, rel_err(t.cpu().numpy(), g[f"{tag}_{k}"]))


def _bn_train_only(m):
    m.eval()
    for mod in m.modules():
        if "BatchNorm" in mod.__class__.__name__:
            mod.train()
    return m


def check_model(golden_dir, tag, dev, opkind="pool", tol_out=5e-5, classes=None):
    """`classes`: tag -> constructor of the model under test (default: the product's own model classes; the import-swap test
    passes the REFERENCE's classes built on top of the product's utils_pt)."""
    from surfacenetworks_amd import arap, dense_correspondence, mesh_mnist
    from surfacenetworks_amd.operators import OperatorPool

    make = {"arap_dir": arap.DirModel, "arap_lap": lambda: arap.Model(15), "mnist_lap": mesh_mnist.Model,
            "mnist_dir": mesh_mnist.DirModel, "faust_lap": lambda: dense_correspondence.SiameseModel("lap", 15)}
    make.update(classes or {})
    g = load(golden_dir, "models_reference.npz")
    if tag == "faust_lap":
        rb = load(golden_dir, "ragged_batch.npz")
        nv = int(rb["nv"])
        L = csr_of(load(golden_dir, "ops_delaunay150.npz"), "L")
        if opkind == "pool":
            L1 = OperatorPool([L], dev).assemble([0], nv, nv)
        else:                                        # what an unmodified driver hands over: sparse_diag_cat's COO tensor
            import surfacenetworks_amd.utils_pt as U
            L1 = U.sparse_diag_cat([U.sp_sparse_to_pt_sparse(L)], nv, nv).coalesce().to(dev)
        lA, lB = torch.from_numpy(g["faust_lA"]).to(dev), torch.from_numpy(g["faust_lB"]).to(dev)
        tX = [(torch.from_numpy(g["faust_GA"]).to(dev), lA, torch.argsort(lA))]
        tY = [(torch.from_numpy(g["faust_GB"]).to(dev), lB, torch.argsort(lB))]
        cA = torch.from_numpy(rb["coords"][1:2]).to(dev)
        cB = torch.from_numpy(rb["coords"][1:2] * 1.1 + 0.02).to(dev)
        mask = torch.from_numpy(rb["mask"][1:2]).to(dev)
        m = deterministic_init(make["faust_lap"](), 11).train().to(dev)
        out = m([L1, mask], [L1, mask], cA, cB)
        loss = dense_correspondence.loss_fun_delta_cross_entropy(out, tX, tY)
        loss.backward()
        L64 = OB.diag_cat([OB.sp_to_coo(L.astype(np.float64))], nv, nv)
        m64 = deterministic_init(OB.SiameseModel("lap", 15), 11).train().double()
        c = lambda x: x.detach().cpu().double()
        out64 = m64([L64, c(mask)], [L64, c(mask)], c(cA), c(cB))
        loss64 = OB.delta_cross_entropy(out64, [(c(tX[0][0]), tX[0][1].cpu(), tX[0][2].cpu())], [(c(tY[0][0]), tY[0][1].cpu(), tY[0][2].cpu())])
        loss64.backward()
        s64 = grad_signature(m64)
        sp = lambda k: float(g[f"faust_lap_spread_{k}"])
        # the same loss streamed over row blocks from the towers' features (no (N, N) score matrix): same value
        with torch.no_grad():
            FA, FB = m.model(L1, mask, cA), m.model(L1, mask, cB)
            l_str = dense_correspondence.streamed_delta_cross_entropy(FA, FB, tX, tY, block=64)
        assert abs(l_str.item() - loss.item()) <= 2e-5 * abs(loss.item()), ("streamed faust loss", l_str.item(), loss.item())
        _as_close_as_reference("faust loss", loss.item(), float(g["faust_lap_loss"]), loss64.item(), sp("loss"))
        _as_close_as_reference("faust out", out.detach().cpu().numpy()[0, ::7, ::7], g["faust_lap_out_sample"],
                               out64.detach().numpy()[0, ::7, ::7], sp("out"))
        e_prod = _sig_err(grad_signature(m), s64)
        e_ref = _sig_err({k: g[f"faust_lap_psig_{k}"] for k in s64}, s64)
        assert e_prod <= SLACK * e_ref + sp("grad") + FLOOR, ("faust grad", e_prod, e_ref)
        if torch.device(dev).type == "cuda":
            # the product's pair step: the same loss from the towers' features, scores never written (sn_pair_fused_*)
            m2 = deterministic_init(make["faust_lap"](), 11).train().to(dev)
            FA2, FB2 = m2.towers([L1, mask], [L1, mask], cA, cB)
            assert dense_correspondence.fused_pair_supported(FA2, FB2)
            tgt = dense_correspondence.correspondence_target(*tX[0], *tY[0])
            loss2 = dense_correspondence.fused_pair_cross_entropy(FA2, FB2, tgt, int(lA.size(0)), int(lB.size(0)))
            loss2.backward()
            _as_close_as_reference("faust loss (fused)", loss2.item(), float(g["faust_lap_loss"]), loss64.item(), sp("loss"))
            e_fused = _sig_err(grad_signature(m2), s64)
            assert e_fused <= SLACK * e_ref + sp("grad") + FLOOR, ("faust grad (fused)", e_fused, e_ref)
        return
    rb, ops = batch_operators(golden_dir, opkind, dev)
    mask = torch.from_numpy(rb["mask"]).to(dev)
    B = mask.shape[0]
    t = lambda a: torch.from_numpy(a).to(dev)
    if tag == "arap_dir":
        m = deterministic_init(make["arap_dir"](), 7).train().to(dev)
        out = m(ops["Di"], ops["DiA"], mask, t(g["inputs6"]))
        loss = arap.loss_fn(out, t(g["targets"]), mask, B)
    elif tag == "arap_lap":
        m = deterministic_init(make["arap_lap"](), 8).train().to(dev)
        out = m(ops["L"], mask, t(g["inputs6"]))
        loss = arap.loss_fn(out, t(g["targets"]), mask, B)
    elif tag == "mnist_lap":
        m = _bn_train_only(deterministic_init(make["mnist_lap"](), 9)).to(dev)
        out = m(t(rb["coords"]), ops["L"], mask)
        loss = torch.nn.functional.nll_loss(out, t(g["labels"]))
    elif tag == "mnist_dir":
        m = _bn_train_only(deterministic_init(make["mnist_dir"](), 10)).to(dev)
        out = m(t(rb["coords"]), ops["Di"], ops["DiA"], mask)
        loss = torch.nn.functional.nll_loss(out, t(g["labels"]))
    else:
        raise KeyError(tag)
    loss.backward()
    l64, o64, s64 = _oracle_fp64(golden_dir, tag, rb, g)
    sp = lambda k: float(g[f"{tag}_spread_{k}"])
    el = _as_close_as_reference(tag + " loss", loss.item(), float(g[f"{tag}_loss"]), l64, sp("loss"))
    eo = _as_close_as_reference(tag + " out", out.detach().cpu().numpy(), g[f"{tag}_out"], o64, sp("out"))
    ref_sig = {k: g[f"{tag}_psig_{k}"] for k in s64}
    e_prod, e_ref = _sig_err(grad_signature(m), s64), _sig_err(ref_sig, s64)
    if os.environ.get("SN_TEST_VERBOSE"):
        print(f"[{tag}] err vs fp64 (product / reference fp32 / spread): loss {el[0]:.2e}/{el[1]:.2e}/{sp('loss'):.2e} "
              f"out {eo[0]:.2e}/{eo[1]:.2e}/{sp('out'):.2e} grad {e_prod:.2e}/{e_ref:.2e}/{sp('grad'):.2e}")
    assert e_prod <= SLACK * e_ref + sp("grad") + FLOOR, (tag, "grad: product err", e_prod, "reference fp32 err", e_ref)


def _oracle_fp64(golden_dir, tag, rb, g):
    """The exact answer: the oracle restatement of the reference model run in float64 on the CPU."""
    ops = {}
    for k in ("L", "Di", "DiA"):
        ops[k] = torch.sparse_coo_tensor(torch.from_numpy(rb[f"{k}_bd_indices"]), torch.from_numpy(rb[f"{k}_bd_values"]).double(),
                                         tuple(rb[f"{k}_bd_shape"])).coalesce()
    mask = torch.from_numpy(rb["mask"]).double()
    B = mask.shape[0]
    d = lambda a: torch.from_numpy(a).double()
    if tag == "arap_dir":
        m = deterministic_init(OB.ArapDirModel(), 7).train().double()
        out = m(ops["Di"], ops["DiA"], mask, d(g["inputs6"]))
        loss = OB.arap_loss(out, d(g["targets"]), mask, B)
    elif tag == "arap_lap":
        m = deterministic_init(OB.ArapLapModel(15), 8).train().double()
        out = m(ops["L"], mask, d(g["inputs6"]))
        loss = OB.arap_loss(out, d(g["targets"]), mask, B)
    elif tag == "mnist_lap":
        m = _bn_train_only(deterministic_init(OB.MnistLapModel(), 9)).double()
        out = m(d(rb["coords"]), ops["L"], mask)
        loss = torch.nn.functional.nll_loss(out, torch.from_numpy(g["labels"]))
    else:
        m = _bn_train_only(deterministic_init(OB.MnistDirModel(), 10)).double()
        out = m(d(rb["coords"]), ops["Di"], ops["DiA"], mask)
        loss = torch.nn.functional.nll_loss(out, torch.from_numpy(g["labels"]))
    loss.backward()
    return loss.item(), out.detach().numpy(), grad_signature(m)


def check_cat_functions(golden_dir):
    """utils_pt.sparse_diag_cat / sparse_cat / sp_sparse_to_pt_sparse reproduce the reference's outputs exactly."""
    import surfacenetworks_amd.utils_pt as U

    rb = load(golden_dir, "ragged_batch.npz")
    order = [str(s) for s in rb["order"]]
    nv, nf = int(rb["nv"]), int(rb["nf"])
    for k, (s0, s1) in {"L": (nv, nv), "Di": (4 * nf, 4 * nv), "DiA": (4 * nv, 4 * nf)}.items():
        parts = [U.sp_sparse_to_pt_sparse(csr_of(load(golden_dir, f"ops_{m}.npz"), k)) for m in order]
        assert parts[0].dtype == torch.float32 and not parts[0].is_coalesced()
        bd, b3 = U.sparse_diag_cat(parts, s0, s1), U.sparse_cat(parts, s0, s1)
        assert np.array_equal(bd._indices().numpy(), rb[f"{k}_bd_indices"]) and np.array_equal(bd._values().numpy(), rb[f"{k}_bd_values"])
        assert tuple(bd.shape) == tuple(rb[f"{k}_bd_shape"])
        assert np.array_equal(b3._indices().numpy(), rb[f"{k}_3d_indices"]) and np.array_equal(b3._values().numpy(), rb[f"{k}_3d_values"])
        assert tuple(b3.shape) == tuple(rb[f"{k}_3d_shape"])
    dense = U.to_dense_batched(parts[0], 2)
    assert dense.shape[0] == 2 and torch.equal(dense[0], parts[0].to_dense())


def check_spmm_autograd(dev):
    """spmm() and SparseBMMFunc: forward vs dense fp64, backward = A^T g, no grad to the operator."""
    import surfacenetworks_amd.utils_pt as U
    from helpers import mesh_fixture
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd.operators import SparseOperator

    _, _, ops = mesh_fixture("cloth")
    for name, group, N in [("L", 1, 24), ("Di", 4, 16), ("DiA", 4, 32)]:
        A = ops[name]
        M, K = A.shape
        rng = np.random.default_rng(3)
        x = rng.standard_normal((K // group, group * N)).astype(np.float32)
        gy = rng.standard_normal((M // group, group * N)).astype(np.float32)
        xt = torch.from_numpy(x).to(dev).requires_grad_(True)
        y = snF.spmm(SparseOperator.from_scipy(A, dev), xt, group)
        y.backward(torch.from_numpy(gy).to(dev))
        A64 = A.astype(np.float64)
        assert rel_err(y.detach().cpu().numpy().reshape(M, N), A64 @ x.reshape(K, N).astype(np.float64)) < 1e-6
        assert rel_err(xt.grad.cpu().numpy().reshape(K, N), A64.T @ gy.reshape(M, N).astype(np.float64)) < 1e-6
    # 3-D batched call shape of the reference: SparseBMMFunc()(A3d, X3d)
    A = ops["Di"].tocoo()
    B = 2
    idx = np.stack([np.repeat(np.arange(B), A.nnz), np.tile(A.row, B), np.tile(A.col, B)]).astype(np.int64)
    A3 = torch.sparse_coo_tensor(torch.from_numpy(idx), torch.from_numpy(np.tile(A.data, B)), (B,) + A.shape).coalesce().to(dev)
    X3 = torch.from_numpy(np.random.default_rng(4).standard_normal((B, A.shape[1], 16)).astype(np.float32)).to(dev).requires_grad_(True)
    Y3 = U.SparseBMMFunc()(A3, X3)
    assert Y3.shape == (B, A.shape[0], 16)
    Y3.sum().backward()
    want = np.stack([ops["Di"].astype(np.float64) @ X3.detach().cpu().numpy()[b].astype(np.float64) for b in range(B)])
    assert rel_err(Y3.detach().cpu().numpy(), want) < 1e-6
    colsum = np.asarray(ops["Di"].astype(np.float64).sum(axis=0)).ravel()
    assert rel_err(X3.grad.cpu().numpy()[0][:, 0], colsum) < 1e-5


def check_arap_sampler(dev):
    """ClothSequences.sample_batch == the reference's sample_batch semantics: padded tensors + block-diag operators
    equal to sparse_diag_cat of the per-sample operators."""
    from surfacenetworks_amd import arap, mesh_ops

    ds = arap.ClothSequences([(7, 6), (9, 8), (5, 5)], frames=45, op_frames=3, seed=1, device=dev, model="dir")
    rng = np.random.default_rng(0)
    seq_ids, offsets = np.array([1, 0, 2, 1]), np.array([0, 1, 1, 1])
    b = ds.sample_batch(4, rng, seq_ids=seq_ids, offsets=offsets)
    nv, nf = 72, int(ds.num_faces.max())
    assert b.inputs.shape == (4, nv, 6) and b.targets.shape == (4, nv, 120) and b.mask.shape == (4, nv, 1)
    xyz = ds.xyz.cpu().numpy()
    for i, (s, o) in enumerate(zip(seq_ids, offsets)):
        n = ds.num_vertices[s]
        for fr in range(2):
            assert np.array_equal(b.inputs[i, :n, 3 * fr: 3 * fr + 3].cpu().numpy(), xyz[s, o + fr, :n])
        for fr in range(40):
            assert np.array_equal(b.targets[i, :n, 3 * fr: 3 * fr + 3].cpu().numpy(), xyz[s, o + 2 + fr, :n])
        assert b.mask[i, :n].sum() == n and b.mask[i, n:].sum() == 0 and b.inputs[i, n:].abs().sum() == 0
    # operators: frame offset+1 of each sequence (main.py:156), padded block-diagonal
    blocks = []
    for s, o in zip(seq_ids, offsets):
        n, m = [(7, 6), (9, 8), (5, 5)][s]
        F_ = mesh_ops._grid_faces(n, m, False)
        Di, _ = mesh_ops.dirac(xyz[s, o + 1, : ds.num_vertices[s]].astype(np.float64), F_)
        P = sp.lil_matrix((4 * nf, 4 * nv), dtype=np.float32)
        P[: Di.shape[0], : Di.shape[1]] = Di.astype(np.float32)
        blocks.append(P.tocsr())
    want = sp.block_diag(blocks, format="csr")
    got = b.Di.to_scipy()
    # operators are built from the fp64 frame coordinates (as the reference does from its .obj files), the test rebuilds
    # them from the stored fp32 coordinates: same pattern, values equal to fp32 round-off of the coordinates
    assert got.shape == want.shape and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert abs(got - want).max() <= 1e-4 * abs(want).max()
    assert b.DiA.shape == (4 * 4 * nv, 4 * 4 * nf)
    m = arap.DirModel().to(dev)
    loss, out = arap.forward_loss(m, b)
    assert out.shape == (4, nv, 120) and torch.isfinite(loss)


def check_mnist_sampler(dev):
    from surfacenetworks_amd import mesh_mnist

    ds = mesh_mnist.MeshDigits(6, seed=2, device=dev, vmin=20, vmax=40, model="lap")
    rng = np.random.default_rng(0)
    order = np.argsort(ds.nv)
    b1 = ds.sample_batch(2, rng, ids=order[:2])
    b2 = ds.sample_batch(2, rng, ids=order[-2:])
    b3 = ds.sample_batch(2, rng, ids=order[:2])
    assert b1.inputs.shape[1] == ds.nv[order[1]] and b2.inputs.shape[1] == ds.nv.max()
    assert b3.inputs.shape[1] == ds.nv.max()          # running maximum, as mesh_mnist/main.py:83-84,119-120
    assert b3.L.shape == (2 * ds.nv.max(), 2 * ds.nv.max())
    m = mesh_mnist.Model().to(dev)
    loss, out = mesh_mnist.forward_loss(m, b3)
    assert out.shape == (2, 10) and torch.isfinite(loss)


def check_mnist_evaluation_mode(dev):
    """mesh_mnist/main.py:178-182: the driver evaluates with `model.eval()` and then puts every BatchNorm module back into
    train mode ("BatchNorm for some reasons is not stable in eval") — dropout off, batch statistics on, running statistics
    still advancing — and calls `loss.backward()` there too.  The product in that mixed mode against the oracle models
    (pinned to the reference's) in the same mode.  The fixture is ill-conditioned in fp32 (Laplacian entries up to 1e4), so
    the yardstick is the oracle's own fp32 run: the product must be as close to the fp64 result as that is."""
    import torch.nn.functional as F

    from oracle import ref_blocks as rb
    from surfacenetworks_amd import mesh_mnist

    def mixed(m_):
        m_.eval()
        for mod in m_.modules():
            if mod.__class__.__name__.find("BatchNorm") > -1:
                mod.train()
        return m_

    def flat(vals):
        return torch.cat([v.detach().cpu().double().reshape(-1) for v in vals])

    def dist(x, ref_):
        return float((x - ref_).norm()) / max(float(ref_.norm()), 1e-30)

    for kind, prod_cls, ref_cls in (("lap", mesh_mnist.Model, rb.MnistLapModel), ("dir", mesh_mnist.DirModel, rb.MnistDirModel)):
        ds = mesh_mnist.MeshDigits(4, seed=6, device=dev, vmin=40, vmax=56, model=kind)
        b = ds.sample_batch(4, np.random.default_rng(1), ids=np.arange(4))
        r64 = deterministic_init(ref_cls(), 21).double()
        r32 = deterministic_init(ref_cls(), 21)
        prod = prod_cls()
        prod.load_state_dict(r32.state_dict())
        prod = prod.to(dev)
        ops_p = (b.L,) if kind == "lap" else (b.Di, b.DiA)
        dense = [torch.from_numpy(o.to_scipy().toarray()) for o in ops_p]
        tg = b.targets.cpu()
        out64 = mixed(r64)(b.inputs.cpu().double(), *(d.double().to_sparse() for d in dense), b.mask.cpu().double())
        out32 = mixed(r32)(b.inputs.cpu(), *(d.float().to_sparse() for d in dense), b.mask.cpu())
        outp = mixed(prod)(b.inputs, *ops_p, b.mask)
        F.nll_loss(out64, tg).backward()
        F.nll_loss(out32, tg).backward()
        F.nll_loss(outp, b.targets).backward()
        assert not prod.training and prod.rn0.bn_fc0.bn.training
        e_ref, e_prod = dist(flat([out32]), flat([out64])), dist(flat([outp]), flat([out64]))
        assert e_prod <= 2 * e_ref + 1e-5, (kind, "outputs", e_prod, e_ref)
        g64 = flat(q.grad for q in r64.parameters())
        e_ref, e_prod = dist(flat(q.grad for q in r32.parameters()), g64), dist(flat(q.grad for q in prod.parameters()), g64)
        assert e_prod <= 2 * e_ref + 1e-5, (kind, "parameter gradients", e_prod, e_ref)
        names = [k for k in r64.state_dict() if "running" in k]
        s64 = flat(r64.state_dict()[k] for k in names)
        e_ref = dist(flat(r32.state_dict()[k] for k in names), s64)
        e_prod = dist(flat(prod.state_dict()[k] for k in names), s64)
        assert e_prod <= 2 * e_ref + 1e-5, (kind, "running statistics", e_prod, e_ref)
        for k, v in prod.state_dict().items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 1, k


def check_pool_packed(golden_dir, dev):
    """OperatorPool.assemble(sel) without sizes = the PACKED batch: block_diag of the unpadded per-mesh operators (exact),
    transpose attached, offsets on the operator; and the packed product equals, mesh by mesh and bit for bit, the padded
    product of the reference layout (the padding only adds empty rows / unused columns)."""
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd.operators import OperatorPool

    names = ["cube", "delaunay150", "delaunay60"]
    sel = [1, 0, 2, 1]
    rng = np.random.default_rng(4)
    for k, group, C in [("L", 1, 64), ("Di", 4, 128), ("DiA", 4, 128), ("L", 1, 128), ("Di", 4, 64)]:
        mats = [csr_of(load(golden_dir, f"ops_{m}.npz"), k).astype(np.float32) for m in names]
        pool = OperatorPool(mats, dev, want_bsr4=(group == 4))
        op = pool.assemble(sel)
        want = sp.block_diag([mats[i] for i in sel], format="csr")
        want.sort_indices()
        got = op.to_scipy()
        assert got.shape == want.shape and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data)
        gt, wt = op.t().to_scipy(), want.T.tocsr()
        wt.sort_indices()
        assert np.array_equal(gt.indptr, wt.indptr) and np.array_equal(gt.indices, wt.indices) and np.array_equal(gt.data, wt.data)
        ro, co = op.row_offsets, op.col_offsets
        assert ro[-1] == want.shape[0] and co[-1] == want.shape[1] and np.array_equal(np.diff(ro), [mats[i].shape[0] for i in sel])
        assert np.array_equal(op.t().row_offsets, co) and op.batch == len(sel)
        # packed vs padded product, forward and transposed backward
        s0, s1 = max(m.shape[0] for m in mats), max(m.shape[1] for m in mats)
        pad = pool.assemble(sel, s0, s1)
        N = C // group
        xp = rng.standard_normal((want.shape[1] // group, group * N)).astype(np.float32)
        gp = rng.standard_normal((want.shape[0] // group, group * N)).astype(np.float32)
        xd = np.zeros((len(sel), s1 // group, group * N), np.float32)
        gd = np.zeros((len(sel), s0 // group, group * N), np.float32)
        for b in range(len(sel)):
            xd[b, : (co[b + 1] - co[b]) // group] = xp[co[b] // group: co[b + 1] // group]
            gd[b, : (ro[b + 1] - ro[b]) // group] = gp[ro[b] // group: ro[b + 1] // group]
        xt = torch.from_numpy(xp).to(dev).requires_grad_(True)
        y = snF.spmm(op, xt, group)
        y.backward(torch.from_numpy(gp).to(dev))
        xdt = torch.from_numpy(xd.reshape(-1, group * N)).to(dev).requires_grad_(True)
        yd = snF.spmm(pad, xdt, group)
        yd.backward(torch.from_numpy(gd.reshape(-1, group * N)).to(dev))
        yd3 = yd.detach().cpu().numpy().reshape(len(sel), s0 // group, group * N)
        gx3 = xdt.grad.cpu().numpy().reshape(len(sel), s1 // group, group * N)
        yp, gxp = y.detach().cpu().numpy(), xt.grad.cpu().numpy()
        for b in range(len(sel)):
            assert np.array_equal(yp[ro[b] // group: ro[b + 1] // group], yd3[b, : (ro[b + 1] - ro[b]) // group]), (k, b)
            assert not yd3[b, (ro[b + 1] - ro[b]) // group:].any()
            assert np.array_equal(gxp[co[b] // group: co[b + 1] // group], gx3[b, : (co[b + 1] - co[b]) // group]), (k, b)
        want64 = want.astype(np.float64) @ (xp.reshape(-1, N) if group == 1 else xp.reshape(-1, 4, N).reshape(-1, N)).astype(np.float64)
        assert rel_err(yp.reshape(-1, N), want64) < 1e-6


def check_inplace_edit_drops_handoff(golden_dir, dev):
    """The activated hand-off between blocks (blocks.attach_activated) must not survive an in-place edit of the tensor it
    rides on: block(x.mul_(m)) has to equal block(x * m)."""
    import surfacenetworks_amd.utils_pt as U

    rb, ops = batch_operators(golden_dir, "pool", dev)
    B, nv, C = rb["mask"].shape[0], int(rb["nv"]), 128
    mask = torch.from_numpy(rb["mask"]).to(dev)
    b0 = deterministic_init(U.LapResNet2(C), 7).train().to(dev)
    b1 = deterministic_init(U.LapResNet2(C), 8).train().to(dev)
    outs = []
    for inplace in (True, False):
        x = torch.from_numpy(det_tensor((B, nv, C), 3)).to(dev)
        with torch.no_grad():
            h = b0(ops["L"], None, x)
            assert "_sn_cat" in h.__dict__                     # the hand-off is there ...
            if inplace:
                h.mul_(mask)                                   # ... and an in-place edit must invalidate it
                h[:, 0] = 0.25
            else:
                h = h * mask
                h = torch.cat([torch.full_like(h[:, :1], 0.25), h[:, 1:]], 1)
            outs.append(b1(ops["L"], None, h).cpu().numpy())
    assert rel_err(outs[0], outs[1]) < 1e-6


def check_model_layers(golden_dir, tag, dev, tol=1e-5):
    """Every layer of the product model, fed the REFERENCE's stored input of that layer (layers_reference.npz: the outputs
    of conv1 and of every rn{i} of the imported reference model on the batch cube + delaunay60), reproduces the reference's
    stored output to `tol` = 1e-5 relative — outputs and, for Dirac blocks, the face stream.  Where the reference's own fp32
    block output is further than tol/4 from the float64 block (stored as {tag}_rn{i}_eref: the Mesh-MNIST-scaled Laplacian
    has entries of 1e4 with rows summing to zero), the bound is 4 x that error — product within 3 x the reference's own."""
    from surfacenetworks_amd import arap, mesh_mnist
    from surfacenetworks_amd.operators import OperatorPool

    z = load(golden_dir, "layers_reference.npz")
    order = [str(s_) for s_ in z["order"]]
    nv, nf = int(z["nv"]), int(z["nf"])
    mask = torch.from_numpy(z["mask"]).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ops = {}
    for k, (s0, s1) in {"L": (nv, nv), "Di": (4 * nf, 4 * nv), "DiA": (4 * nv, 4 * nf)}.items():
        mats = [csr_of(load(golden_dir, f"ops_{m}.npz"), k) for m in order]
        ops[k] = OperatorPool(mats, dev, want_bsr4=(k != "L")).assemble(np.arange(len(order)), s0, s1)
    if tag == "arap_dir":
        m, nlayer, x0 = deterministic_init(arap.DirModel(), 7).train().to(dev), 15, t(z["inputs6"])
    elif tag == "arap_lap":
        m, nlayer, x0 = deterministic_init(arap.Model(15), 8).train().to(dev), 15, t(z["inputs6"])
    elif tag == "faust_lap":                     # one tower of the siamese model (3 input channels)
        from surfacenetworks_amd import dense_correspondence

        m, nlayer, x0 = deterministic_init(dense_correspondence.Model(15), 11).train().to(dev), 15, t(z["coords"])
    elif tag == "mnist_dir":
        m, nlayer, x0 = _bn_train_only(deterministic_init(mesh_mnist.DirModel(), 10)).to(dev), 5, t(z["coords"])
    else:
        m, nlayer, x0 = _bn_train_only(deterministic_init(mesh_mnist.Model(), 9)).to(dev), 5, t(z["coords"])
    worst = 0.0
    with torch.no_grad():
        e = rel_err(m.conv1(x0).cpu().numpy(), z[f"{tag}_conv1_v"])
        assert e <= tol, (tag, "conv1", e)
        for i in range(nlayer):
            prev = "conv1" if i == 0 else f"rn{i - 1}"
            blk = m._modules[f"rn{i}"]
            v_in = t(z[f"{tag}_{prev}_v"])
            want_v = z[f"{tag}_rn{i}_v"]
            if (tag == "arap_dir" and i % 2 == 0) or tag == "mnist_dir":
                # the face stream entering block i is the f returned by the previous Dirac block (zeros for the first)
                back = 2 if tag == "arap_dir" else 1
                fkey = f"{tag}_rn{i - back}_f"
                f_in = t(z[fkey]) if i >= back else torch.zeros(v_in.shape[0], nf, v_in.shape[2], device=dev)
                v_out, f_out = blk(ops["Di"], ops["DiA"], v_in, f_in)
                ef = rel_err(f_out.cpu().numpy(), z[f"{tag}_rn{i}_f"])
                assert ef <= max(tol, 4.0 * float(z[f"{tag}_rn{i}_eref"])), (tag, f"rn{i} face stream", ef)
                worst = max(worst, ef)
            elif tag == "arap_dir":
                v_out = blk(None, mask, v_in)
            else:
                v_out = blk(ops["L"], mask, v_in)
            e = rel_err(v_out.cpu().numpy(), want_v)
            assert e <= max(tol, 4.0 * float(z[f"{tag}_rn{i}_eref"])), (tag, f"rn{i}", e, "reference's own fp32 error", float(z[f"{tag}_rn{i}_eref"]))
            worst = max(worst, e)
    if os.environ.get("SN_TEST_VERBOSE"):
        print(f"[{tag}] per-layer: worst relative deviation from the reference's layer outputs {worst:.2e}")


def check_dataset_files(golden_dir, dev):
    """files in the reference's on-disk layouts (tests/golden/data_*: written by the reference's own
    add_laplacian.process functions, see make_dataset_fixtures.py) -> device-resident pools -> training steps."""
    from surfacenetworks_amd import arap, datasets, dense_correspondence as dc, mesh_mnist

    # ---- ARAP sequences: data_plus/<seq>.npy ----
    paths = [os.path.join(golden_dir, f"data_arap_seq{i}.npy") for i in (0, 1)]
    for kind in ("dir", "lap"):
        ds = datasets.arap_from_files(paths, device=dev, model=kind)
        assert (ds.n, ds.frames, ds.op_frames) == (2, 50, 10) and ds.num_vertices.tolist() == [36, 25]
        seq_ids, offs = np.array([1, 0, 1, 0]), np.array([3, 0, 7, 8])
        b = ds.sample_batch(4, None, seq_ids=seq_ids, offsets=offs)
        nv, nf = 36, int(ds.num_faces.max())
        raw = [datasets.load_arap_sequence(p) for p in paths]
        for i, (s_, o) in enumerate(zip(seq_ids, offs)):                 # operator of the last input frame (main.py:156)
            want = raw[s_][o + 1]["Di" if kind == "dir" else "L"]
            got = (b.Di if kind == "dir" else b.L).to_scipy()
            r0, c0 = (4 * nf * i, 4 * nv * i) if kind == "dir" else (nv * i, nv * i)
            assert abs(got[r0: r0 + want.shape[0], c0: c0 + want.shape[1]] - want).max() == 0
            n = raw[s_][0]["V"].shape[0]
            assert np.array_equal(b.inputs[i, :n, :3].cpu().numpy(), raw[s_][o]["V"]) and np.array_equal(b.targets[i, :n, -3:].cpu().numpy(), raw[s_][o + 41]["V"])
        torch.manual_seed(0)
        model = deterministic_init(arap.DirModel() if kind == "dir" else arap.Model(15), 21).train().to(dev)
        # the same batch through the oracle restatement of the reference model on the CPU torch.sparse path
        o_model = deterministic_init(OB.ArapDirModel() if kind == "dir" else OB.ArapLapModel(15), 21).train()
        cpu = lambda t_: t_.detach().cpu()
        if kind == "dir":
            Dib = OB.diag_cat([OB.sp_to_coo(raw[s_][o + 1]["Di"]) for s_, o in zip(seq_ids, offs)], 4 * nf, 4 * nv)
            DiAb = OB.diag_cat([OB.sp_to_coo(raw[s_][o + 1]["DiA"]) for s_, o in zip(seq_ids, offs)], 4 * nv, 4 * nf)
            o_out = o_model(Dib, DiAb, cpu(b.mask), cpu(b.inputs))
        else:
            Lb = OB.diag_cat([OB.sp_to_coo(raw[s_][o + 1]["L"]) for s_, o in zip(seq_ids, offs)], nv, nv)
            o_out = o_model(Lb, cpu(b.mask), cpu(b.inputs))
        o_loss = OB.arap_loss(o_out, cpu(b.targets), cpu(b.mask), 4)
        loss, out = arap.forward_loss(model, b)
        assert abs(loss.item() - o_loss.item()) <= 2e-4 * abs(o_loss.item()), (kind, loss.item(), o_loss.item())
        opt = arap.make_optimizer(model)
        before = torch.cat([p_.detach().reshape(-1) for p_ in model.parameters()]).clone()
        l1 = arap.train_step(model, opt, b)
        after = torch.cat([p_.detach().reshape(-1) for p_ in model.parameters()])
        assert torch.isfinite(l1) and not torch.equal(before, after)
    # ---- Mesh-MNIST: {train,test}_plus.np ----
    samples = datasets.load_mesh_mnist(os.path.join(golden_dir, "data_mnist_plus.np"))
    for kind, cls in (("lap", mesh_mnist.Model), ("dir", mesh_mnist.DirModel)):
        ds = datasets.mnist_from_samples(samples, device=dev, model=kind)
        b = ds.sample_batch(4, None, ids=np.array([2, 0, 3, 1]))
        assert b.targets.tolist() == [int(samples[i]["label"]) for i in (2, 0, 3, 1)]
        # (stored in the locality numbering — Delaunay vertices arrive in random order: the file's operator, renumbered)
        from surfacenetworks_amd import mesh_ops as _mo

        o = ds.orders[2]
        want = samples[2]["L" if kind == "lap" else "Di"]
        want = _mo.permute_operator(want, o.vorder, o.vorder) if kind == "lap" else _mo.permute_operator(want, o.forder, o.vorder, 4)
        got = (b.L if kind == "lap" else b.Di).to_scipy()
        assert abs(got[: want.shape[0], : want.shape[1]] - want).max() == 0
        model = cls().to(dev)
        opt = mesh_mnist.make_optimizer(model)
        l1 = mesh_mnist.train_step(model, opt, b)
        assert torch.isfinite(l1)
    # ---- FAUST: *.npz frames ----
    p = os.path.join(golden_dir, "data_faust_frame.npz")
    for kind in ("lap", "dir"):
        ds = datasets.faust_from_files([p, p], device=dev, model=kind, pad_to=64)
        torch.manual_seed(1)
        model = deterministic_init(dc.SiameseModel(kind, 15), 13).train().to(dev)
        l_mat = dc.forward_pair_loss(model, ds, 0, 1)
        l_str = dc.forward_pair_loss(model, ds, 0, 1, streamed=True, block=16)
        assert torch.isfinite(l_mat) and abs(l_mat.item() - l_str.item()) <= 2e-5 * abs(l_mat.item())
        opt = dc.make_optimizer(model)
        assert torch.isfinite(dc.train_step(model, opt, ds, 0, 1, streamed=True))


def check_streamed_faust_loss(dev, N=1500, dtype=torch.float32, tol=2e-5):
    """streamed_delta_cross_entropy == loss_fun_delta_cross_entropy(bmm(FA, FB^T)) — value and both gradients — on `dev`
    (main.py:229-240, models.py:203)."""
    from surfacenetworks_amd import dense_correspondence as dc

    g = torch.Generator().manual_seed(0)
    FA = (0.3 * torch.randn(1, N, 120, generator=g, dtype=dtype)).to(dev).requires_grad_(True)
    FB = (0.3 * torch.randn(1, N, 120, generator=g, dtype=dtype)).to(dev).requires_grad_(True)
    GA, GB = torch.rand(N, N, generator=g, dtype=dtype).to(dev), torch.rand(N, N, generator=g, dtype=dtype).to(dev)
    lA, lB = torch.randperm(N, generator=g).to(dev), torch.randperm(N, generator=g).to(dev)
    tX, tY = [(GA, lA, torch.argsort(lA))], [(GB, lB, torch.argsort(lB))]
    ref = dc.loss_fun_delta_cross_entropy(torch.bmm(FA, FB.transpose(1, 2)), tX, tY)
    ref.backward()
    gA, gB = FA.grad.clone(), FB.grad.clone()
    FA.grad = FB.grad = None
    got = dc.streamed_delta_cross_entropy(FA, FB, tX, tY, block=256)
    got.backward()
    assert abs(got.item() - ref.item()) <= tol * abs(ref.item())
    assert rel_err(FA.grad.cpu().numpy(), gA.cpu().numpy()) <= 10 * tol and rel_err(FB.grad.cpu().numpy(), gB.cpu().numpy()) <= 10 * tol


def check_siamese_gradients_meet_once(dev):
    """SiameseModel reads its tower's parameters through two aliases whose gradients are added by one multi-tensor launch
    (dense_correspondence._TwoReaders).  Same parameter gradients as the plain double application of the tower
    (models.py:201-203) followed by autograd's own accumulation — stored (`.grad is None`) and accumulated into existing
    gradients — and the running statistics advance twice either way."""
    import copy

    from surfacenetworks_amd import dense_correspondence as dc

    torch.manual_seed(3)
    ds = dc.TorusBodies(2, n=7, m=9, pad_to=64, seed=5, device=dev)
    model = dc.SiameseModel("lap", 3).to(dev).train()
    plain = copy.deepcopy(model)
    (inX, tX, mX, LX), (inY, tY, mY, LY) = ds.sample(0), ds.sample(1)
    for rounds in (1, 2):                       # second round: gradients already exist and are accumulated into
        out = model(dc._operation(LX, mX), dc._operation(LY, mY), inX, inY)
        dc.loss_fun_delta_cross_entropy(out, tX, tY).backward()
        FA = plain.model(*dc._operation(LX, mX), inX)
        FB = plain.model(*dc._operation(LY, mY), inY)
        dc.loss_fun_delta_cross_entropy(torch.bmm(FA, FB.transpose(1, 2)), tX, tY).backward()
        for (n, a), (_, b) in zip(model.named_parameters(), plain.named_parameters()):
            assert a.grad is not None, n
            if rounds == 1:                     # a + b in both cases
                assert torch.equal(a.grad, b.grad), n
            else:                               # g + (a + b) against (g + a) + b
                assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-6 * float(b.grad.abs().max())), n
    for (n, a), (_, b) in zip(model.named_buffers(), plain.named_buffers()):
        # running statistics and counters: advanced by every application.  On the GPU the second application runs on a side
        # stream and its update is applied after the join from its stored batch statistics (one more fp32 rounding: <= 1 ulp)
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-6 * float(b.abs().max())), (n, float((a - b).abs().max()))
        else:
            assert torch.equal(a, b), n
    with torch.no_grad():                       # no gradients wanted: the plain double application
        o1 = model(dc._operation(LX, mX), dc._operation(LY, mY), inX, inY)
    assert not o1.requires_grad


def check_model_variants(golden_dir, dev, tol=1e-5):
    """The remaining model variants of the three drivers (AvgModel / MlpModel / AmplifyModel and every SiameseModel tower)
    against tests/golden/variants_reference.npz (one forward pass of the imported reference on the two-mesh batch):
      * state_dict keys in the reference's order and parameter counts;
      * the ORACLE composition of the same blocks reproduces the reference's output (pins layer order, heads, wiring);
      * the PRODUCT model agrees with that oracle layer by layer (each layer fed the oracle's input of that layer) and end to
        end.  All in eval mode (running statistics): with batch statistics 15 stacked global-average blocks are chaotic on
        this fixture — one-ulp input noise moves the reference's own output by 50 % — so a train-mode output pins nothing."""
    import torch.nn as nn
    import torch.nn.functional as F

    from surfacenetworks_amd import arap, dense_correspondence as dc, mesh_mnist
    from surfacenetworks_amd.operators import OperatorPool

    z = load(golden_dir, "variants_reference.npz")
    lay = load(golden_dir, "layers_reference.npz")
    order = [str(s_) for s_ in lay["order"]]
    nv = int(lay["nv"])
    mask_c = torch.from_numpy(lay["mask"])
    mask = mask_c.to(dev)
    in6_c, c2_c = torch.from_numpy(lay["inputs6"]), torch.from_numpy(lay["coords"])
    mats = [csr_of(load(golden_dir, f"ops_{m}.npz"), "L") for m in order]
    L = OperatorPool(mats, dev).assemble(np.arange(len(order)), nv, nv)
    L_half = OperatorPool([m_ * np.float32(0.5) for m_ in mats], dev).assemble(np.arange(len(order)), nv, nv)
    Lo = OB.diag_cat([OB.sp_to_coo(m_) for m_ in mats], nv, nv)
    Lo_half = OB.diag_cat([OB.sp_to_coo(m_ * np.float32(0.5)) for m_ in mats], nv, nv)

    class OStack(nn.Module):
        """Oracle restatement of a variant: the same attribute names as the reference class (=> same state_dict order)."""

        def __init__(self, cin, width, blocks, head):
            super().__init__()
            self.conv1 = OB.GraphConv1x1(cin, width, batch_norm=None)
            for i, b in enumerate(blocks):
                self.add_module(f"rn{i}", getattr(OB, b)(width))
            if head == "mnist":
                self.bn_conv2 = OB.GraphConv1x1(width, width, batch_norm="pre")
                self.fc1 = nn.Linear(width, 10)
            elif head == "mlp":
                self.bn = OB.GraphBatchNorm(width)
                self.conv2 = OB.GraphConv1x1(width, 120, batch_norm=None)
            else:
                self.conv2 = OB.GraphConv1x1(width, 120, batch_norm="pre")

    lap_avg = ["LapResNet2" if i % 2 == 0 else "AvgResNet2" for i in range(15)]
    cases = (("arap_avg", arap.AvgModel, 31, (6, 128, ["AvgResNet2"] * 15, "bn"), "in6", None),
             ("arap_mlp", arap.MlpModel, 32, (6, 128, ["MlpResNet2"] * 15, "mlp"), "in6", None),
             ("mnist_avg", mesh_mnist.AvgModel, 33, (3, 64, ["AvgResNet2"] * 5, "mnist"), "c2", None),
             ("mnist_mlp", mesh_mnist.MlpModel, 34, (3, 64, ["MlpResNet2"] * 5, "mnist"), "c2", None),
             ("faust_amp", lambda: dc.AmplifyModel(15), 35, (3, 128, lap_avg, "bn"), "c2", "seq"),
             ("faust_avg", lambda: dc.AvgModel(15), 36, (3, 128, ["AvgResNet2"] * 15, "bn"), "c2", None),
             ("faust_mlp", lambda: dc.MlpModel(15), 37, (3, 128, ["MlpResNet2"] * 15, "mlp"), "c2", None))
    for tag, mk, seed, ospec, inp, opmode in cases:
        m = deterministic_init(mk(), seed)
        assert list(m.state_dict().keys()) == [str(k) for k in z[f"{tag}_keys"]], tag
        assert sum(p_.numel() for p_ in m.parameters()) == int(z[f"{tag}_numel"]), tag
        mo = deterministic_init(OStack(*ospec), seed)
        assert list(mo.state_dict().keys()) == list(m.state_dict().keys())
        mnist = tag.startswith("mnist")
        # running statistics, see make_golden.py (7) for why; the Amplify tower (Laplacian blocks) in train mode
        m, mo = (m.train().to(dev), mo.train()) if tag == "faust_amp" else (m.eval().to(dev), mo.eval())
        x_c = in6_c if inp == "in6" else c2_c
        nblk = len(ospec[2])
        with torch.no_grad():
            xo = mo.conv1(x_c)
            xp = m.conv1(x_c.to(dev))
            assert rel_err(xp.cpu().numpy(), xo.numpy()) <= tol, (tag, "conv1")
            for i in range(nblk):
                op_p = ([L, L_half][min(i // 2, 1)] if opmode == "seq" else None)
                op_o = ([Lo, Lo_half][min(i // 2, 1)] if opmode == "seq" else None)
                xp = m._modules[f"rn{i}"](op_p, mask, xo.to(dev))            # product layer on the ORACLE's input
                xo = mo._modules[f"rn{i}"](op_o, mask_c, xo)
                e = rel_err(xp.cpu().numpy(), xo.numpy())
                assert e <= 2 * tol, (tag, f"rn{i}", e)
            # heads (models.py of each driver): product on the oracle's last activation, and the oracle's own output
            if mnist:
                out_o = F.log_softmax(mo.fc1(OB.masked_mean(F.elu(mo.bn_conv2(F.elu(xo))), mask_c).squeeze(1)), dim=1)
                out_p = m._classify(xo.to(dev), mask)
            elif ospec[3] == "mlp":
                out_o = mo.conv2(F.elu(mo.bn(xo))) + x_c[:, :, -3:].repeat(1, 1, 40)
                out_p = m.conv2(F.elu(m.bn(xo.to(dev)))) + x_c.to(dev)[:, :, -3:].repeat(1, 1, 40)
            else:
                out_o = mo.conv2(F.elu(xo)) + x_c[:, :, -3:].repeat(1, 1, 40)
                out_p = m.conv2(F.elu(xo.to(dev))) + x_c.to(dev)[:, :, -3:].repeat(1, 1, 40)
        # (the train-mode Laplacian tower amplifies the CPU's own summation-order differences between machines: out spread
        # of the comparable arap_lap model 2.7e-4, models_reference.npz)
        tol_o = 2e-3 if tag == "faust_amp" else tol
        assert rel_err(out_o.numpy(), z[f"{tag}_out"]) <= tol_o, (tag, "oracle composition vs reference", rel_err(out_o.numpy(), z[f"{tag}_out"]))
        assert rel_err(out_p.cpu().numpy(), out_o.numpy()) <= 2 * tol, (tag, "head")
        with torch.no_grad():                          # and the product model end to end against the reference's output
            full = m(*{"in6": (None, mask, x_c.to(dev)), "c2": ((x_c.to(dev), None, mask) if mnist else
                                                               (([L, L_half] if opmode == "seq" else None), mask, x_c.to(dev)))}[inp])
        if tag != "faust_amp":       # (train-mode Laplacian tower: conditioned like arap_lap, covered layer by layer above)
            assert rel_err(full.cpu().numpy(), z[f"{tag}_out"]) <= 5 * tol, (tag, "end to end", rel_err(full.cpu().numpy(), z[f"{tag}_out"]))
    for key in ("dir", "amp", "lap", "avg", "mlp"):
        assert list(dc.SiameseModel(key, 15).state_dict().keys()) == [str(k) for k in z[f"siamese_{key}_keys"]], key


def check_packed_model(dev):
    """Whole models on PACKED batches (SURVEY.md §7 "ragged not padded"; no counterpart in the reference, which pads every
    mesh to the batch maximum): inputs (1, sum V_i, C), PackedSegments in place of the mask, packed block-diagonal operators.
      * eval-mode BatchNorm: the packed model equals the padded model on the real rows (padding rows cannot influence real
        rows when no batch statistics are taken), loss included — Dirac and Laplacian ARAP models on a ragged batch;
      * train mode on equally sized meshes (no padding exists): packed == padded in outputs, loss and gradients;
      * the ragged global-average stage's backward against torch autograd on the same composition;
      * one training step on a ragged packed batch runs and changes the parameters."""
    import torch.nn.functional as F

    from surfacenetworks_amd import arap, functional as snF
    from surfacenetworks_amd.operators import PackedSegments

    grids = [(6, 6), (9, 8), (7, 5), (17, 16)]                   # 36, 72, 35, 272 vertices (one mesh spans two 256-row tiles)
    ids, offs = np.array([1, 0, 3, 2, 1]), np.array([0, 1, 1, 0, 1])
    for kind in ("dir", "lap"):
        ds = arap.ClothSequences(grids, frames=45, op_frames=3, seed=1, device=dev, model=kind)
        bp = ds.sample_batch(5, None, seq_ids=ids, offsets=offs, packed=True)
        bd = ds.sample_batch(5, None, seq_ids=ids, offsets=offs)
        assert bp.inputs.shape == (1, int(ds.num_vertices[ids].sum()), 6) and isinstance(bp.mask, PackedSegments)
        assert (bp.Di if kind == "dir" else bp.L).shape[1] == (4 if kind == "dir" else 1) * bp.inputs.shape[1]
        # (eval-mode Laplacian blocks are not normalised — cotangent entries of 1e3..1e4 — so that model keeps 3 layers to stay finite)
        m = deterministic_init(arap.DirModel() if kind == "dir" else arap.Model(3), 3).eval().to(dev)
        with torch.no_grad():
            lp, op_ = arap.forward_loss(m, bp)
            ld_, od = arap.forward_loss(m, bd)
        keep = (bd.mask.reshape(5, -1) > 0).cpu().numpy()
        assert np.isfinite(od.cpu().numpy()).all() and rel_err(op_[0].cpu().numpy(), od.cpu().numpy()[keep]) < 1e-5, kind
        assert abs(lp.item() - ld_.item()) <= 1e-5 * abs(ld_.item())
    # train mode, equal sizes
    ds = arap.ClothSequences([(8, 8)] * 3, frames=45, op_frames=3, seed=2, device=dev, model="dir")
    ids3, offs3 = np.arange(3), np.zeros(3, dtype=np.int64)
    res = []
    for packed in (True, False):
        m = deterministic_init(arap.DirModel(), 4).train().to(dev)
        b = ds.sample_batch(3, None, seq_ids=ids3, offsets=offs3, packed=packed)
        loss, out = arap.forward_loss(m, b)
        loss.backward()
        res.append((loss.item(), out.detach().reshape(-1, 120).cpu().numpy(), grad_signature(m)))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[1][0]) and rel_err(res[0][1], res[1][1]) < 2e-5
    # gradients: the two paths run the global-average stages through different kernels (ragged full-width vs the half-width
    # algebra), i.e. two fp32 evaluation orders of a 15-layer train-mode model whose gradients move by 3.5e-3 of their norm
    # under one-ulp input noise in the reference itself (models_reference.npz: arap_dir_spread_grad)
    assert _sig_err(res[0][2], res[1][2]) < 4e-3, _sig_err(res[0][2], res[1][2])
    # ragged global-average stage: forward and backward against torch autograd
    seg = PackedSegments([5, 300, 17, 64], dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(seg.rows, 128, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(seg.rows, 256, generator=g).to(dev)
    cat = snF.avg_propagate(x, seg)
    (cat * w).sum().backward()
    xr = x.detach().clone().requires_grad_(True)
    e = F.elu(xr)
    means = torch.cat([e[seg.offsets[i]: seg.offsets[i + 1]].mean(0, keepdim=True).expand(int(seg.lengths[i]), -1) for i in range(seg.nseg)])
    ref = torch.cat([e, means], 1)
    (ref * w).sum().backward()
    assert rel_err(cat.detach().cpu().numpy(), ref.detach().cpu().numpy()) < 2e-6
    assert rel_err(x.grad.cpu().numpy(), xr.grad.cpu().numpy()) < 1e-5
    # a training step on the ragged packed batch
    ds = arap.ClothSequences(grids, frames=45, op_frames=3, seed=1, device=dev, model="dir")
    m = deterministic_init(arap.DirModel(), 5).train().to(dev)
    opt = arap.make_optimizer(m)
    before = torch.cat([p_.detach().reshape(-1) for p_ in m.parameters()]).clone()
    l1 = arap.train_step(m, opt, ds.sample_batch(5, None, seq_ids=ids, offsets=offs, packed=True))
    assert torch.isfinite(l1) and not torch.equal(before, torch.cat([p_.detach().reshape(-1) for p_ in m.parameters()]))


def check_inference_mode(golden_dir, dev):
    """A forward under torch.inference_mode(): inference tensors carry no version counter (reading it raises), so the
    activated hand-off between blocks and the per-mask cache must not ask for one.  Same values as under no_grad."""
    from surfacenetworks_amd import arap

    rb, ops = batch_operators(golden_dir, "pool", dev)
    g = load(golden_dir, "models_reference.npz")
    mask = torch.from_numpy(rb["mask"]).to(dev)
    x = torch.from_numpy(g["inputs6"]).to(dev)
    for make, args in ((arap.DirModel, ("Di", "DiA")), (lambda: arap.Model(15), ("L",))):
        # (train-mode BatchNorm: with the fixture's untrained running statistics the 15 cotangent-Laplacian layers overflow)
        m = deterministic_init(make(), 7).train().to(dev)
        with torch.no_grad():
            want = m(*(ops[k] for k in args), mask, x)
        with torch.inference_mode():
            got = m(*(ops[k] for k in args), mask.clone(), x.clone())
        assert torch.isfinite(want).all() and torch.equal(got, want)


def check_faust_amp_tower(golden_dir, dev):
    """The 'amp' tower fed from FAUST files: the operator sequence of main.py:72-83 (D^-1/2 scaling, two squarings) as ONE
    list argument of AmplifyModel.forward (main.py:187-188), forward + backward."""
    import scipy.sparse as sps

    from surfacenetworks_amd import datasets, dense_correspondence as dc

    p = os.path.join(golden_dir, "data_faust_frame.npz")
    fr = datasets.load_faust_frame(p, device=dev)
    seq = dc.amplify_sequence(fr["L"])
    # independent restatement of main.py:72-83 in float64 on dense matrices
    L = fr["L"].astype(np.float64).toarray()
    cnt = np.diff(fr["L"].tocsr().indptr) - 1
    Dm = np.diag(1.0 / np.sqrt(cnt.astype(np.float32)).astype(np.float64))
    cur = Dm @ L @ Dm
    want = [cur]
    for _ in range(2):
        cur = Dm @ cur @ Dm
        cur = cur @ cur
        want.append(cur)
    assert len(seq) == 3
    for got, w in zip(seq, want):
        assert sps.issparse(got) and got.dtype == np.float32
        assert rel_err(got.toarray(), w) <= 5e-6
    ds = datasets.faust_from_files([p, p], device=dev, model="amp", pad_to=64)
    inX, tX, mX, LX = ds.sample(0)
    assert isinstance(LX, dc.LSequence) and len(LX) == 3 and tuple(LX[0].shape) == (64, 64)
    assert len(dc._operation(LX, mX)) == 2                      # [L_sequence, mask]: one positional argument, not splatted
    model = deterministic_init(dc.SiameseModel("amp", 15), 13).train().to(dev)
    loss = dc.forward_pair_loss(model, ds, 0, 1)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(q.grad).all() for q in model.parameters() if q.grad is not None)
    pb = dc.PairBatch(ds, 0, 1)
    assert pb.graph_constants() == (pb.NA, pb.NB) and len(pb.graph_tensors()) > 5
    own = pb.owned()
    assert isinstance(own.LX, dc.LSequence) and own.LX[0].rowptr.data_ptr() != pb.LX[0].rowptr.data_ptr()
