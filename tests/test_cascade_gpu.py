"""The cascade model on the device (surfacenetworks_amd/cascade.py) against the float64 restatement of tests/cascade_cases.py,
which tests/test_cascade.py pins to the reference's `EfficientCascade`.

Forward: the model rule (README "Parity"): against float64 on the same inputs the product may be as far off as the fp32 torch
restatement of the same model, times four, and never needs to be closer than 1e-5.
Gradients: max-pool routing is discontinuous, so a float64 comparison of gradients proves nothing at near-ties; the blocks are
held to float64 by tests/block_truth.py, and what is new here — the two pooling kernels inside the model — is held to torch's own
MaxPool1d / interpolate + add in the SAME module: loss, input gradient and every parameter gradient bit-identical."""
import copy

import numpy as np
import pytest
import torch

import cascade_cases as cc
from helpers import deterministic_init

pytestmark = pytest.mark.gpu

DEV = "cuda"
LEVELS = (2, 4)


def _batch(case):
    from surfacenetworks_amd import normal_predict as NP
    from surfacenetworks_amd.operators import SparseOperator

    Laps = [SparseOperator.from_scipy(M, DEV) for M in case["Laps"]]
    return NP.Batch(case["inputs"].to(DEV), case["targets"].to(DEV), case["mask"].to(DEV), None, None, None, [0, 1], Laps=Laps)


@pytest.fixture(scope="module")
def cases():
    return {n: cc.cascade_batch(n) for n in LEVELS}


def _model(levels, seed=17):
    from surfacenetworks_amd import cascade

    return deterministic_init(cascade.LapCascade(3, 3, cascade_levels=levels), seed).train().to(DEV)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("levels", LEVELS)
def test_forward_against_float64(cases, levels):
    """Measured on an MI355X (LABNOTES.md#cascade), product / fp32 restatement: 2 levels 8.3e-6 / 5.1e-6, 4 levels 1.1e-5 / 7.7e-6."""
    case = cases[levels]
    b = _batch(case)
    model = _model(levels)
    state = copy.deepcopy(model.state_dict())
    with torch.no_grad():
        out = model(b.operator, b.mask, b.inputs)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = cc.RefCascade(3, 3, levels)
        m.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
        with torch.no_grad():
            ref[dtype] = m.to(dtype).train()(cc.host_operators(case, dtype), case["mask"].to(dtype), case["inputs"].to(dtype))
    e_prod, e_ref = _rel(out, ref[torch.float64]), _rel(ref[torch.float32], ref[torch.float64])
    print(f"[cascade levels={levels}] outputs: product {e_prod:.2e}, fp32 restatement {e_ref:.2e}")
    assert out.shape == (2, case["V"], 3)
    assert e_prod <= max(1e-5, 4 * e_ref), (levels, e_prod, e_ref)


def _step(model, b):
    from surfacenetworks_amd import normal_predict as NP

    model.zero_grad()
    inputs = b.inputs.detach().clone().requires_grad_(True)
    bb = NP.Batch(inputs, b.targets, b.mask, None, None, None, b.names, Laps=b.Laps)
    out = model(bb.operator, bb.mask, bb.inputs)
    loss = NP.cosine_loss(out, bb.mask, bb.targets)
    loss.backward()
    return [loss.detach().clone(), out.detach().clone(), inputs.grad.clone()] + [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("levels", LEVELS)
def test_gradients_equal_the_same_module_with_torch_pooling(cases, levels):
    b = _batch(cases[levels])
    model = _model(levels)
    twin = copy.deepcopy(model)
    twin.down_pool, twin.up_pool_add = cc.torch_pool, cc.torch_unpool_add
    got, want = _step(model, b), _step(twin, b)
    names = ["loss", "outputs", "input gradient"] + [k for k, _ in model.named_parameters()]
    for name, a, c in zip(names, got, want):
        assert torch.equal(a, c), (levels, name)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert float(got[2].abs().max()) > 0 and float(got[3].abs().max()) > 0
    for (_, p), (_, q) in zip(model.named_buffers(), twin.named_buffers()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("levels", LEVELS)
def test_strict_mode_finds_no_library_gemm_and_the_loss_goes_down(cases, levels, monkeypatch):
    """SN_STRICT=1 raises nowhere in the step at these shapes (the coarsest level of the 4-level case has 2 x 12 rows), and a few
    Adam steps on one batch lower the loss."""
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd import normal_predict as NP

    monkeypatch.setattr(snF, "_STRICT", True)
    b = _batch(cases[levels])
    model = _model(levels, seed=29)
    opt = NP.make_optimizer(model)
    losses = [float(NP.train_step(model, opt, b)[0].detach()) for _ in range(8)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


@pytest.mark.parametrize("levels", LEVELS)
def test_three_graph_replays_equal_three_eager_steps(cases, levels):
    from surfacenetworks_amd import normal_predict as NP

    model_e = _model(levels)
    model_g = copy.deepcopy(model_e)
    opt_e, opt_g = NP.make_optimizer(model_e), NP.make_optimizer(model_g)
    graphed = NP.graphed_train_step(model_g, opt_g, _batch(cases[levels]))
    # the replays run on OTHER batches of the captured shape (the same sparsity, other operator values on every level, other
    # inputs), so a level whose arrays were not among the graph's inputs, or not reloaded, would replay the example's operator
    def variant(case, k):
        return dict(case, Laps=[(M * np.float32(1 + 0.25 * k)).astype(np.float32) for M in case["Laps"]],
                    inputs=case["inputs"] * (1 - 0.125 * k))

    others = [variant(cases[levels], k) for k in (1, 2)]
    for step, case in enumerate((others[0], others[1], cases[levels])):
        be, bg = _batch(case), _batch(case)
        assert graphed.matches(bg)
        le, _ = NP.train_step(model_e, opt_e, be)
        lg = graphed(bg)
        assert torch.equal(le.detach(), lg.detach()), (levels, step)
        for (name, pe), pg in zip(model_e.named_parameters(), model_g.parameters()):
            assert torch.equal(pe.grad, pg.grad), (levels, name, step)
            assert torch.equal(pe.detach(), pg.detach()), (levels, name, step)
    for be_, bg_ in zip(model_e.buffers(), model_g.buffers()):
        assert torch.equal(be_, bg_)
    other = _batch(cc.cascade_batch(levels, sizes=((5, 4), (6, 5))))
    assert not graphed.matches(other)                     # another padded size: every level's operator has another shape


def test_forward_loss_evaluation_and_fuzzy_load(cases):
    """forward_loss takes the model unchanged (the padded head and the residual frame go to the loss kernel): the same bits as
    model(...) followed by cosine_loss(...); a checkpoint in the reference's layout loads."""
    from surfacenetworks_amd import normal_predict as NP

    b = _batch(cases[4])
    model = _model(4)
    twin = copy.deepcopy(model)
    loss, mad, out = NP.forward_loss(model, b)
    out2 = twin(b.operator, b.mask, b.inputs)
    assert torch.equal(out, out2) and torch.equal(loss, NP.cosine_loss(out2, b.mask, b.targets))
    assert torch.equal(mad, NP.mean_angle_deviation(out2, b.mask, b.targets))
    # the mask of these cases is no prefix of the node axis (fake nodes between real ones): the loss kernels select its rows as
    # the plain-torch statement does on the host.  Both are means of per-row values in [0, 1] and [0, pi / 2] whose fp32
    # expressions carry at most 19 roundings each (LABNOTES.md#normals): 1e-5 covers both sides with room to spare.
    m0 = b.mask[:, :, 0].cpu()
    assert not any(bool(m0[i, :int(m0[i].sum())].all()) for i in range(2))
    assert abs(float(loss.detach()) - float(NP.loss_reference(out.cpu(), b.mask.cpu(), b.targets.cpu()))) <= 1e-5
    assert abs(float(mad) - float(NP.mad_reference(out.cpu(), b.mask.cpu(), b.targets.cpu()))) <= 1e-5
    src = deterministic_init(cc.RefCascade(3, 3, 4), 23).double()
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in src.state_dict().items()}
    for how in ("load_state_dict", "fuzzy_load"):
        m = _model(4, seed=1)
        getattr(m, how)(sd)
        assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())


# ---- the sampler: hierarchies from frame["L"], one pool per level, position order ------------------------------------------------
def _cas_meshes():
    from surfacenetworks_amd import mesh_ops

    rng = np.random.default_rng(21)
    return [mesh_ops.grid_cloth(9, 8, rng), mesh_ops.torus_grid(10, 9, rng), mesh_ops.grid_cloth(6, 5, rng)]


@pytest.fixture(scope="module")
def cas_frames():
    from surfacenetworks_amd import normal_predict as NP

    return {mass: NP.NormalFrames.from_meshes(_cas_meshes(), model="cas", device=DEV, levels=4, mass=mass) for mass in (None, "barycentric")}


@pytest.mark.parametrize("mass", [None, "barycentric"])
def test_the_cas_batch_equals_a_hand_assembled_one(cas_frames, mass):
    """Per frame the numpy statement of the hierarchy on the frame's own L (and the device's vertex mass); level k padded to
    2^k max n_0 of the batch behind each mesh's own nodes; inputs and targets by position, zero rows at fake nodes; the mask
    is the real-node mask of the finest level and no prefix; to_mesh_order brings the rows back."""
    import scipy.sparse as sp

    from surfacenetworks_amd import mesh_ops, operators
    from surfacenetworks_amd import normal_predict as NP
    from surfacenetworks_amd.datasets import normal_frame_from_mesh

    ds = cas_frames[mass]
    frames = [normal_frame_from_mesh(V, F_, model="lap", device=DEV, name=i) for i, (V, F_) in enumerate(_cas_meshes())]
    hs = []
    for fr in frames:
        m = None if mass is None else operators.vertex_mass(fr["V"], fr["F"], mass).cpu().numpy()
        hs.append(mesh_ops.mesh_hierarchy(fr["L"].to_scipy(), levels=4, mass=m))
    for ids in ([0, 1], [2, 0], [1], [2, 1, 0]):
        b = ds.sample_batch(len(ids), ids=ids)
        n0 = max(hs[i].L[0].shape[0] for i in ids)
        assert b.L is None and len(b.Laps) == 4 and b.operator is b.Laps and b.names == list(ids)
        for k in range(4):
            size = n0 << k
            blocks = []
            for i in ids:
                M = hs[i].L[k].tocoo()
                blocks.append(sp.coo_matrix((M.data, (M.row, M.col)), shape=(size, size)))
            want = sp.block_diag(blocks, format="csr")
            got = b.Laps[k].to_scipy()
            assert got.shape == want.shape and got.nnz == want.nnz and abs(got - want).max() == 0, (ids, k)
        nodes = n0 << 3
        assert b.inputs.shape == (len(ids), nodes, 3) and b.targets.shape == (len(ids), nodes, 3) and b.mask.shape == (len(ids), nodes, 1)
        for j, i in enumerate(ids):
            pos = torch.from_numpy(hs[i].position)
            inp, tgt, msk = torch.zeros(nodes, 3), torch.zeros(nodes, 3), torch.zeros(nodes)
            inp[pos], tgt[pos], msk[pos] = frames[i]["input"].cpu(), frames[i]["target_dist"].cpu().reshape(-1, 3), 1.0
            assert torch.equal(b.inputs[j].cpu(), inp) and torch.equal(b.targets[j].cpu(), tgt) and torch.equal(b.mask[j, :, 0].cpu(), msk)
            assert torch.equal(b.positions[j].cpu(), pos)
            assert not bool(msk[:int(msk.sum())].all())                                  # no prefix
        back = NP.to_mesh_order(b, b.inputs)
        for j, i in enumerate(ids):
            assert torch.equal(back[j], frames[i]["input"])
    with pytest.raises(ValueError, match="positions"):
        NP.to_mesh_order(NP.Batch(b.inputs, b.targets, b.mask, None, None, None, b.names, Laps=b.Laps), b.inputs)


def test_the_cascade_trains_on_sampled_batches(cas_frames, monkeypatch):
    """SN_STRICT=1 raises nowhere on a sampled 4-level batch (real hierarchy, 3 meshes), Adam lowers the loss, three graph replays
    on batches of the captured shape equal eager steps, predict returns every mesh in vertex order."""
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd import normal_predict as NP

    monkeypatch.setattr(snF, "_STRICT", True)
    ds = cas_frames["barycentric"]
    b = ds.sample_batch(3, ids=[0, 1, 2])
    model = _model(4, seed=29)
    opt = NP.make_optimizer(model)
    losses = [float(NP.train_step(model, opt, b)[0].detach()) for _ in range(8)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    model_e = _model(4)
    model_g = copy.deepcopy(model_e)
    opt_e, opt_g = NP.make_optimizer(model_e), NP.make_optimizer(model_g)
    graphed = NP.graphed_train_step(model_g, opt_g, ds.sample_batch(3, ids=[0, 1, 2]))
    for step in range(3):
        be, bg = ds.sample_batch(3, ids=[0, 1, 2]), ds.sample_batch(3, ids=[0, 1, 2])
        assert graphed.matches(bg)
        le, _ = NP.train_step(model_e, opt_e, be)
        lg = graphed(bg)
        assert torch.equal(le.detach(), lg.detach()), step
        for pe, pg in zip(model_e.parameters(), model_g.parameters()):
            assert torch.equal(pe.grad, pg.grad) and torch.equal(pe.detach(), pg.detach()), step
    found = NP.predict(model_e, ds, 3)
    assert [n for n, _ in found] == [0, 1, 2] and [tuple(o.shape) for _, o in found] == [(int(v), 3) for v in ds.nv]


def test_forward_and_gradients_on_a_sampled_batch(cas_frames):
    """The two model checks above on a NormalFrames(model="cas") batch of three meshes (real hierarchy, barycentric restriction
    weights, 4 levels): outputs within the parity rule of the float64 restatement; loss and every gradient bit-identical to the
    same module with torch's pooling.  Measured on an MI355X: product 5.7e-5, fp32 restatement 2.7e-5 (the coarsest level of the smallest mesh
    has a handful of real nodes: BatchNorm statistics there are less well conditioned than on the larger cases above)."""
    from oracle import ref_blocks as OB

    b = cas_frames["barycentric"].sample_batch(3, ids=[0, 1, 2])
    model = _model(4)
    state = copy.deepcopy(model.state_dict())
    with torch.no_grad():
        out = model(b.operator, b.mask, b.inputs)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = cc.RefCascade(3, 3, 4)
        m.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
        Laps = [OB.sp_to_coo(L.to_scipy().astype(np.float64)).coalesce().to(dtype) for L in b.Laps]
        with torch.no_grad():
            ref[dtype] = m.to(dtype).train()(Laps, b.mask.cpu().to(dtype), b.inputs.cpu().to(dtype))
    e_prod, e_ref = _rel(out, ref[torch.float64]), _rel(ref[torch.float32], ref[torch.float64])
    print(f"[cascade sampled batch] outputs: product {e_prod:.2e}, fp32 restatement {e_ref:.2e}")
    assert e_prod <= max(1e-5, 4 * e_ref), (e_prod, e_ref)
    twin = copy.deepcopy(model)
    twin.down_pool, twin.up_pool_add = cc.torch_pool, cc.torch_unpool_add
    for a, c in zip(_step(model, b), _step(twin, b)):
        assert torch.equal(a, c)
