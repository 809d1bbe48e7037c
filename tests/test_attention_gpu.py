"""Graph attention on the device (surfacenetworks_amd/attention.py over csrc/sn_attention.hip) against
attention.attn_propagate_reference evaluated in float64 on the host (tests/attention_cases.py; tests/test_attention.py pins that
statement to an independent dense one).

The bound, per tensor:   max |dev - f64| <= 4 max(max |cpu32 - f64|, 2^-23 max |f64|),
cpu32 the same statement in fp32 on the host: four times the reference's own fp32 error (README, "Parity"), floored at one ulp of
the tensor's largest entry.  Every test prints the ratio of the device's error to that bound before it asserts.

Measured on an MI355X (LABNOTES.md#attention has the table), operands as seeded here: the worst ratio error / bound over the 40
kernel cases is 0.42 for p (batch3, C = 128, H = 1, large scores), 0.70 for x.grad (random, C = 128, H = 1, large scores) and 0.54
for a.grad (cloth, C = 16, H = 1, large scores); the block's tensors stay at 0.06 - 0.27; the model's outputs are 2.4e-6 off
float64 against 2.1e-6 for the fp32 restatement, its worst gradient 1.7e-5 against 3.6e-5."""
import copy

import numpy as np
import pytest
import torch

import attention_cases as ac
from helpers import deterministic_init

pytestmark = pytest.mark.gpu

DEV = "cuda"
PATTERNS = ("cloth", "batch3", "fan", "random")
TORI = ((8, 6), (10, 7), (12, 9))


@pytest.fixture(scope="module")
def batch3():
    """The padded block-diagonal batch of three cloths, assembled through OperatorPool: the padded rows are empty."""
    from surfacenetworks_amd.operators import OperatorPool

    mats = [ac.cloth_laplacian(n, m, seed=5 + i) for i, (n, m) in enumerate(ac.CLOTHS)]
    nv = max(M.shape[0] for M in mats)
    op = OperatorPool(mats, torch.device(DEV)).assemble(np.arange(3), nv, nv)
    M = op.to_scipy().tocsr()
    assert M.shape == (3 * nv, 3 * nv) and (np.diff(M.indptr)[30:nv] == 0).all() and M.nnz == sum(m.nnz for m in mats)
    return op, M


_cases = {}


def _case(pattern, C, H, large, batch3):
    """(device operator, host case): the operands and the host evaluations, computed once per case and left unchanged."""
    from surfacenetworks_amd.operators import SparseOperator

    key = (pattern, C, H, large)
    if key not in _cases:
        if pattern == "batch3":
            _cases[key] = (batch3[0], ac.reference(batch3[1], C, H, large, seed=4))
        else:
            ref = ac.host_case(pattern, C, H, large)
            _cases[key] = (SparseOperator.from_scipy(ref["M"], torch.device(DEV)), ref)
    return _cases[key]


def _run(op, ref, H, g=None):
    from surfacenetworks_amd import attention

    x = ref["x"].to(DEV).requires_grad_(True)
    a = ref["a"].to(DEV).requires_grad_(True)
    cat = attention.attn_propagate(op, x, a, H)
    cat.backward((ref["g"] if g is None else g).to(DEV))
    return cat.detach(), x.grad, a.grad


def _held(figures, name, dev, cpu32, f64):
    assert bool(torch.isfinite(dev).all()), name
    r = ac.ratio(dev, cpu32, f64)
    figures.append(f"{name} {r:.3f}")
    return r <= 1.0


@pytest.mark.parametrize("large", [False, True], ids=["unit", "large_scores"])
@pytest.mark.parametrize("C,H", ac.WIDTHS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_forward_and_backward_within_the_bound(pattern, C, H, large, batch3):
    """cat[:, :C] is the library's ELU of x bit for bit (kernels.elu_into: the expression lap_propagate writes there) and within
    the bound of the float64 statement; p, x.grad and a.grad within the bound; with `large` the scores reach |s| = 100, where an
    unshifted exp overflows fp32."""
    from surfacenetworks_amd import kernels

    op, ref = _case(pattern, C, H, large, batch3)
    cat, dx, da = _run(op, ref, H)
    (c64, dx64, da64), (c32, dx32, da32) = ref["f64"], ref["f32"]
    if large:
        R = ref["x"].shape[0]
        eh = torch.nn.functional.elu(ref["x"].double()).reshape(R, H, C // H)
        assert float((eh * ref["a"][0].double().reshape(1, H, -1)).sum(-1).abs().max()) > 88.0 or \
            float((eh * ref["a"][1].double().reshape(1, H, -1)).sum(-1).abs().max()) > 88.0
    e_lib = torch.empty(ref["x"].shape, device=DEV)
    kernels.elu_into(ref["x"].to(DEV), e_lib)
    figures, ok = [], []
    try:
        assert cat.shape == (ref["x"].shape[0], 2 * C)
        assert torch.equal(cat[:, :C], e_lib)
        assert torch.equal(cat[:, :C], torch.nn.functional.elu(ref["x"].to(DEV)))      # (torch's own ELU on the device: the same bits)
        ok.append(_held(figures, "e", cat[:, :C], c32[:, :C], c64[:, :C]))
        ok.append(_held(figures, "p", cat[:, C:], c32[:, C:], c64[:, C:]))
        ok.append(_held(figures, "dx", dx, dx32, dx64))
        ok.append(_held(figures, "da", da, da32, da64))
    finally:
        print(f"[attn {pattern} C={C} H={H} {'large' if large else 'unit'}] error / bound: " + ", ".join(figures))
    assert all(ok), figures


@pytest.mark.parametrize("C,H", ac.WIDTHS)
@pytest.mark.parametrize("pattern", ("batch3", "random"))
def test_rows_that_take_part_in_nothing_are_exactly_zero(pattern, C, H, batch3):
    """Rows with no stored entry and no entry in their column — every padded vertex of the batch, index 7 of the random pattern:
    p is exactly zero there, and with an upstream gradient on the p half alone so is x.grad (with both halves x.grad there is the
    ELU half's own term, which the first test bounds); a row that is only empty still has p = 0."""
    op, ref = _case(pattern, C, H, False, batch3)
    idle = torch.from_numpy(ac.idle_rows(ref["M"]))
    empty = torch.from_numpy(np.flatnonzero(np.diff(ref["M"].indptr) == 0))
    assert idle.numel() >= 1 and empty.numel() >= idle.numel()
    g = ref["g"].clone()
    g[:, :C] = 0
    cat, dx, da = _run(op, ref, H, g)
    assert not cat[empty.to(DEV), C:].any()
    assert not dx[idle.to(DEV)].any()
    assert bool(dx.abs().sum() > 0) and bool(da.abs().sum() > 0)
    # the rows of a that a head does not own get nothing from another head: a.grad is dense, so only finiteness is asked here
    assert bool(torch.isfinite(da).all())


@pytest.mark.parametrize("C,H", ((16, 4), (128, 8)))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_two_runs_and_a_rebuilt_transpose_give_the_same_bits(pattern, C, H, batch3):
    op, ref = _case(pattern, C, H, False, batch3)
    first = _run(op, ref, H)
    second = _run(op, ref, H)
    op._t = None                                                     # drop the cached transpose: the next backward rebuilds it
    third = _run(op, ref, H)
    assert op._t is not None
    for name, a, b, c in zip(("cat", "dx", "da"), first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c), (pattern, name)


def test_the_values_of_the_operator_are_never_read():
    from surfacenetworks_amd.operators import SparseOperator

    ref = ac.host_case("cloth", 128, 8, False)
    op = SparseOperator.from_scipy(ref["M"], torch.device(DEV))
    want = _run(op, ref, 8)
    poisoned = SparseOperator.from_scipy(ref["M"], torch.device(DEV))
    poisoned.vals.fill_(float("nan"))
    poisoned.t().vals.fill_(float("nan"))
    got = _run(poisoned, ref, 8)
    for name, a, b in zip(("cat", "dx", "da"), want, got):
        assert torch.equal(a, b), name


def test_refusals_on_the_device_path():
    from surfacenetworks_amd import attention
    from surfacenetworks_amd.operators import SparseOperator
    import scipy.sparse as sp

    ref = ac.host_case("cloth", 16, 4, False)
    op = SparseOperator.from_scipy(ref["M"], torch.device(DEV))
    x, a = ref["x"].to(DEV), ref["a"].to(DEV)
    with pytest.raises(ValueError):
        attention.attn_propagate(op, x[:, :6].contiguous(), a[:, :6].contiguous(), 1)            # C = 6
    with pytest.raises(ValueError):
        attention.attn_propagate(op, x, a, 8)                                                    # (C / H) % 4 != 0
    with pytest.raises(ValueError):
        attention.attn_propagate(op, x, a, 3)                                                    # C % H != 0
    wide = SparseOperator.from_scipy(sp.csr_matrix(ref["M"][:, :].tocsr()[:100]), torch.device(DEV))      # 100 x 108
    assert wide.shape[0] != wide.shape[1]
    with pytest.raises(ValueError):
        attention.attn_propagate(wide, x, a, 4)
    with pytest.raises(ValueError):
        attention.attn_propagate(wide, x[:100], a, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        attention.attn_propagate(op, ref["x"], ref["a"], 4)


# ---- the block -----------------------------------------------------------------------------------------------------------------------
def _rel(a, b, top=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()) if top is None else top, 1e-30)


def test_block_on_the_padded_batch_against_the_float64_module(batch3):
    """GatResNet2(128) in training mode: the output and every parameter gradient against the float64 module built from the
    reference statement, tensor by tensor under the bound above; a tensor that BatchNorm's 1 / sigma amplifies beyond it is held to
    four times the error of the fp32 module instead (never closer than 1e-5 of the largest entry), the rule
    tests/test_normal_predict_gpu.py applies to whole models."""
    from surfacenetworks_amd import attention

    op, M = batch3
    host = ac.host_operator(M)
    nv = M.shape[0] // 3
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(3, nv, 128, generator=gen)
    for b, (n, m) in enumerate(ac.CLOTHS):
        x[b, n * m:] = 0                                             # the padded vertices carry zeros, as in a sampled batch
    gout = torch.randn(3, nv, 128, generator=gen)
    blk = deterministic_init(attention.GatResNet2(128), 31).train().to(DEV)
    state = copy.deepcopy(blk.state_dict())
    xd = x.to(DEV).requires_grad_(True)
    out = blk(op, None, xd)
    out.backward(gout.to(DEV))
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = ac.RefGatResNet2(128)
        m.load_state_dict({k: v.cpu() for k, v in state.items()})
        m = m.to(dtype).train()
        xr = x.to(dtype).clone().requires_grad_(True)
        o = m(host, None, xr)
        o.backward(gout.to(dtype))
        ref[dtype] = {"out": o.detach(), "x.grad": xr.grad, **{k: p.grad for k, p in m.named_parameters()}}
    got = {"out": out, "x.grad": xd.grad, **{k: p.grad for k, p in blk.named_parameters()}}
    f64, f32 = ref[torch.float64], ref[torch.float32]
    top = max(float(f64[k].abs().max()) for k in f64 if k not in ("out", "x.grad"))
    figures, bad = [], []
    for k in f64:
        r = ac.ratio(got[k], f32[k], f64[k])
        scale = None if k in ("out", "x.grad") else top
        e_dev, e_32 = _rel(got[k], f64[k], scale), _rel(f32[k], f64[k], scale)
        figures.append(f"{k}: ratio {r:.2f}, device {e_dev:.2e}, fp32 module {e_32:.2e}")
        if not (r <= 1.0 or e_dev <= max(1e-5, 4 * e_32)):
            bad.append(figures[-1])
    print("[GatResNet2] " + "; ".join(figures))
    assert not bad, bad
    assert all(k in got for k in ("att0", "att1")) and bool(got["att0"].abs().sum() > 0) and bool(got["att1"].abs().sum() > 0)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tori():
    from surfacenetworks_amd import mesh_ops
    from surfacenetworks_amd import normal_predict as NP

    rng = np.random.default_rng(3)
    return NP.NormalFrames.from_meshes([mesh_ops.torus_grid(n, m, rng) for n, m in TORI], model="lap", device=DEV)


def _model(seed=17, layers=3):
    from surfacenetworks_amd import attention

    return deterministic_init(attention.LapGatModel(3, 3, layers=layers), seed).train().to(DEV)


def _tori_batch(tori):
    return tori.sample_batch(3, ids=[0, 1, 2])


def test_model_loss_and_gradients_against_float64(tori):
    """The rule of tests/test_normal_predict_gpu.py: err(product) <= max(1e-5, 4 err(fp32 restatement)), errors relative to the
    largest entry of the float64 tensor (parameter gradients: of the model's largest gradient entry)."""
    from surfacenetworks_amd import normal_predict as NP

    b = _tori_batch(tori)
    model = _model()
    state = copy.deepcopy(model.state_dict())
    loss, mad, out = NP.forward_loss(model, b)
    loss.backward()
    host = ac.host_operator(b.L.to_scipy())
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = ac.RefLapGat(3, 3, 3)
        m.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
        m = m.to(dtype).train()
        o = m(host, b.mask.cpu().to(dtype), b.inputs.cpu().to(dtype))
        l = NP.loss_reference(o, b.mask.cpu(), b.targets.cpu().to(dtype))
        a = NP.mad_reference(o, b.mask.cpu(), b.targets.cpu().to(dtype))
        l.backward()
        ref[dtype] = (o.detach(), l.detach(), a.detach(), {k: p.grad for k, p in m.named_parameters()})
    (o64, l64, a64, g64), (o32, l32, a32, g32) = ref[torch.float64], ref[torch.float32]
    figures, bad = [], []

    def held(name, got, r32, truth, top=None):
        e_prod, e_ref = _rel(got, truth, top), _rel(r32, truth, top)
        figures.append(f"{name}: product {e_prod:.2e}, fp32 restatement {e_ref:.2e}")
        if not e_prod <= max(1e-5, 4 * e_ref):
            bad.append(figures[-1])

    assert out.shape == o64.shape == (3, b.inputs.shape[1], 3)
    held("outputs", out, o32, o64)
    held("loss", loss, l32, l64)
    held("mad", mad, a32, a64)
    top = max(float(g.abs().max()) for g in g64.values())
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == g64[k].shape, k
        held(f"grad {k}", p.grad, g32[k], g64[k], top)
    print("[LapGatModel] " + "; ".join(figures[:3]) + "; worst gradient: " +
          max(figures[3:], key=lambda s: float(s.split("product ")[1].split(",")[0])))
    assert not bad, bad
    assert all(bool(model._modules[f"rn{i}"]._parameters[n].grad.abs().sum() > 0) for i in (0, 2) for n in ("att0", "att1"))


def test_strict_mode_finds_no_library_gemm(tori, monkeypatch):
    from surfacenetworks_amd import functional as snF
    from surfacenetworks_amd import normal_predict as NP

    monkeypatch.setattr(snF, "_STRICT", True)
    b = _tori_batch(tori)
    model = _model()
    loss, mad = NP.train_step(model, NP.make_optimizer(model), b)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(mad))
    out = model(b.operator, b.mask, b.inputs)
    NP.cosine_loss(out, b.mask, b.targets).backward()
    assert out.shape == (3, b.inputs.shape[1], 3)


def test_three_graph_replays_equal_three_eager_steps(tori):
    from surfacenetworks_amd import normal_predict as NP

    model_e = _model()
    model_g = copy.deepcopy(model_e)
    opt_e, opt_g = NP.make_optimizer(model_e), NP.make_optimizer(model_g)
    graphed = NP.graphed_train_step(model_g, opt_g, _tori_batch(tori))
    for step in range(3):
        be, bg = _tori_batch(tori), _tori_batch(tori)
        assert graphed.matches(bg)
        le, _ = NP.train_step(model_e, opt_e, be)
        lg = graphed(bg)
        assert torch.equal(le.detach(), lg.detach()), step
        for (name, pe), pg in zip(model_e.named_parameters(), model_g.parameters()):
            assert torch.equal(pe.grad, pg.grad), (name, step)
            assert torch.equal(pe.detach(), pg.detach()), (name, step)
    for be_, bg_ in zip(model_e.buffers(), model_g.buffers()):
        assert torch.equal(be_, bg_)


def test_evaluate_and_predict_run_the_model_unchanged(tori):
    from surfacenetworks_amd import normal_predict as NP

    model = _model()
    got = NP.evaluate(model, tori, 3)
    assert bool(torch.isfinite(got["loss"])) and bool(torch.isfinite(got["mad"]))
    found = NP.predict(model, tori, 3)
    assert [n for n, _ in found] == [0, 1, 2]
    assert all(o.shape == (n * m, 3) and bool(torch.isfinite(o).all()) for (_, o), (n, m) in zip(found, TORI))


def test_thirty_adam_steps_lower_the_loss(tori):
    from surfacenetworks_amd import normal_predict as NP

    torch.manual_seed(0)
    model = _model(seed=29)
    opt = NP.make_optimizer(model)
    losses = [float(NP.train_step(model, opt, _tori_batch(tori))[0].detach()) for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
