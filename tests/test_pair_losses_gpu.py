"""The `cel` (soft-target cross entropy) and `sl1` (smooth-L1) dense-correspondence losses from the tower features
(sn_pair_soft_* / sn_pair_sl1_*) against src/dense_correspondence/main.py:197-227 restated in float64 on the materialised
score matrix and the materialised `GA[:, pa] + GB[pb, :]`.

Bounds: the project's own for the fused pair loss (tests/test_dense_gpu.py: value 2e-6 relative, gradients rel_err < 5e-6),
derived from the arithmetic (two fp16 pieces = 22+ bits, fp32 accumulation), not from what these kernels give."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUE_BOUND, GRAD_BOUND = 2e-6, 5e-6

from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402

SHAPES = [(7, 7, 7, 120), (80, 63, 70, 120), (33, 33, 1, 5), (300, 257, 290, 128), (1024, 1000, 1021, 64), (7000, 6890, 6890, 120)]


def _case(rows, NA, NB, K, scale, seed):
    """Features (views with a leading dimension larger than the row), two label-order matrices (NA x NB corners of wider
    storage) and a random inverse-permutation pair per side.  In the reference's terms: GA = HA[lA, :] with pa = lB,
    GB = HB[:, lB] with pb = lA, so that GA[:, pa] + GB[pb, :] = (HA + HB)[lA][:, lB]."""
    g = torch.Generator().manual_seed(seed)
    rowsB = rows + 5
    FA = (torch.randn(1, rows, K + 8, generator=g) * 0.7).to(DEV)[:, :, :K].requires_grad_(True)
    FB = (torch.randn(1, rowsB, K + 4, generator=g) * 0.7).to(DEV)[:, :, :K].requires_grad_(True)
    HA = (torch.rand(NA, NB + 12, generator=g) * scale).to(DEV)[:, :NB]
    HB = (torch.rand(NA, NB + 4, generator=g) * scale).to(DEV)[:, :NB]
    lA, lB = torch.randperm(NA, generator=g).to(DEV), torch.randperm(NB, generator=g).to(DEV)
    liA, liB = torch.argsort(lA), torch.argsort(lB)
    assert dc.labels_are_inverse(lA, liA) and dc.labels_are_inverse(lB, liB)
    GA, pa, GB, pb = HA[lA, :], lB, HB[:, lB], lA
    G = GA[:, pa] + GB[pb, :]                                       # fp32 + fp32 (main.py:206,224)
    return FA, FB, HA, HB, liA, liB, G


def _want(name, A64, B64, G, NA, NB):
    """main.py:197-227 in float64 on the materialised bmm and the materialised geodesic sum."""
    S = torch.bmm(A64, B64.transpose(1, 2))
    if name == "cel":                                               # main.py:224-226 (sum of the elementwise products)
        return -(F.softmin(G.double(), dim=1) * F.log_softmax(S[0, :NA, :NB], dim=1)).sum()
    full = torch.zeros_like(S)                                      # main.py:205-206,214
    full[0, :NA, :NB] = G.double()
    return F.smooth_l1_loss(S, full)


def _fused(name):
    return dc.fused_pair_soft_cross_entropy if name == "cel" else dc.fused_pair_smooth_l1


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("rows,NA,NB,K", SHAPES)
@pytest.mark.parametrize("name", ["cel", "sl1"])
def test_fused_pair_loss_matches_the_reference_in_fp64(name, rows, NA, NB, K, scale):
    """Value and both feature gradients; structure of the gradients (cel: exact zeros in the padding rows; sl1: the padding
    rows carry the fp64 gradient); gloss through the backward (x 1.7); two runs bit-identical."""
    FA, FB, HA, HB, liA, liB, G = _case(rows, NA, NB, K, scale, rows + K)
    A64, B64 = FA.detach().double().requires_grad_(True), FB.detach().double().requires_grad_(True)
    want = _want(name, A64, B64, G, NA, NB)
    wa, wb = torch.autograd.grad(want * 1.7, (A64, B64))
    got = _fused(name)(FA, FB, HA, HB, liA, liB, NA, NB)
    ga, gb = torch.autograd.grad(got * 1.7, (FA, FB))
    ev = abs(got.item() - want.item()) / max(abs(want.item()), 1e-300)      # (cel at NB = 1 is identically 0)
    ea, eb = rel_err(ga.cpu().numpy(), wa.cpu().numpy()), rel_err(gb.cpu().numpy(), wb.cpu().numpy())
    print(f"pairloss {name} rows={rows} scale={scale}: value {ev:.2e} dFA {ea:.2e} dFB {eb:.2e}")
    assert abs(got.item() - want.item()) <= VALUE_BOUND * abs(want.item())
    assert ga.shape == FA.shape and gb.shape == FB.shape
    assert ea < GRAD_BOUND and eb < GRAD_BOUND
    if name == "cel":
        assert rows == NA or ga[0, NA:].abs().max().item() == 0
        assert gb[0, NB:].abs().max().item() == 0
    else:
        assert wb[0, NB:].abs().max().item() > 0                    # the padding is scored (main.py:205-214)
        assert rel_err(gb[0, NB:].cpu().numpy(), wb[0, NB:].cpu().numpy()) < GRAD_BOUND
        assert rows == NA or rel_err(ga[0, NA:].cpu().numpy(), wa[0, NA:].cpu().numpy()) < GRAD_BOUND
    got2 = _fused(name)(FA, FB, HA, HB, liA, liB, NA, NB)
    ga2, gb2 = torch.autograd.grad(got2 * 1.7, (FA, FB))
    assert torch.equal(got, got2) and torch.equal(ga, ga2) and torch.equal(gb, gb2)


def _frames(n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        label = torch.randperm(n, generator=g).to(DEV)
        out.append(((torch.rand(n, n, generator=g) * scale).to(DEV), label, torch.argsort(label)))
    return out


@pytest.mark.parametrize("rows,n,scale", [(80, 70, 1.0), (7000, 6890, 30.0)])
@pytest.mark.parametrize("name", ["cel", "sl1"])
def test_the_three_forms_agree(name, rows, n, scale):
    """Fused from the features == the package's loss_fun_* on the materialised (1, N, N) output == the float64 restatement,
    from the reference's target triples (G, label, label_inv); and the masked evaluation form (main.py:352-353) equals the fused
    loss on masked features."""
    tx, ty = _frames(n, scale, rows)
    g = torch.Generator().manual_seed(rows + 1)
    FA, FB = (torch.randn(1, rows, 120, generator=g) * 0.7).to(DEV), (torch.randn(1, rows, 120, generator=g) * 0.7).to(DEV)
    HA, HB = dc.label_order_matrix(tx[0], tx[2]), dc.label_order_matrix(ty[0], ty[2])
    G = tx[0][:, tx[2][ty[1]]] + ty[0][ty[2][tx[1]], :]
    want = _want(name, FA.double(), FB.double(), G, n, n).item()
    fused = _fused(name)(FA, FB, HA, HB, tx[2], ty[2], n, n).item()
    out64 = torch.bmm(FA.double(), FB.double().transpose(1, 2))
    pkg64 = dc.LOSSES[name](out64, [tx], [ty]).item()                   # the package's function, plain-torch branch in float64
    pkg32 = dc.LOSSES[name](torch.bmm(FA, FB.transpose(1, 2)), [tx], [ty]).item()
    print(f"pairloss forms {name} rows={rows}: fused {abs(fused - want) / abs(want):.2e} pkg64 {abs(pkg64 - want) / abs(want):.2e} "
          f"pkg32 (plain fp32 torch) {abs(pkg32 - want) / abs(want):.2e}")
    assert abs(fused - want) <= VALUE_BOUND * abs(want)
    assert abs(pkg64 - want) <= 1e-12 * abs(want)
    # (the plain fp32 torch composition is library code, not this package's: its distance from fp64 is printed, and recorded in
    #  LABNOTES.md#pairlosses as the yardstick the rule of tests/test_dense_gpu.py:120 would use; nothing of ours to assert on it)
    # masked evaluation: outputs * (maskX maskY^T) == scores of masked features
    mX = torch.zeros(1, rows, 1, device=DEV)
    mX[0, :n - 3] = 1
    mY = torch.zeros(1, rows, 1, device=DEV)
    mY[0, :n - 1] = 1
    masked_out = out64 * torch.bmm(mX.double(), mY.double().transpose(1, 2))
    wm = dc.LOSSES[name](masked_out, [tx], [ty]).item()
    gm = _fused(name)(FA * mX, FB * mY, HA, HB, tx[2], ty[2], n, n).item()
    assert abs(gm - wm) <= VALUE_BOUND * abs(wm)


@pytest.mark.parametrize("name", ["cel", "sl1"])
def test_no_score_sized_temporary(name):
    """At 7000 padded / 6890 scored rows, with the label-order matrices resident, fused forward + backward raise the peak
    allocation by less than ONE score matrix (rowsA * rowsB * 4 bytes; the materialised composition holds at least five)."""
    rows, n, K = 7000, 6890, 120
    FA, FB, HA, HB, liA, liB, _ = _case(rows, n, n, K, 3.0, 77)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = _fused(name)(FA, FB, HA, HB, liA, liB, n, n)
    torch.autograd.grad(loss, (FA, FB))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"pairloss peak {name}: {rise / 2**20:.1f} MiB")
    assert rise < rows * (rows + 5) * 4


def test_pair_loss_argument_checks():
    from surfacenetworks_amd import _lib

    lib = _lib.load()
    f = torch.zeros(64, 120, device=DEV)
    H = torch.zeros(64, 64, device=DEV)
    geo = dc.pair_geo_table(H, H)
    o = torch.zeros(128, device=DEV)
    o64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    need = lib.sn_pair_loss_workspace_bytes(64, 64)
    assert need == lib.sn_pair_fused_workspace_bytes(64, 64) + 8 * 64 * 4 * 4          # + the soft-min partials
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = lambda x: x.data_ptr()
    SN_E_NULL, SN_E_SHAPE, SN_E_UNSUPPORTED, SN_E_WORKSPACE = -1, -2, -7, -6
    sf = lambda *a: lib.sn_pair_soft_fwd_f32(*a)
    ok = [p(f), 120, p(f), 120, None, None, p(geo), 64, 64, 64, 64, 64, 64, 120, p(o), p(o), p(ws), need, None]
    assert sf(*ok) == 0
    ch = lambda i, v: [v if j == i else a for j, a in enumerate(ok)]
    assert sf(*ch(9, 65)) == SN_E_SHAPE                       # NA > rowsA
    assert sf(*ch(7, 63)) == SN_E_SHAPE                       # ldgA < NB
    assert sf(*ch(1, 119)) == SN_E_SHAPE                      # lda < K
    assert sf(*(ch(13, 129)[:1] + [200] + ch(13, 129)[2:3] + [200] + ch(13, 129)[4:])) == SN_E_UNSUPPORTED
    assert sf(*ch(17, need - 1)) == SN_E_WORKSPACE
    assert sf(*ch(6, None)) == SN_E_NULL and sf(*ch(0, None)) == SN_E_NULL
    sb = lib.sn_pair_soft_bwd_f32
    assert sb(None, None, p(geo), 64, 64, p(o), p(o), 64, 64, 64, 64, 120, p(f), 120, None, 120, p(ws), need, None) == SN_E_NULL
    assert sb(None, None, p(geo), 64, 64, p(o), p(o), 64, 64, 64, 64, 120, p(f), 119, p(f), 120, p(ws), need, None) == SN_E_SHAPE
    lf = lib.sn_pair_sl1_fwd_f32
    okl = [p(f), 120, p(f), 120, None, None, p(geo), 64, 64, 64, 64, 64, 64, 120, p(o64), p(ws), need, None]
    assert lf(*okl) == 0
    chl = lambda i, v: [v if j == i else a for j, a in enumerate(okl)]
    assert lf(*chl(10, 65)) == SN_E_SHAPE and lf(*chl(16, need - 1)) == SN_E_WORKSPACE and lf(*chl(14, None)) == SN_E_NULL
    lb = lib.sn_pair_sl1_bwd_f32
    assert lb(None, None, p(geo), 64, 64, None, 64, 64, 64, 64, 120, p(f), 120, p(f), 120, p(ws), need, None) == SN_E_NULL
    assert lb(None, None, p(geo), 64, 64, p(o), 64, 64, 64, 64, 129, p(f), 200, p(f), 200, p(ws), need, None) == SN_E_UNSUPPORTED
    torch.cuda.synchronize()


def _datasets(kind):
    if kind == "lap":
        return dc.TorusBodies(3, n=9, m=14, pad_to=160, seed=4, device=DEV)
    from surfacenetworks_amd import datasets

    p = os.path.join(os.path.dirname(__file__), "golden", "data_faust_frame.npz")
    return datasets.faust_from_files([p, p, p], device=DEV, model="dir", pad_to=64)


@pytest.mark.parametrize("kind", ["lap", "dir"])
@pytest.mark.parametrize("name", ["cel", "sl1"])
def test_forward_loss_through_the_model(name, kind):
    """forward_loss on a PairBatch(..., loss=name) == LOSSES[name](model(...), tX, tY), the latter in float64 on the model's
    (1, N, N) output; gradients reach the parameters."""
    from helpers import deterministic_init

    ds = _datasets(kind)
    model = deterministic_init(dc.SiameseModel(kind, 3), 12).to(DEV).train()
    b = dc.PairBatch(ds, 0, 1, loss=name)
    assert b.geo is not None and b.target is None
    got = dc.forward_loss(model, b)
    out = model(dc._operation(b.LX, b.mX), dc._operation(b.LY, b.mY), b.inX, b.inY)
    want = dc.LOSSES[name](out.double(), b.tX, b.tY)
    print(f"pairloss model {name} {kind}: {abs(got.item() - want.item()) / abs(want.item()):.2e}")
    assert got.shape == (1,) and abs(got.item() - want.item()) <= VALUE_BOUND * abs(want.item())
    got.sum().backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())


@pytest.mark.parametrize("name", ["cel", "sl1"])
def test_graph_replay_of_the_pair_step_on_alternating_pairs(name):
    """graphed_train_step on PairBatch(loss=name): three replays on other pairs than the captured one — the geodesic matrices
    reached through the 2-entry address table — bit-identical to the eager step."""
    from surfacenetworks_amd import kernels

    torch.manual_seed(3)
    ds = dc.TorusBodies(3, n=9, m=14, pad_to=160, seed=4, device=DEV)
    model_e = dc.SiameseModel("lap", 3).to(DEV).train()
    model_g = copy.deepcopy(model_e)
    opt_e, opt_g = dc.make_optimizer(model_e), dc.make_optimizer(model_g)
    graphed = dc.graphed_train_step(model_g, opt_g, dc.PairBatch(ds, 0, 1, loss=name))
    for ia, ib in [(1, 2), (2, 0), (1, 0)]:
        for q in model_e.parameters():
            q.grad = None
        le = dc.forward_loss(model_e, dc.PairBatch(ds, ia, ib, loss=name))
        le.backward()
        kernels.clear_absmax()
        opt_e.step()
        pb = dc.PairBatch(ds, ia, ib, loss=name)
        assert graphed.matches(pb)
        lg = graphed(pb)
        assert torch.equal(le.detach(), lg.detach()), (ia, ib, le.item(), lg.item())
        for (nm, pe), pg in zip(model_e.named_parameters(), model_g.parameters()):
            assert torch.equal(pe.detach(), pg.detach()), f"{nm} differs after pair {(ia, ib)}"
    assert not graphed.matches(dc.PairBatch(ds, 0, 1))               # another loss: another capture


@pytest.mark.parametrize("name", ["cel", "sl1"])
def test_the_pair_step_issues_no_library_matrix_product(name, monkeypatch):
    """As tests/test_graph_gpu.py for the delta loss: under SN_STRICT=1 a `cel` / `sl1` pair step (towers, loss, backward) runs
    no aten::mm / bmm / addmm / matmul."""
    from torch.profiler import ProfilerActivity, profile

    monkeypatch.setenv("SN_STRICT", "1")
    torch.manual_seed(5)
    ds = dc.TorusBodies(2, n=8, m=9, pad_to=80, seed=4, device=DEV)
    model = dc.SiameseModel("lap", 15).to(DEV).train()
    dc.forward_loss(model, dc.PairBatch(ds, 0, 1, loss=name)).sum().backward()
    model.zero_grad(set_to_none=True)
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        loss = dc.forward_loss(model, dc.PairBatch(ds, 1, 0, loss=name)).sum()
        loss.backward()
        torch.cuda.synchronize()
    names = {ev.name for ev in prof.events()}
    assert not names & {"aten::mm", "aten::bmm", "aten::addmm", "aten::matmul", "aten::baddbmm", "aten::linear"}, sorted(
        n for n in names if "mm" in n or "linear" in n or "matmul" in n)
    assert torch.isfinite(loss).item()


def test_labels_that_are_not_inverse_fall_back_or_raise(monkeypatch):
    ds = dc.TorusBodies(2, n=8, m=9, pad_to=80, seed=4, device=DEV)
    fr = ds.frames[1]
    fr["label_inv"] = fr["label_inv"].roll(1)
    b = dc.PairBatch(ds, 0, 1, loss="cel")
    assert b.geo is None
    model = dc.SiameseModel("lap", 3).to(DEV).train()
    assert torch.isfinite(dc.forward_loss(model, b)).all()           # the materialised composition
    monkeypatch.setenv("SN_STRICT", "1")
    with pytest.raises(RuntimeError, match="SN_STRICT"):
        dc.forward_loss(model, b)
