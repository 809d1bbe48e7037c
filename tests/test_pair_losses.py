"""Host part of the `cel` / `sl1` dense-correspondence losses (src/dense_correspondence/main.py:197-227): the reference's
names and dispatch table, the plain-torch branch of loss_fun_cross_entropy / loss_fun_sl1 against the formulas restated here
in float64, and the inverse-permutation check the label-order store rests on.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from surfacenetworks_amd import dense_correspondence as dc


def _frame(n, g, scale=3.0):
    label = torch.randperm(n, generator=g)
    return (torch.rand(n, n, generator=g, dtype=torch.float64) * scale, label, torch.argsort(label))


def _G(tx, ty):
    (GA, lA, liA), (GB, lB, liB) = tx, ty
    return GA[:, liA[lB]] + GB[liB[lA], :]                      # main.py:206,224


def test_losses_table_has_the_three_keys_of_the_reference():
    assert set(dc.LOSSES) == {"sl1", "cel", "dcel"}             # main.py:46
    assert dc.LOSSES["sl1"] is dc.loss_fun_sl1 and dc.LOSSES["cel"] is dc.loss_fun_cross_entropy
    assert dc.LOSSES["dcel"] is dc.loss_fun_delta_cross_entropy


def test_cross_entropy_is_a_sum_over_rows_of_sample_zero():
    """main.py:216-227: -sum(softmin(G) * log_softmax(outputs[0, :NA, :NB])) per pair (a sum, not a mean), over the batch
    size; outputs[0] is scored for every i."""
    g = torch.Generator().manual_seed(1)
    N, n = 13, 11
    out = torch.randn(2, N, N, generator=g, dtype=torch.float64, requires_grad=True)
    tX, tY = [_frame(n, g), _frame(n, g)], [_frame(n, g), _frame(n, g)]
    want = 0.0
    for i in range(2):
        t = torch.softmax(-_G(tX[i], tY[i]), dim=1)
        want = want - (t * torch.log_softmax(out[0, :n, :n], dim=1)).sum()
    want = want / 2
    got = dc.loss_fun_cross_entropy(out, tX, tY)
    assert got.shape == (1,) and abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    (gg,) = torch.autograd.grad(got.sum(), out)
    assert gg[1].abs().max().item() == 0 and gg[0, n:].abs().max().item() == 0 and gg[0, :, n:].abs().max().item() == 0
    # a mean over the rows would be n times smaller
    mean_form = sum(F.cross_entropy(out[0, :n, :n], torch.softmax(-_G(tX[i], tY[i]), dim=1)) for i in range(2)) / 2
    assert abs(got.item() - n * mean_form.item()) <= 1e-10 * abs(got.item())


def test_smooth_l1_scores_the_padding_against_zero():
    """main.py:197-214: mean over ALL entries of smooth_l1(outputs - FullG), FullG zero outside the corner, over the batch size."""
    g = torch.Generator().manual_seed(2)
    N, n = 12, 9
    out = (2 * torch.randn(2, N, N, generator=g, dtype=torch.float64)).requires_grad_(True)
    tX, tY = [_frame(n, g), _frame(n, g)], [_frame(n, g), _frame(n, g)]
    full = torch.zeros(2, N, N, dtype=torch.float64)
    for i in range(2):
        full[i, :n, :n] = _G(tX[i], tY[i])
    d = out - full
    want = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum() / (2 * N * N) / 2
    got = dc.loss_fun_sl1(out, tX, tY)
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    (gg,) = torch.autograd.grad(got, out)
    assert gg[0, n:].abs().max().item() > 0 and gg[1, :, n:].abs().max().item() > 0          # the padding has a gradient
    assert torch.allclose(gg, d.detach().clamp(-1, 1) / (2 * N * N) / 2, rtol=1e-12, atol=0)


def test_inverse_permutation_check():
    g = torch.Generator().manual_seed(3)
    label = torch.randperm(56, generator=g)
    inv = torch.argsort(label)
    assert dc.labels_are_inverse(label, inv) and dc.labels_are_inverse(inv, label)
    bad = inv.clone()
    bad[[0, 1]] = bad[[1, 0]]
    assert not dc.labels_are_inverse(label, bad)                         # a permutation, not the inverse
    dup = label.clone()
    dup[0] = dup[1]
    assert not dc.labels_are_inverse(dup, inv)                           # not a permutation
    assert not dc.labels_are_inverse(label, inv[:-1])
    assert not dc.labels_are_inverse(label + 1, inv)                     # out of range
    assert not dc.labels_are_inverse(label.to(torch.int32), inv)


def test_label_order_matrices_reproduce_the_gathered_sum():
    """(HA + HB)[lA][:, lB] == GA[:, liA[lB]] + GB[liB[lA], :] for mutually inverse labels — the identity the fused kernels use."""
    g = torch.Generator().manual_seed(4)
    tx, ty = _frame(17, g), _frame(17, g)
    HA, HB = dc.label_order_matrix(tx[0], tx[2]), dc.label_order_matrix(ty[0], ty[2])
    assert torch.equal((HA + HB)[tx[1]][:, ty[1]], _G(tx, ty))


def test_golden_faust_frame_labels_are_inverse_permutations():
    import os

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "data_faust_frame.npz"), allow_pickle=True)
    assert dc.labels_are_inverse(torch.from_numpy(z["label"].astype(np.int64)), torch.from_numpy(z["label_inv"].astype(np.int64)))


def test_pair_batch_rejects_an_unknown_loss():
    import pytest

    with pytest.raises(ValueError, match="loss"):
        dc.PairBatch(None, 0, 1, loss="l2")
