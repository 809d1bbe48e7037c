"""The 128 -> 3 head of the normal-prediction models runs as a 4-output layer (normal_predict, blocks.elu_conv with pad_to): the
Linear kernels at K = 128, J = 4 — forward, the plain input gradient, the input gradient through the ELU as _EluConv's backward
uses it, and the weight gradient — against float64, with tests/linear_truth.py's operands and bound (operands inside NaN arenas,
outputs inside canary arenas).  Rows: one, either side of a 32-row tile, a ragged multiple, and more than one workgroup's share."""
import numpy as np
import pytest
import torch

import linear_truth as lt
from helpers import _arena, _outside_untouched
from surfacenetworks_amd import _lib, kernels
from surfacenetworks_amd.kernels import _ld, _p, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 7.0
K, J = 128, 4
ROWS = (1, 31, 33, 97, 16481)


def _in(t):
    return _arena(t.shape[0], t.shape[1], values=t, device=DEV)[1]


def _vec(t):
    a = torch.full((t.numel() + 16,), float("nan"), device=DEV)
    v = a[8:8 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _out(rows, width):
    return _arena(rows, width, fill=CANARY, values=torch.tensor(CANARY), device=DEV)


def _held(name, arena, got, ref, tol, scale, pad_cols=8):
    r = lt.worst_ratio(got, ref, tol, scale)
    assert r <= 1.0, (name, r)
    assert _outside_untouched(arena, got.shape[0], got.shape[1], CANARY, pad_cols=pad_cols), f"{name}: wrote outside its view"


def test_the_shape_is_one_the_kernels_take():
    assert kernels.linear_fwd_supported(K, J) and kernels.linear_dgrad_supported(J, K) and kernels.wgrad_supported(J, K)
    assert kernels.linear_dgrad_elu_supported(128, K)
    assert not kernels.linear_fwd_supported(K, 3) and not kernels.wgrad_supported(3, K)      # why the head is padded


@pytest.mark.parametrize("flavour", ["plain", "magnitudes"])
@pytest.mark.parametrize("rows", ROWS)
def test_forward(rows, flavour):
    o = lt.fwd_operands(rows, K, J, flavour, DEV)
    o["W"][3] = 0.0                              # the pad row, as the models run the layer ...
    o["bias"][3] = 0.0
    x, W, bias = _in(o["x"]), _in(o["W"]), _vec(o["bias"])
    ya, y = _out(rows, J)
    _lib.call("sn_linear_fwd_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), None, 0, _p(y), _ld(y), None, 0, rows, K, J, None,
              None, _stream())
    ref, scale = lt.ref_fwd(x, W, bias=bias)
    _held("y", ya, y, ref, lt.tol_of(scale, K), scale)
    assert not bool(y[:, 3].any())               # ... whose column is exactly zero
    # every row of W live, too: nothing in the kernel may depend on the pad
    o = lt.fwd_operands(rows, K, J, flavour, DEV)
    x, W, bias = _in(o["x"]), _in(o["W"]), _vec(o["bias"])
    ya, y = _out(rows, J)
    _lib.call("sn_linear_fwd_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), None, 0, _p(y), _ld(y), None, 0, rows, K, J, None,
              None, _stream())
    ref, scale = lt.ref_fwd(x, W, bias=bias)
    _held("y (four live rows)", ya, y, ref, lt.tol_of(scale, K), scale)


@pytest.mark.parametrize("flavour", ["plain", "magnitudes"])
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("rows", ROWS)
def test_plain_input_gradient(rows, tail, flavour):
    o = lt.dgrad_operands(rows, K, J, flavour, DEV)
    o["dy"][:, 3] = 0.0                          # the loss kernel writes 0 into the fourth gradient column
    dy, W = _in(o["dy"]), _in(o["W"])
    x, cen, B, Cc = (_in(o["x"]), _vec(o["center"]), _vec(o["B"]), _vec(o["Cc"])) if tail else (None, None, None, None)
    da, dx = _out(rows, K)
    _lib.call("sn_linear_dgrad_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x) if tail else 0, _p(cen), _p(B), _p(Cc), _p(dx),
              _ld(dx), rows, J, K, _stream())
    ref, scale = lt.ref_dgrad(dy, W, x, cen, B, Cc)
    _held("dx", da, dx, ref, lt.tol_of(scale, J), scale)


@pytest.mark.parametrize("flavour", ["plain", "magnitudes"])
@pytest.mark.parametrize("rows", ROWS)
def test_input_gradient_through_the_elu(rows, flavour):
    """kernels.linear_dgrad_eluseg(dy, Wf, x, mean, Bc, Cc, None, 0): functional.bnlin_backward_elu_input's launch."""
    o = lt.dgrad_operands(rows, K, J, flavour, DEV)
    o["dy"][:, 3] = 0.0
    dy, W, x, cen, B, Cc = _in(o["dy"]), _in(o["W"]), _in(o["x"]), _vec(o["center"]), _vec(o["B"]), _vec(o["Cc"])
    ga, gact = _out(rows, K)
    am = torch.full((int(_lib.load().sn_linear_dgrad_absmax_blocks()),), float("nan"), device=DEV)
    _lib.call("sn_linear_dgrad_eluseg_absmax_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), None, 0,
              None, _p(gact), _ld(gact), None, 0, rows, J, K, _p(am), _stream())
    ref, scale = lt.ref_dgrad_act(dy, W, x, cen, B, Cc)
    _held("gact", ga, gact, ref, lt.tol_of(scale, J), scale)
    assert bool(torch.isfinite(am).all()) and float(am.max()) == float(gact.abs().max())


@pytest.mark.parametrize("rows", ROWS)
def test_weight_gradient(rows):
    """G = dy^T (x - center) and colsum(dy) (sn_wgrad_f32: the three-piece form, what a dy without recorded maxima takes)."""
    o = lt.dgrad_operands(rows, K, J, "plain", DEV)
    o["dy"][:, 3] = 0.0
    dy, x, cen = _in(o["dy"]), _in(o["x"]), _vec(o["center"])
    Ga, G = _arena(J, K, pad_cols=0, fill=CANARY, values=torch.tensor(CANARY), device=DEV)      # (G has no leading dimension in the ABI)
    dysum = torch.full((J,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(max(int(_lib.load().sn_wgrad_workspace_bytes(rows, J, K)), 16), dtype=torch.uint8, device=DEV)
    _lib.call("sn_wgrad_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(cen), rows, J, K, _p(G), _p(dysum), _p(ws),
              int(_lib.load().sn_wgrad_workspace_bytes(rows, J, K)), _stream())
    xc = x.double() - cen.double()
    ref, scale = dy.double().t() @ xc, dy.double().abs().t() @ xc.abs()
    _held("G", Ga, G, ref, lt.tol_of(scale, rows), scale, pad_cols=0)
    assert not bool(G[3].any())                  # the pad's gradient row: exactly zero (dropped by the pad's backward anyway)
    s_ref, s_scale = dy.double().sum(0), dy.double().abs().sum(0)
    assert bool(((dysum - s_ref).abs() <= lt.tol_of(s_scale, rows)).all())
