"""The squared-cosine loss kernels (sn_normal_cosine_*, csrc/sn_dense.hip) against the float64 statement of their definition
(include/sn_spmm.h, "Normal prediction"; tests/normal_cases.cos_truth) evaluated on the kernels' own fp32 operands.

THE BOUNDS, from the kernels' expression (roundings counted from csrc/sn_dense.hip, cos_row / cos_store_grad; d = 2^-24, every
magnitude `scale` the formula with each term replaced by its absolute value, as tests/linear_truth.py does):
  o = y + frame        1 rounding per component (none without a frame)
  n = sqrt(o·o)        3 roundings of the sum of squares (all terms >= 0) + 2 from o, halved by the root, + 1:  3.5 d (2.5 d)
  u = o / n            1 (o) + 3.5 (n) + 1 (division) = 5.5 d   (3.5 d)
  c = u·t              3 roundings, each of a partial sum bounded by C = sum |u_k t_k|, + 5.5 d C from u:  8.5 d C -> COUNT_C = 9 (7)
  l = 1 - c^2          2 C err_c + 1 rounding of the result:  (2 COUNT_C + 1) d (1 + C^2) -> COUNT_L = 19 (15)
  g = k (-2c) (t - c u) / n,  k = gloss (1/|S|):  2 (k) + COUNT_C (c in the coefficient) + 1 (product) + 3.5 + 1 (n, division)
      + 1 + COUNT_C + 5.5 (the bracket: its rounding, c, u) + 1 (last product), + 1 for second-order terms:  COUNT_G = 34 (27),
      times g_scale = (|gloss|/|S|) 2 C (|t| + C |u|) / n.  Below the 1e-12 clamp the expression is shorter (the bracket is t, n is
      the constant, whose fp32 value is within d of 1e-12): the same counts hold.
  loss = (sum l) / |S| in fp64, rounded to fp32 once: the mean of the row bounds + d |loss|.
  mad: acos is decreasing in |c|: every row's angle lies in [acos(min(|c| + err_c, 1)), acos(max(|c| - err_c, 0))] up to the
      error of acosf itself, allowed for as 2 A per row, A the largest deviation of THIS device's torch.acos in fp32 from float64
      acos over 4096 points of [0, 1] (the ruler is torch's implementation, not the code under test; the factor 2 admits another
      equally legitimate acosf); the mean's interval is widened by the one fp32 rounding of the result.
Nothing is fitted to what the kernels return."""
import numpy as np
import pytest
import torch

import normal_cases as nc
from helpers import _arena, _outside_untouched

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = nc.EPS32
COUNT_C = {False: 7, True: 9}
COUNT_L = {False: 15, True: 19}
COUNT_G = {False: 27, True: 34}
CANARY = 777.0
PREFILL = 5.0


def _same(a, b):
    """Bit for bit (torch.equal calls two NaN different; an empty mask gives NaN by definition)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _grid_rows():
    from surfacenetworks_amd import kernels

    return kernels.normal_cosine_grid_rows()


@pytest.fixture(scope="module")
def acos_ruler():
    x = torch.linspace(0.0, 1.0, 4096, dtype=torch.float64, device=DEV)
    return float((torch.acos(x.float()).double() - torch.acos(x.float().double())).abs().max())


def _masks(rows):
    ragged = torch.ones(rows, device=DEV)
    ragged[torch.arange(rows, device=DEV) % 7 == 6] = 0
    if rows >= 8:
        ragged[(3 * rows) // 4:] = 0
    return {"none": None, "ones": torch.ones(rows, device=DEV), "ragged": ragged, "zero": torch.zeros(rows, device=DEV)}


def _operands(rows, pitch, frame_kind, mask, seed):
    """y as a (rows, 3) view of a (rows, pitch) buffer (the fourth column of a pitch-4 buffer is NaN: never an operand), t, the
    frame (None / stride 3 / a stride-7 view that starts 12 bytes past a 16-byte boundary); NaN in every row outside the mask."""
    y, t, fr = nc.planted_rows(rows, seed, DEV, frame=frame_kind != "none")
    buf = torch.full((rows, pitch), float("nan"), device=DEV)
    buf[:, :3] = y
    frame = None
    if frame_kind == "stride3":
        frame = fr.contiguous()
    elif frame_kind == "stride7":
        base = torch.full((rows * 7 + 8,), float("nan"), device=DEV)
        frame = base[3:3 + rows * 7].view(rows, 7)[:, :3]
        assert frame.data_ptr() % 16 == 12
        frame.copy_(fr)
    if mask is not None:
        out_rows = mask == 0
        buf[out_rows] = float("nan")
        t[out_rows] = float("nan")
        if frame is not None:
            frame[out_rows] = float("nan")
    return buf, buf[:, :3], t, frame


def _check(rows, pitch, frame_kind, mask_kind, mask, acos_a, seed):
    from surfacenetworks_amd import _lib, kernels

    what = (rows, pitch, frame_kind, mask_kind)
    buf, y3, t, frame = _operands(rows, pitch, frame_kind, mask, seed)
    has_frame = frame is not None
    tr = nc.cos_truth(y3, t, mask, frame)
    # the operand: the (rows, 3) view of the buffer; a single row has no pitch of its own, so there the contiguous (1, 4) buffer
    # itself stands for pitch 4 (the padded head's form: one 16-byte load, one 16-byte store, fourth gradient column 0)
    y = buf if (pitch == 4 and rows == 1) else y3
    count = tr["count"]
    # ---- the launchers: forward-only, forward with gradient (twice: the same bits), the finished gradient for gloss 1 and 0.5
    out_f = kernels.normal_cosine_fwd(y, t, mask, frame)
    out, g = kernels.normal_cosine_fwdg(y, t, mask, frame)
    out2, g2 = kernels.normal_cosine_fwdg(y, t, mask, frame)
    assert _same(out, out2) and _same(g, g2), what
    assert _same(out_f, out), what                                                        # forward-only entry: the same loss bits
    eff_pitch = pitch
    assert g.shape == (rows, eff_pitch) and float(out[2]) == count, what
    one = torch.ones(1, device=DEV)
    assert torch.equal(kernels.normal_cosine_bwd(y, t, mask, frame, out, one), g), what                  # recomputed == written by the pass
    assert torch.equal(kernels.normal_cosine_bwd(y, t, mask, frame, out, one, g=g.clone()), g), what     # kept
    half = torch.full((1,), 0.5, device=DEV)
    g_half = kernels.normal_cosine_bwd(y, t, mask, frame, out, half, g=g.clone())
    assert torch.equal(g_half, kernels.normal_cosine_bwd(y, t, mask, frame, out, half)), what
    if pitch == 4:
        # the contiguous (rows, 4) buffer itself as the operand (the padded head's output): the same bits
        out4, g4 = kernels.normal_cosine_fwdg(buf, t, mask, frame)
        assert _same(out4, out) and _same(g4, g), what
        assert torch.equal(g[:, 3], torch.zeros(rows, device=DEV)) and torch.equal(g_half[:, 3], torch.zeros(rows, device=DEV)), what
    # ---- rows outside the mask: exactly zero; an empty mask: NaN, NaN, all zero
    if mask is not None:
        assert not bool(g[mask == 0].any()) and not bool(g_half[mask == 0].any()), what
    if count == 0:
        assert bool(torch.isnan(out[:2]).all()) and not bool(g.any()), what
        return
    # ---- loss
    C = tr["c_scale"]
    S = tr["S"]
    l_tol = float((COUNT_L[has_frame] * D * (1 + C * C))[S].sum()) / count + D * abs(tr["loss"])
    assert abs(float(out[0]) - tr["loss"]) <= l_tol, (what, float(out[0]), tr["loss"], l_tol)
    # ---- metric
    err_c = COUNT_C[has_frame] * D * C
    lo = torch.acos((tr["c"].abs() + err_c).clamp(max=1.0))[S].sum()
    hi = torch.acos((tr["c"].abs() - err_c).clamp(min=0.0, max=1.0))[S].sum()
    lo, hi = float(lo - 2 * acos_a * count) / count, float(hi + 2 * acos_a * count) / count
    assert lo * (1 - D) <= float(out[1]) <= hi * (1 + D), (what, lo, float(out[1]), hi)
    # ---- gradient, every element, for gloss 1 and 0.5
    for got, gl in ((g, 1.0), (g_half, 0.5)):
        trg = tr if gl == 1.0 else nc.cos_truth(y3, t, mask, frame, gloss=gl)
        tol = COUNT_G[has_frame] * D * trg["g_scale"]
        err = (got[:, :3].double() - trg["g"]).abs()
        assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), (what, gl, float((err / tol.clamp_min(1e-300)).max()))
    # ---- canaries: the C entry points write g rows [0, rows) x pitch and three floats of `out`, nothing else
    # (the views are pre-filled with a value no output takes: an element the entry point skips shows)
    arena_g, view_g = _arena(rows, eff_pitch, pad_cols=0, fill=CANARY, values=torch.full((rows, eff_pitch), PREFILL))
    arena_o, view_o = _arena(1, 3, pad_rows=1, pad_cols=0, fill=CANARY, values=torch.full((1, 3), PREFILL))
    ws = torch.empty(int(_lib.load().sn_normal_cosine_workspace_bytes(rows)), dtype=torch.uint8, device=DEV)
    p = lambda x: None if x is None else x.data_ptr()
    ldy = pitch
    ldf = (frame.stride(0) if rows > 1 else 3) if has_frame else 0
    _lib.call("sn_normal_cosine_fwdg_f32", p(y), ldy, p(frame), ldf, p(t), 3, p(mask), rows, p(view_o), p(view_g), eff_pitch, p(ws),
              ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert torch.equal(view_g, g) and torch.equal(view_o.reshape(3), out), what
    assert _outside_untouched(arena_g, rows, eff_pitch, CANARY, pad_cols=0) and _outside_untouched(arena_o, 1, 3, CANARY, 1, 0), what
    _lib.call("sn_normal_cosine_bwdg_f32", p(y), ldy, p(frame), ldf, p(t), 3, p(mask), rows, p(view_o.reshape(3)[2:]), p(half),
              p(view_g), eff_pitch, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(view_g, g_half) and _outside_untouched(arena_g, rows, eff_pitch, CANARY, pad_cols=0), what
    if pitch == 4:
        # a pitch-4 g that starts 4 bytes past a 16-byte boundary takes 4-byte stores: the fourth column is written 0 all the same
        base = torch.full((rows * 4 + 8,), CANARY, device=DEV)
        off_g = base[1:1 + rows * 4].view(rows, 4)
        assert off_g.data_ptr() % 16 == 4
        for name, tail, want in (("sn_normal_cosine_fwdg_f32", (p(ws), ws.numel()), g), ("sn_normal_cosine_bwd_f32", (), g_half)):
            off_g.fill_(PREFILL)
            if tail:
                _lib.call(name, p(y), ldy, p(frame), ldf, p(t), 3, p(mask), rows, p(view_o), p(off_g), 4, *tail,
                          torch.cuda.current_stream().cuda_stream)
            else:
                _lib.call(name, p(y), ldy, p(frame), ldf, p(t), 3, p(mask), rows, p(view_o.reshape(3)[2:]), p(half), p(off_g), 4,
                          torch.cuda.current_stream().cuda_stream)
            assert torch.equal(off_g, want), (what, name)
            assert bool((base[:1] == CANARY).all()) and bool((base[1 + rows * 4:] == CANARY).all()), (what, name)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, "grid+65"])
def test_loss_metric_and_gradient_against_float64(rows, acos_ruler):
    """Rows either side of a wavefront, a ragged tail, and more rows than the grid has threads (every thread walks on); pitch
    3 / 4; frame none / stride 3 / stride 7 off the 16-byte grid; mask none / ones / ragged with NaN planted in every masked row
    of y, frame and t / all zero; a zero row, a row below the 1e-12 norm, parallel and anti-parallel rows, rows scaled by 2^+-20."""
    rows = _grid_rows() + 65 if rows == "grid+65" else rows
    seed = 0
    for pitch in (3, 4):
        for frame_kind in ("none", "stride3", "stride7"):
            for mask_kind, mask in _masks(rows).items():
                seed += 1
                _check(rows, pitch, frame_kind, mask_kind, mask, acos_ruler, seed)


def test_autograd_node_no_grad_and_a_scaled_loss(monkeypatch):
    """normal_predict.cosine_loss / loss_and_mad / mean_angle_deviation on device tensors: one launch for both numbers, the
    forward-only entry under no_grad with the same loss bits, and (0.5 * loss).backward() within the gradient bound."""
    from surfacenetworks_amd import kernels
    from surfacenetworks_amd import normal_predict as NP

    B, V = 2, 131
    y, t, _ = nc.planted_rows(B * V, 5, DEV)
    mask = torch.ones(B, V, 1, device=DEV)
    mask[0, 100:] = 0
    mask[1, 77:] = 0
    y[(mask.reshape(-1) == 0)] = float("nan")
    outputs = y.reshape(B, V, 3).clone().requires_grad_(True)
    targets = t.reshape(B, V, 3)
    calls = {"fwd": 0, "fwdg": 0}
    real_fwd, real_fwdg = kernels.normal_cosine_fwd, kernels.normal_cosine_fwdg
    monkeypatch.setattr(kernels, "normal_cosine_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), real_fwd(*a, **k))[1])
    monkeypatch.setattr(kernels, "normal_cosine_fwdg", lambda *a, **k: (calls.__setitem__("fwdg", calls["fwdg"] + 1), real_fwdg(*a, **k))[1])
    loss, mad = NP.loss_and_mad(outputs, mask, targets)
    assert calls == {"fwd": 0, "fwdg": 1} and loss.requires_grad and not mad.requires_grad
    with torch.no_grad():
        loss_ng, mad_ng = NP.loss_and_mad(outputs, mask, targets)
    assert calls == {"fwd": 1, "fwdg": 1} and torch.equal(loss_ng, loss.detach()) and torch.equal(mad_ng, mad)
    assert torch.equal(NP.mean_angle_deviation(outputs, mask, targets), mad) and calls["fwd"] == 2
    assert torch.equal(NP.cosine_loss(outputs, mask, targets).detach(), loss.detach())
    (0.5 * loss).backward()
    tr = nc.cos_truth(y, t, mask.reshape(-1), None, gloss=0.5)
    err = (outputs.grad.reshape(-1, 3).double() - tr["g"]).abs()
    assert bool((err <= COUNT_G[False] * D * tr["g_scale"]).all())
    assert not bool(outputs.grad.reshape(-1, 3)[mask.reshape(-1) == 0].any())          # NaN rows outside the mask: exactly zero
    # against the plain-torch statement on the device, on operands without NaN (autograd turns 0 * NaN into NaN)
    clean = torch.where(mask.expand(B, V, 3) != 0, outputs.detach(), torch.ones_like(outputs)).requires_grad_(True)
    l_ref = NP.loss_reference(clean, mask, targets)
    assert abs(float(l_ref.detach()) - float(loss.detach())) <= 1e-5 * max(abs(float(l_ref.detach())), 1e-6)
    assert abs(float(NP.mad_reference(clean, mask, targets).detach()) - float(mad)) <= 1e-5
    with pytest.raises(RuntimeError, match="no CPU"):
        NP.loss_and_mad(outputs, mask, targets.cpu())


@pytest.mark.parametrize("pitch", [3, 4])
def test_two_backwards_of_one_forward(pitch):
    """The gradient the forward pass wrote serves ONE backward.  gloss 0.5 first (it rewrites that buffer in place), then gloss 1
    (whose launch would keep whatever the buffer holds), then gloss 1 again after the caller zeroed the gradient it was handed in
    place: each within the gradient bound of its own gloss."""
    from surfacenetworks_amd import normal_predict as NP

    B, V = 2, 97
    y, t, _ = nc.planted_rows(B * V, 8, DEV)
    mask = torch.ones(B, V, 1, device=DEV)
    mask[1, 60:] = 0
    buf = torch.zeros(B, V, pitch, device=DEV)
    buf[:, :, :3] = y.reshape(B, V, 3)
    buf.requires_grad_(True)
    loss, _ = NP.loss_and_mad(buf[:, :, :3], mask, t.reshape(B, V, 3))
    first = None
    for step, gl in enumerate((0.5, 1.0, 1.0)):
        buf.grad = None
        (gl * loss).backward(retain_graph=True)
        tr = nc.cos_truth(y, t, mask.reshape(-1), None, gloss=gl)
        got = buf.grad.reshape(-1, pitch)
        err = (got[:, :3].double() - tr["g"]).abs()
        assert bool((err <= COUNT_G[False] * D * tr["g_scale"]).all()), (pitch, step, gl, float((err / tr["g_scale"].clamp_min(1e-300)).max()) / D)
        assert not bool(got[:, 3:].any()) and not bool(got[mask.reshape(-1) == 0].any()), (pitch, step)
        if step == 1:
            first = got.clone()
            buf.grad.zero_()                     # (an in-place edit of what the backward handed out)
        if step == 2:
            assert torch.equal(got, first), pitch
