"""Every compiled form of the Linear GEMM kernels (csrc/sn_gemm.hip) against float64, on both sides of the launchers' operand-size
threshold: the SMALL instantiations of gemm_rows_split_k (one-pass weight prologue), the large ones (two-pass prologue) and the
eight-wave forward kernel gemm_fwd_w8_k.  The threshold comes from the library (kernels.linear_small_rows()), the form a forward
launch takes from kernels.linear_fwd_form(); references, operands and the per-element bound are tests/linear_truth.py — the
bound is derived there, and tests/test_linear_truth.py shows on a model of the split that it separates a right kernel from one
that loses a correction product.

Row counts, with R = kernels.linear_small_rows(): 33 (two tiles, the second of one row, almost every workgroup without a tile),
R (SMALL form, several tiles per workgroup, a full last tile) and R + 1 (large form, a last tile of one row).  Every operand is
a strided view inside an arena of NaN, every output a view inside an arena of canaries (helpers._arena) that must stay untouched
outside the view — so the entry points are called through the C ABI the kernels.* wrappers call (the wrappers allocate dense
outputs of their own).  The uniform per-mesh forms use the factorisation of the row count with the fewest meshes (more than one
where possible) of at least 32 rows; the ragged forms a PackedSegments whose lengths are >= 32 and not all multiples of 32."""
import gc

import numpy as np
import pytest
import torch

import linear_truth as lt
from helpers import _arena, _outside_untouched

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 7.0

from surfacenetworks_amd import _lib, kernels  # noqa: E402
from surfacenetworks_amd.kernels import _ld, _p, _stream  # noqa: E402

ROW_KINDS = ("33", "R", "R+1")


def _rows(kind):
    R = kernels.linear_small_rows()
    return {"33": 33, "R": R, "R+1": R + 1}[kind]


def _case(entry, width, J=128, **flags):
    return dict(entry=entry, width=width, J=J, **flags)


def _case_id(c):
    flags = "-".join(k if v is True else f"{k}={v}" for k, v in c.items() if k not in ("entry", "width", "J") and v not in (False, None))
    return f"{c['entry']}-{c['width']}-J{c['J']}" + (f"-{flags}" if flags else "")


# the table: entry point, K (forward) or C (input gradient), J, flags.  Together the rows reach every instantiation the
# launchers of sn_gemm.hip compile, on both sides of R.
CASES = (
    # forward, sn_linear_fwd_tiles_f32 (kernels.linear_fwd)
    [_case("fwd", K, res=res, elu=elu) for K in (128, 256) for res in (False, True) for elu in (False, True)]
    + [_case("fwd", 128, J=120, res=True, elu=True), _case("fwd", 256, J=120, elu=True), _case("fwd", 256, J=4)]
    + [_case("fwd", 256, elu=True, copy_only=True),               # gemm_fwd_w8_k above R: its first value test
       _case("fwd", 128, elu=True, copy_only=True),
       _case("fwd", 256, elu=True, copy_only=True, tiles=True)]   # statistics + tile sums: not the eight-wave kernel
    # per-mesh bias, sn_linear_fwd_segbias[_ragged]_tiles_f32 (kernels.linear_fwd_segbias, linear_fwd_segbias_ragged)
    + [_case("fwd_segbias", 128, res=True, elu=True), _case("fwd_segbias", 256, J=120, elu=True),
       _case("fwd_segbias", 128, res=True, elu=True, ragged=True), _case("fwd_segbias", 256, ragged=True)]
    # input gradient, sn_linear_dgrad_f32 (kernels.linear_dgrad)
    + [_case("dgrad", C, tail=tail) for C in (128, 256) for tail in (False, True)]
    + [_case("dgrad", 256, J=120, tail=True), _case("dgrad", 128, J=64)]
    # through the activation, sn_linear_dgrad_elu_absmax_f32 (kernels.linear_dgrad_elu)
    + [_case("dgrad_elu", C, gadd=gadd) for C in (128, 256) for gadd in (False, True)]
    # every column through the activation, sn_linear_dgrad_eluseg[_ragged]_absmax_f32 (kernels.linear_dgrad_eluseg[_ragged])
    + [_case("eluseg", C, gadd=True) for C in (128, 256)]
    + [_case("eluseg", C, segvec=True, mask=True, gadd=True) for C in (128, 256)]
    + [_case("eluseg", C, segvec=True, ragged=True) for C in (128, 256)]
    # raw low half, sn_linear_dgrad_elu_rawlow_f32 (kernels.linear_dgrad_elu_raw)
    + [_case("raw", C) for C in (128, 256)]
)
# one case per entry point (and the eight-wave kernel) once more with rows / columns spread over 2^40 / 2^20, above R: the
# two-pass weight prologue is where the large form differs, and column scales are what it computes
MAGNITUDES = [_case("fwd", 256, res=True, elu=True), _case("fwd", 256, elu=True, copy_only=True),
              _case("fwd_segbias", 128, res=True, elu=True), _case("fwd_segbias", 256, ragged=True),
              _case("dgrad", 256, tail=True), _case("dgrad_elu", 256, gadd=True),
              _case("eluseg", 128, segvec=True, mask=True, gadd=True), _case("eluseg", 256, segvec=True, ragged=True),
              _case("raw", 256)]
PARAMS = [pytest.param(c, kind, "plain", id=f"{_case_id(c)}-rows{kind}") for c in CASES for kind in ROW_KINDS] + \
         [pytest.param(c, "R+1", "magnitudes", id=f"{_case_id(c)}-rowsR+1-magnitudes") for c in MAGNITUDES]


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    gc.collect()
    torch.cuda.empty_cache()


# ---- placement ---------------------------------------------------------------------------------------------------------------
def _in(t):
    """A rows x width operand as a strided view inside an arena of NaN (pad rows and pad columns on every side)."""
    return _arena(t.shape[0], t.shape[1], values=t, device=DEV)[1]


def _vec(t):
    """A dense vector (or a dense table such as segbias, which has no leading dimension in the ABI) between NaNs."""
    a = torch.full((t.numel() + 16,), float("nan"), device=DEV)
    v = a[8:8 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _out(rows, width):
    """(arena, view) of canaries for an output."""
    return _arena(rows, width, fill=CANARY, values=torch.tensor(CANARY), device=DEV)


def _check(report, name, arena, got, ref, tol, scale):
    r = lt.worst_ratio(got, ref, tol, scale)
    report.append(f"{name} {r:.3f}")
    assert _outside_untouched(arena, got.shape[0], got.shape[1], CANARY), f"{name}: wrote outside its view"
    return r


def _absmax_buffer():
    return torch.full((int(_lib.load().sn_linear_dgrad_absmax_blocks()),), float("nan"), device=DEV)


def _check_absmax(am, gact):
    """Every slot written, finite and >= 0; their maximum IS the largest |gact| of the kernel's own output."""
    assert bool(torch.isfinite(am).all()) and bool((am >= 0).all())
    assert float(am.max()) == float(gact.abs().max())


def _meshes(c, rows):
    """(mesh index per row, rows_per_seg | None, PackedSegments | None, nseg)"""
    if c.get("ragged"):
        from surfacenetworks_amd.operators import PackedSegments

        lengths = lt.ragged_lengths(rows)
        assert min(lengths) >= 32 and sum(lengths) == rows and (rows == 33 or any(n % 32 for n in lengths))
        seg = PackedSegments(lengths, DEV)
        return lt.mesh_of_rows(rows, DEV, lengths=lengths), None, seg, seg.nseg
    nseg, per = lt.uniform_meshes(rows)
    assert nseg * per == rows and per >= 32
    return lt.mesh_of_rows(rows, DEV, rows_per_seg=per), per, None, nseg


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def _run_fwd(c, rows, kind, flavour, report):
    K, J = c["width"], c["J"]
    res, elu, copy_only, tiles = c.get("res", False), c.get("elu", False), c.get("copy_only", False), c.get("tiles", False)
    segb = c["entry"] == "fwd_segbias"
    o = lt.fwd_operands(rows, K, J, flavour, DEV)
    x, W = _in(o["x"]), _in(o["W"])
    r = _in(o["residual"]) if res else None
    ya, y = (None, None) if copy_only else _out(rows, J)
    ea, e = _out(rows, J) if elu else (None, None)
    part = tsum = None
    if tiles:
        part = kernels.new_elu_stats_part(rows, DEV).fill_(float("nan"))      # every entry the merge reads must be written
        tsum = kernels.new_tile_sums(rows, DEV).fill_(float("nan"))           # ... and every tile
    args_tail = (_p(r), _ld(r) if res else 0, _p(y), _ld(y) if y is not None else 0, _p(e), _ld(e) if elu else 0, rows, K, J,
                 _p(part), _p(tsum), _stream())
    if not segb:
        form = kernels.linear_fwd_form(rows, K, J, residual=res, want_y=not copy_only, y_elu=elu, tile_sums=tiles)
        if not kernels._split_gemm():
            want_form = 0
        elif kind != "R+1":
            want_form = 1
        else:
            want_form = 3 if (copy_only and K == 256 and J == 128 and not res and not tiles) else 2
        assert form == want_form, (form, want_form)
        report.append(f"form {form}")
        bias = _vec(o["bias"])
        _lib.call("sn_linear_fwd_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), *args_tail)
        ref, scale = lt.ref_fwd(x, W, bias=bias, residual=r)
    else:
        mesh, per, seg, nseg = _meshes(c, rows)
        sb = _vec(lt.seg_vectors(nseg, J, DEV, rows, K))
        if seg is not None:
            _lib.call("sn_linear_fwd_segbias_ragged_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(sb), _p(seg.off_dev), nseg, *args_tail)
        else:
            _lib.call("sn_linear_fwd_segbias_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(sb), per, *args_tail)
        ref, scale = lt.ref_fwd(x, W, residual=r, segbias=sb, mesh=mesh)
    worst = 0.0
    if y is not None:
        worst = max(worst, _check(report, "y", ya, y, ref, lt.tol_of(scale, K), scale))
    if elu:
        worst = max(worst, _check(report, "y_elu", ea, e, lt.elu64(ref), lt.tol_elu_of(scale, K), scale))
    if tiles:
        # tile sums: the float64 sums of the kernel's OWN activated output over each 32-row tile, within 32 fp32 roundings of
        # the tile's sum of |e|; merged statistics: one fp64 pass over the buffer
        nt = (rows + 31) // 32
        e64 = torch.zeros(nt * 32, J, dtype=torch.float64, device=DEV)
        e64[:rows] = e.double()
        e64 = e64.view(nt, 32, J)
        assert bool(((tsum.double() - e64.sum(1)).abs() <= 32 * lt.EPS * e64.abs().sum(1)).all()), "tile sums"
        st, want = kernels.colstats_from_part(part, rows).cpu().numpy(), kernels.colstats(e).cpu().numpy()
        assert np.isfinite(st).all() and np.allclose(st, want, rtol=1e-12, atol=1e-9), "merged statistics"
    return worst


def _run_dgrad(c, rows, kind, flavour, report):
    C, J, tail = c["width"], c["J"], c.get("tail", False)
    o = lt.dgrad_operands(rows, C, J, flavour, DEV)
    dy, W = _in(o["dy"]), _in(o["W"])
    x, cen, B, Cc = (_in(o["x"]), _vec(o["center"]), _vec(o["B"]), _vec(o["Cc"])) if tail else (None, None, None, None)
    da, dx = _out(rows, C)
    _lib.call("sn_linear_dgrad_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x) if tail else 0, _p(cen), _p(B), _p(Cc), _p(dx),
              _ld(dx), rows, J, C, _stream())
    ref, scale = lt.ref_dgrad(dy, W, x, cen, B, Cc)
    return _check(report, "dx", da, dx, ref, lt.tol_of(scale, J), scale)


def _run_dgrad_elu(c, rows, kind, flavour, report):
    C, J, h = c["width"], c["J"], c["width"] // 2
    o = lt.dgrad_operands(rows, C, J, flavour, DEV)
    dy, W, x, cen, B, Cc = _in(o["dy"]), _in(o["W"]), _in(o["x"]), _vec(o["center"]), _vec(o["B"]), _vec(o["Cc"])
    gadd = _in(o["gadd"][:, :h]) if c.get("gadd") else None
    ha, dx_hi = _out(rows, h)
    ga, gact = _out(rows, h)
    am = _absmax_buffer()
    _lib.call("sn_linear_dgrad_elu_absmax_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), _p(dx_hi),
              _ld(dx_hi), _p(gact), _ld(gact), _p(gadd), _ld(gadd) if gadd is not None else 0, rows, J, C, _p(am), _stream())
    ref, scale = lt.ref_dgrad(dy, W[:, h:], x[:, h:], cen[h:], B[h:], Cc[h:])
    worst = _check(report, "dx_hi", ha, dx_hi, ref, lt.tol_of(scale, J), scale)
    ref, scale = lt.ref_dgrad_act(dy, W[:, :h], x[:, :h], cen[:h], B[:h], Cc[:h], gadd=gadd)
    worst = max(worst, _check(report, "gact", ga, gact, ref, lt.tol_of(scale, J), scale))
    _check_absmax(am, gact)
    return worst


def _run_eluseg(c, rows, kind, flavour, report):
    C, J = c["width"], c["J"]
    o = lt.dgrad_operands(rows, C, J, flavour, DEV)
    dy, W, x, cen, B, Cc = _in(o["dy"]), _in(o["W"]), _in(o["x"]), _vec(o["center"]), _vec(o["B"]), _vec(o["Cc"])
    gadd = _in(o["gadd"]) if c.get("gadd") else None
    ga, gact = _out(rows, C)
    am = _absmax_buffer()
    sv = mesh = mask = None
    head = (_p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc))
    tail = (_p(gact), _ld(gact), _p(gadd), _ld(gadd) if gadd is not None else 0, rows, J, C, _p(am), _stream())
    if c.get("segvec"):
        mesh, per, seg, nseg = _meshes(c, rows)
        sv = _vec(lt.seg_vectors(nseg, C, DEV, rows, J))
        if seg is not None:
            _lib.call("sn_linear_dgrad_eluseg_ragged_absmax_f32", *head, _p(sv), _p(seg.off_dev), nseg, *tail)
        else:
            mask = _vec(lt.row_mask(rows, DEV)) if c.get("mask") else None
            _lib.call("sn_linear_dgrad_eluseg_absmax_f32", *head, _p(sv), per, _p(mask), *tail)
    else:
        _lib.call("sn_linear_dgrad_eluseg_absmax_f32", *head, None, 0, None, *tail)
    ref, scale = lt.ref_dgrad_act(dy, W, x, cen, B, Cc, segvec=sv, mesh=mesh, rowmask=mask, gadd=gadd)
    worst = _check(report, "gact", ga, gact, ref, lt.tol_of(scale, J), scale)
    _check_absmax(am, gact)
    return worst


def _run_raw(c, rows, kind, flavour, report):
    C, J, h = c["width"], c["J"], c["width"] // 2
    o = lt.dgrad_operands(rows, C, J, flavour, DEV)
    o["x"][:, :h] = float("nan")                                  # the low half of x must not reach any output
    dy, W, x, cen, B, Cc = _in(o["dy"]), _in(o["W"]), _in(o["x"]), _vec(o["center"]), _vec(o["B"]), _vec(o["Cc"])
    ha, dx_hi = _out(rows, h)
    ra, graw = _out(rows, h)
    _lib.call("sn_linear_dgrad_elu_rawlow_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), _p(dx_hi),
              _ld(dx_hi), _p(graw), _ld(graw), rows, J, C, _stream())
    ref, scale = lt.ref_dgrad(dy, W[:, h:], x[:, h:], cen[h:], B[h:], Cc[h:])          # dx_hi carries the full tail
    worst = _check(report, "dx_hi", ha, dx_hi, ref, lt.tol_of(scale, J), scale)
    ref, scale = lt.ref_dgrad(dy, W[:, :h])                                            # graw = dy·W[:, :C/2], bare
    return max(worst, _check(report, "graw", ra, graw, ref, lt.tol_of(scale, J), scale))


RUNNERS = {"fwd": _run_fwd, "fwd_segbias": _run_fwd, "dgrad": _run_dgrad, "dgrad_elu": _run_dgrad_elu, "eluseg": _run_eluseg,
           "raw": _run_raw}


def _baseline_offers(c):
    """What the fp32-MFMA A/B baseline (SN_GEMM_VARIANT=0) runs: the plain forward and input gradient at J = 128, y written."""
    return c["entry"] in ("fwd", "dgrad") and c["J"] == 128 and not c.get("copy_only") and not c.get("tiles")


@pytest.mark.parametrize("case,kind,flavour", PARAMS)
def test_linear_kernel_forms_against_float64(case, kind, flavour, request):
    """Each output within linear_truth's bound of its float64 reference, element by element; finite wherever the bound is;
    nothing written outside the output views; the forward's form is the one the row count asks for."""
    if not kernels._split_gemm() and not _baseline_offers(case):
        pytest.skip("16-bit matrix-pipe kernels only (SN_GEMM_VARIANT=0 is the A/B baseline)")
    rows = _rows(kind)
    report = []
    try:
        worst = RUNNERS[case["entry"]](case, rows, kind, flavour, report)
    finally:
        print(f"\nlinear-forms {request.node.callspec.id}: rows {rows}  err/tol  " + "  ".join(report))
    assert worst <= 1.0, report
