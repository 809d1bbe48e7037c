"""The bounds behind the two-piece fp16 weight gradient (wgrad16_k<CT, WgradHalf2>, csrc/sn_dense.hip), end to end on the device.

  producers   the per-workgroup maxima the kernels that write dy leave (quaternion-packed Dirac product, the three
              input-gradient GEMM forms) are true, exact, complete, non-negative by bit pattern and stay inside their buffer;
  consumer    the dy scale of sn_wgrad_bounded_f32 is a function of max(dybound) alone: any array with maximum m gives the bits of
              the one-element array [m] (the four paths of the in-kernel reduction, the unaligned pointer, -0.0 and denormals);
  accuracy    flat / seg / slabs forms against float64 at the tile ends, with the tolerances the flat form is already held to
              (tests/test_dense_gpu.py: test_two_piece_weight_gradient_ignores_the_rows_past_the_end,
              test_operands_spanning_more_than_2_28_along_the_contraction), and the header's model (include/sn_spmm.h,
              sn_wgrad_*_bounded_f32) element by element on operands whose premises tests/test_wgrad_bounds.py checks without a GPU;
  audit       every bound a real training step hands to the weight gradient is true for the operands it arrives with.
"""
import inspect

import numpy as np
import pytest
import torch

from helpers import pow2_up_for, split_probe_operands, top_of_binade_operands, wgrad_xbound

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import _lib, kernels  # noqa: E402
from surfacenetworks_amd.kernels import _ld, _p, _stream  # noqa: E402

CANARY = 3e38            # finite and above any |Y| here (a NaN canary would be dropped by fmaxf)


@pytest.fixture(autouse=True)
def _needs_the_bounded_form():
    if not kernels.absmax_wanted():
        pytest.skip("the two-piece weight gradient exists in the 16-bit matrix-pipe kernels only (SN_GEMM_VARIANT=0 is the A/B baseline)")
    yield
    kernels.clear_absmax()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _arena(rows, width, seed, fill=float("nan"), pad_rows=3, pad_cols=8):
    """`view` = rows x width of random values inside an arena filled with `fill` (rows before / after, columns on both sides)."""
    a = torch.full((rows + 2 * pad_rows, width + 2 * pad_cols), fill, device=DEV)
    v = a[pad_rows:pad_rows + rows, pad_cols:pad_cols + width]
    v.copy_(torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32)))
    return a, v


def _outside_untouched(arena, rows, width, canary, pad_rows=3, pad_cols=8):
    m = torch.ones_like(arena, dtype=torch.bool)
    m[pad_rows:pad_rows + rows, pad_cols:pad_cols + width] = False
    return bool((arena[m] == canary).all())


def _maxima_buffer(blocks):
    return torch.full((blocks + 64,), CANARY, device=DEV)


def _check_maxima(am, blocks, Y, what):
    """The contract of a producer's maxima against the output of the same launch (exact: a maximum involves no rounding)."""
    top = float(Y.abs().max())
    assert np.isfinite(top) and top < CANARY
    assert bool((am[blocks:] == CANARY).all()), (what, "wrote past its maxima")
    got = am[:blocks]
    assert bool(torch.isfinite(got).all()), what
    assert int(got.view(torch.int32).min()) >= 0, (what, "an entry below +0.0 by bit pattern")    # the consumer orders bit patterns
    assert float(got.max()) == top, (what, float(got.max()), top)


# ---- 1. producers ---------------------------------------------------------------------------------------------------------------
def _q3_operator(kind, which):
    from helpers import mesh_fixture

    _, _, ops = mesh_fixture(kind)
    A = ops[which[:-1]].T.tocsr() if which.endswith("T") else ops[which]
    A.sort_indices()
    M, K = A.shape
    rp, ci, va = [dev(a) for a in (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32))]
    b = kernels.csr_to_bsr4(rp, ci, va, M, K)
    q, flag = kernels.bsr4_to_q3(b[1], b[2])
    assert int(flag.item()) == 0
    return b[0], q, M // 4, K // 4


def _q3_spike_rows(Mb, N):
    rpb = 256 // (N // 4)                       # block rows per workgroup (sn_spmm_q3_absmax_blocks)
    rows = {0, Mb - 1, min(rpb - 1, Mb - 1), (Mb - 1) // rpb * rpb}
    if Mb > 32:
        rows |= {Mb - 1 - (Mb - 1) % 32, 31, 32}            # first row of the last 32-row block; both sides of a block boundary
    return sorted(rows)


def _q3_check(rp, q, Mb, Kb, N, with_g, seed):
    C = 4 * N
    rng = np.random.default_rng(seed)
    x = dev(rng.standard_normal((Kb, C)).astype(np.float32))
    blocks = int(_lib.load().sn_spmm_q3_absmax_blocks(Mb, N))
    assert blocks >= 1
    e0 = rng.standard_normal((Mb, C)).astype(np.float32)
    g0 = rng.standard_normal((Mb, C)).astype(np.float32)
    spikes = [None] + [(r, c) for r in _q3_spike_rows(Mb, N) for c in (0, C - 1)]
    for spike in spikes:
        e, g = e0.copy(), g0.copy()
        if spike is not None:
            r, c = spike
            if with_g:                          # elu'(-1) = 0: the product part is exactly zero, only the added term carries it
                e[r, c], g[r, c] = -1.0, -1e6
            else:                               # elu'(e) = e + 1: the product times -1e6
                e[r, c] = -1e6 - 1
        ed, gd = dev(e), (dev(g) if with_g else None)
        y0 = torch.full((Mb, C), float("nan"), device=DEV)
        kernels.spmm_q3(rp, q, Mb, Kb, x, y0, 4, ed, gd)
        ya = torch.full((Mb, 2 * C), 7.0, device=DEV)
        y = ya[:, C:]
        am = _maxima_buffer(blocks)
        _lib.call("sn_spmm_q3_elubwd_absmax_f32", _p(rp), _p(q), Mb, Kb, int(q.shape[0]), _p(x), _ld(x), 4, N, _p(ed), _ld(ed), _p(gd),
                  _ld(gd) if with_g else 0, _p(y), _ld(y), 4, _p(am), _stream())
        assert torch.equal(y, y0) and bool((ya[:, :C] == 7.0).all()), spike
        _check_maxima(am, blocks, y, ("q3", N, with_g, spike))
        if spike is not None and with_g:
            assert float(y[spike[0], spike[1]]) == -1e6 and float(am[:blocks].max()) == 1e6


@pytest.mark.parametrize("N", [16, 32, 64, 128])
@pytest.mark.parametrize("kind", ["cloth", "cloth_perm", "torus", "delaunay"])
@pytest.mark.parametrize("which", ["Di", "DiA", "DiT", "DiAT"])
def test_quaternion_product_leaves_true_maxima(N, kind, which):
    """sn_spmm_q3_elubwd_absmax_f32 on the operators of test_quaternion_packed_dirac_product_is_bit_exact: same Y as the plain
    entry point; maxima exact, non-negative by bit pattern, inside their buffer; a spike in the first / last row, at both sides of
    a 32-row block, in the last (partial) workgroup and in the first / last column is seen, carried by the product or by G alone."""
    rp, q, Mb, Kb = _q3_operator(kind, which)
    for with_g in (True, False):
        _q3_check(rp, q, Mb, Kb, N, with_g, seed=N + len(kind))


def test_quaternion_product_maxima_of_a_batch_with_more_than_16384_workgroups():
    """A block-diagonal batch of cloth operators large enough that sn_spmm_q3_absmax_blocks exceeds 16 384 (the consumer's
    unrolled path starts near 14 k maxima): the maxima stay exact and in their buffer, and the bounded weight gradient fed with
    all of them gives the bits of the one fed with their maximum."""
    import scipy.sparse as sp
    from helpers import mesh_fixture

    _, _, ops = mesh_fixture("cloth")
    A1 = ops["Di"].T.tocsr()
    N, C = 32, 128
    rpb = 256 // (N // 4)
    copies = (16500 * rpb) // (A1.shape[0] // 4) + 1
    A = sp.block_diag([A1] * copies, format="csr").astype(np.float32)
    A.sort_indices()
    M, K = A.shape
    rp, ci, va = [dev(a) for a in (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32))]
    b = kernels.csr_to_bsr4(rp, ci, va, M, K)
    q, flag = kernels.bsr4_to_q3(b[1], b[2])
    assert int(flag.item()) == 0
    Mb, Kb = M // 4, K // 4
    blocks = int(_lib.load().sn_spmm_q3_absmax_blocks(Mb, N))
    assert blocks > 16384
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(Kb, C, device=DEV, generator=g)
    e = torch.randn(Mb, C, device=DEV, generator=g)
    gadd = torch.randn(Mb, C, device=DEV, generator=g)
    e[Mb - 1, C - 1], gadd[Mb - 1, C - 1] = -1.0, 1e6            # the last element of the last workgroup carries the maximum
    y0 = torch.empty(Mb, C, device=DEV)
    kernels.spmm_q3(b[0], q, Mb, Kb, x, y0, 4, e, gadd)
    y = torch.empty(Mb, C, device=DEV)
    am = _maxima_buffer(blocks)
    _lib.call("sn_spmm_q3_elubwd_absmax_f32", _p(b[0]), _p(q), Mb, Kb, int(q.shape[0]), _p(x), _ld(x), 4, N, _p(e), _ld(e), _p(gadd),
              _ld(gadd), _p(y), _ld(y), 4, _p(am), _stream())
    assert torch.equal(y, y0)
    _check_maxima(am, blocks, y, "q3 batch")
    assert float(am[:blocks].max()) == 1e6
    xs = torch.randn(Mb, C, device=DEV, generator=g)
    st = kernels.colstats(xs)
    mean = (st[0] / Mb).float()
    invstd = (1.0 / torch.sqrt((st[1] / Mb - (st[0] / Mb) ** 2).clamp_min(0) + 1e-5)).float()
    G = kernels.wgrad(y, xs, mean, bounds=(am[:blocks].contiguous(), invstd, Mb))
    G1 = kernels.wgrad(y, xs, mean, bounds=(am[:blocks].max().reshape(1), invstd, Mb))
    assert bool(torch.isfinite(G).all()) and torch.equal(G, G1)


def _dgrad_operands(rows, J, C, seed):
    rng = np.random.default_rng(seed)
    W = dev((rng.standard_normal((J, C)) / np.sqrt(J)).astype(np.float32))
    cen, B, Cc = [dev(rng.standard_normal(C).astype(np.float32)) for _ in range(3)]
    _, dy = _arena(rows, J, seed + 1)
    _, x = _arena(rows, C, seed + 2)
    return W, cen, B, Cc, dy, x


def _spike_positions(rows, width):
    rs = sorted({0, rows - 1, (rows - 1) // 32 * 32, min(31, rows - 1), min(32, rows - 1)})
    return [None] + [(r, c) for r in rs for c in (0, width - 1)]


DGRAD_ROWS = [1, 31, 32, 33, 95, 1017, 8200, 40001]
DGRAD_JC = [(128, 128), (128, 256), (120, 128), (64, 128), (4, 256)]


@pytest.mark.parametrize("rows", DGRAD_ROWS)
@pytest.mark.parametrize("J,C", DGRAD_JC)
def test_input_gradient_through_half_the_activation_leaves_true_maxima(rows, J, C):
    """sn_linear_dgrad_elu_absmax_f32 (outputs as strided views inside canary arenas): gact bit-identical to the plain launch,
    maxima exact / complete / in their buffer; a spike carried by gadd alone (elu'(-1) = 0 kills the product part) is seen in the
    first and last row, the first row of the last (partial) tile, both sides of a tile boundary, first and last column."""
    h = C // 2
    W, cen, B, Cc, dy, x = _dgrad_operands(rows, J, C, rows + J + C)
    blocks = int(_lib.load().sn_linear_dgrad_absmax_blocks())
    # the largest grid of an input-gradient launch: one workgroup per 32-row tile, at most two per compute unit (sn_gemm.hip)
    assert blocks >= min((rows + 31) // 32, 2 * torch.cuda.get_device_properties(0).multi_processor_count)
    _, gadd = _arena(rows, h, 7)
    x0, gadd0 = x.clone(), gadd.clone()
    for spike in _spike_positions(rows, h):
        x.copy_(x0), gadd.copy_(gadd0)
        if spike is not None:
            x[spike], gadd[spike] = -1.0, 1e6
        outs = []
        for with_max in (False, True):
            ha, dx_hi = _arena(rows, h, 8, fill=7.0)
            ga, gact = _arena(rows, h, 9, fill=7.0)
            dx_hi.fill_(7.0), gact.fill_(7.0)
            am = _maxima_buffer(blocks)
            args = (_p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), _p(dx_hi), _ld(dx_hi), _p(gact), _ld(gact),
                    _p(gadd), _ld(gadd), rows, J, C)
            if with_max:
                _lib.call("sn_linear_dgrad_elu_absmax_f32", *args, _p(am), _stream())
            else:
                _lib.call("sn_linear_dgrad_elu_f32", *args, _stream())
            assert _outside_untouched(ha, rows, h, 7.0) and _outside_untouched(ga, rows, h, 7.0)
            outs.append((dx_hi.clone(), gact.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), spike
        _check_maxima(am, blocks, outs[1][1], ("dgrad_elu", rows, J, C, spike))
        if spike is not None:
            assert float(outs[1][1][spike]) == 1e6 and float(am[:blocks].max()) == 1e6


def _seg_shape(rows):
    """(rows_per_seg, nseg) with whole meshes of at least 32 rows, or None (then the launch has no per-mesh vector)."""
    return {32: (32, 1), 33: (33, 1), 95: (95, 1), 1017: (113, 9), 8200: (1025, 8), 40001: (3077, 13)}.get(rows)


@pytest.mark.parametrize("rows", DGRAD_ROWS)
@pytest.mark.parametrize("J,C", DGRAD_JC)
def test_input_gradient_through_the_whole_activation_leaves_true_maxima(rows, J, C):
    """sn_linear_dgrad_eluseg_absmax_f32, with and without the per-mesh vector and the row mask: the maxima are those of what
    the kernel STORES — a huge per-mesh vector counts in the rows whose mask is 1 and not in the rows whose mask is 0."""
    W, cen, B, Cc, dy, x = _dgrad_operands(rows, J, C, rows + 2 * J + C)
    blocks = int(_lib.load().sn_linear_dgrad_absmax_blocks())
    _, gadd = _arena(rows, C, 7)
    x0, gadd0 = x.clone(), gadd.clone()
    shape = _seg_shape(rows)
    rng = np.random.default_rng(rows)
    cases = [("plain", sp) for sp in _spike_positions(rows, C)]
    if shape is not None:
        cases += [("segvec", None), ("segvec_masked", None), ("masked_row_spike", (rows - 1, C - 1))]
    for kind, spike in cases:
        x.copy_(x0), gadd.copy_(gadd0)
        segvec = rowmask = None
        per = 0
        if kind != "plain":
            per, nseg = shape
            sv = rng.standard_normal((nseg, C)).astype(np.float32)
            sv[nseg - 1, C // 2] = 1e6                              # the per-mesh term carries the maximum of the last mesh
            segvec = dev(sv)
            mask = np.ones(rows, np.float32)
            if kind != "segvec":
                mask[rows - per:] = 0.0                            # ... unless the mask removes it from every row of that mesh
                mask[::5] = 0.0
            rowmask = dev(mask)
            x[:, C // 2] = x[:, C // 2].abs() + 0.5                # elu' = 1 in that column
        if spike is not None:
            x[spike], gadd[spike] = -1.0, 1e6
        outs = []
        for with_max in (False, True):
            aa, gact = _arena(rows, C, 9, fill=7.0)
            gact.fill_(7.0)
            am = _maxima_buffer(blocks)
            args = (_p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), _p(segvec), per, _p(rowmask), _p(gact),
                    _ld(gact), _p(gadd), _ld(gadd), rows, J, C)
            if with_max:
                _lib.call("sn_linear_dgrad_eluseg_absmax_f32", *args, _p(am), _stream())
            else:
                _lib.call("sn_linear_dgrad_eluseg_f32", *args, _stream())
            assert _outside_untouched(aa, rows, C, 7.0)
            outs.append(gact.clone())
        assert torch.equal(outs[0], outs[1]), (kind, spike)
        _check_maxima(am, blocks, outs[1], ("dgrad_eluseg", rows, J, C, kind, spike))
        top = float(am[:blocks].max())
        if kind == "segvec":
            assert top > 9e5
        elif kind == "segvec_masked":
            assert top < 1e5
        elif spike is not None:
            assert float(outs[1][spike]) == 1e6 and top == 1e6


@pytest.mark.parametrize("lengths", [[32, 700, 45, 33, 2000], [5041, 5041], [40] * 37])
@pytest.mark.parametrize("J,C", DGRAD_JC)
def test_ragged_input_gradient_leaves_true_maxima(lengths, J, C):
    """sn_linear_dgrad_eluseg_ragged_absmax_f32 on the packed batches of test_ragged_mesh_entry_points."""
    from surfacenetworks_amd.operators import PackedSegments

    seg = PackedSegments(lengths, DEV)
    rows = seg.rows
    W, cen, B, Cc, dy, x = _dgrad_operands(rows, J, C, rows + 3 * J + C)
    blocks = int(_lib.load().sn_linear_dgrad_absmax_blocks())
    _, gadd = _arena(rows, C, 7)
    x0, gadd0 = x.clone(), gadd.clone()
    rng = np.random.default_rng(rows)
    sv0 = rng.standard_normal((seg.nseg, C)).astype(np.float32)
    for kind, spike in [("segvec", None)] + [("gadd", sp) for sp in _spike_positions(rows, C)]:
        x.copy_(x0), gadd.copy_(gadd0)
        sv = sv0.copy()
        if kind == "segvec":
            sv[seg.nseg - 1, C // 2] = 1e6
            x[:, C // 2] = x[:, C // 2].abs() + 0.5
        if spike is not None:
            x[spike], gadd[spike] = -1.0, 1e6
        segvec = dev(sv)
        outs = []
        for with_max in (False, True):
            aa, gact = _arena(rows, C, 9, fill=7.0)
            gact.fill_(7.0)
            am = _maxima_buffer(blocks)
            args = (_p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), _p(segvec), _p(seg.off_dev), seg.nseg,
                    _p(gact), _ld(gact), _p(gadd), _ld(gadd), rows, J, C)
            if with_max:
                _lib.call("sn_linear_dgrad_eluseg_ragged_absmax_f32", *args, _p(am), _stream())
            else:
                _lib.call("sn_linear_dgrad_eluseg_ragged_f32", *args, _stream())
            assert _outside_untouched(aa, rows, C, 7.0)
            outs.append(gact.clone())
        assert torch.equal(outs[0], outs[1]), (kind, spike)
        _check_maxima(am, blocks, outs[1], ("dgrad_eluseg_ragged", lengths[:2], J, C, kind, spike))
        top = float(am[:blocks].max())
        assert top > 9e5 if kind == "segvec" else (spike is None or (float(outs[1][spike]) == 1e6 and top == 1e6))


# ---- 2. consumer: the scale depends on max(dybound) and on nothing else ------------------------------------------------------------
DYBOUND_LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 2047, 2048, 4096, 14336, 14337, 16384, 16387, 20000, 40001]


def _flat_operands(rows, J, C, seed):
    rng = np.random.default_rng(seed)
    dy = dev(rng.standard_normal((rows, J)).astype(np.float32))
    x = dev((rng.standard_normal((rows, C)) * 1.5 + rng.standard_normal(C)).astype(np.float32))
    st = kernels.colstats(x)
    mean = (st[0] / rows).float()
    invstd = (1.0 / torch.sqrt((st[1] / rows - (st[0] / rows) ** 2).clamp_min(0) + 1e-5)).float()
    return dy, x, mean, invstd


@pytest.mark.parametrize("C", [128, 256])
def test_scale_of_the_bounded_weight_gradient_depends_on_the_maximum_alone(C):
    """The reduction over n_dybound inside wgrad16_k<CT, WgradHalf2> (unaligned pointer, eight-deep 16-byte loads, 16-byte remainder, scalar
    tail, the order of bit patterns across lanes): for every length, position of the maximum, alignment of the pointer and kind
    of filler the result has the bits of the launch that is handed [m] alone.  Fillers of m * 2^-20: a missed maximum moves the
    scale by twenty binary orders, the scaled dy then passes fp16's range (tests/test_wgrad_bounds.py:
    test_a_bound_that_is_too_small_or_too_large_shows_in_the_model)."""
    rows, J = 1000, 128
    dy, x, mean, invstd = _flat_operands(rows, J, C, C)
    m = float(dy.abs().max())
    want = kernels.wgrad(dy, x, mean, bounds=(torch.tensor([m], device=DEV), invstd, rows))
    assert bool(torch.isfinite(want).all())
    fillers = {"m*2^-20": m * 2.0 ** -20, "+0": 0.0, "-0": -0.0, "denormal": 1e-41}
    bad = []
    for n in DYBOUND_LENGTHS:
        for pos in sorted({0, n - 1, n // 2, (n - 1) // 4 * 4}):
            for off in (0, 1, 2, 3):
                buf = torch.empty(n + 4, device=DEV)
                assert buf.data_ptr() % 16 == 0
                for name, f in fillers.items():
                    buf.fill_(f)
                    arr = buf[off:off + n]
                    arr[pos] = m
                    G = kernels.wgrad(dy, x, mean, bounds=(arr, invstd, rows))
                    if not torch.equal(G, want):
                        bad.append((n, pos, 4 * off, name, bool(torch.isfinite(G).all())))
    assert not bad, bad[:20]


def test_all_zero_gradient_with_an_all_zero_bound():
    rows, J, C = 1000, 128, 256
    _, x, mean, invstd = _flat_operands(rows, J, C, 3)
    dy = torch.zeros(rows, J, device=DEV)
    for zeros in (torch.zeros(1, device=DEV), torch.zeros(777, device=DEV), -torch.zeros(5, device=DEV)):
        G, s = kernels.wgrad(dy, x, mean, want_colsum=True, bounds=(zeros, invstd, rows))
        assert bool((G == 0).all()) and bool((s == 0).all())


def test_bounded_weight_gradient_statuses():
    rows, J, C = 100, 128, 128
    dy, x, mean, invstd = _flat_operands(rows, J, C, 4)
    lib = _lib.load()
    G = torch.empty(J, C, device=DEV)
    ws_bytes = int(lib.sn_wgrad_workspace_bytes(rows, J, C))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    b = dy.abs().max().reshape(1)

    def call(dyb, n, inv, stat_rows):
        return lib.sn_wgrad_bounded_f32(_p(dy), _ld(dy), _p(x), _ld(x), _p(mean), rows, J, C, _p(G), None, _p(ws), ws_bytes, dyb, n,
                                        inv, stat_rows, _stream())

    assert call(_p(b), 1, _p(invstd), rows - 1) == -2            # SN_E_SHAPE: statistics over fewer rows than the operand has
    assert call(None, 1, _p(invstd), rows) == -1                 # SN_E_NULL: maxima announced, none given
    assert call(_p(b), 1, None, rows) == -1                      # SN_E_NULL: no inverse standard deviations
    assert call(_p(b), -1, _p(invstd), rows) == -1               # n_dybound < 0
    assert call(_p(b), 1, _p(invstd), rows) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(G).all())


# ---- 3. the three bounded entry points against float64 ----------------------------------------------------------------------------
WGRAD_JC = [(128, 128), (128, 256), (120, 128), (120, 256), (64, 128), (4, 256)]
KINDS = ["saturated", "constant", "spread"]


def _wgrad_operands(rows, J, C, kind, seed):
    """x as the first half of a NaN-filled concat buffer, dy with NaN rows before and after the view; operands of the two
    direct tests of the flat form (tests/test_dense_gpu.py) plus an exactly constant column."""
    rng = np.random.default_rng(seed)
    xn = rng.standard_normal((rows, C)).astype(np.float32)
    dyn = rng.standard_normal((rows, J)).astype(np.float32)
    if kind == "saturated":
        xn[:, ::3] = -1.0 + 1e-4 * xn[:, ::3]
        xn[:, 1::3] = 1000.0 + 0.5 * xn[:, 1::3]
    elif kind == "constant":
        xn = xn * 1.5 + rng.standard_normal(C).astype(np.float32)
        xn[:, 5] = 0.75
        xn[:, C - 1] = -3.0
    else:
        xn = ((rng.standard_normal((rows, C)) + 4 * rng.standard_normal(C)[None, :]) * np.exp2(rng.integers(-20, 21, size=C))[None, :]).astype(np.float32)
        dyn = (dyn * np.array([1e-12, 1e-6, 1.0, 1e3])[np.arange(rows) % 4][:, None]).astype(np.float32)
    cat = torch.full((rows + 6, 2 * C), float("nan"), device=DEV)
    x = cat[3:3 + rows, :C]
    x.copy_(dev(xn))
    da = torch.full((rows + 6, J + 8), float("nan"), device=DEV)
    dy = da[3:3 + rows, 4:4 + J]
    dy.copy_(dev(dyn))
    st = kernels.colstats(x)
    mean = (st[0] / rows).float()
    invstd = (1.0 / torch.sqrt((st[1] / rows - (st[0] / rows) ** 2).clamp_min(0) + 1e-5)).float()
    return dy, x, mean, invstd


def _check_against_float64(run, dy, x, mean, invstd, rows):
    """`run(bounds)` -> (G, dysum, seg_dysum | None).  The tolerances of the flat form's direct tests."""
    bound = dy.abs().max().reshape(1)
    got = run((bound, invstd, rows))
    base = run(None)
    G, G0 = got[0].double(), base[0].double()
    xc = x.double() - mean.double()
    ref = dy.double().t() @ xc
    scale = dy.double().abs().t() @ xc.abs()
    assert bool(torch.isfinite(got[0]).all())
    err, err0 = (G - ref).abs(), (G0 - ref).abs()
    # tests/test_dense_gpu.py::test_operands_spanning_more_than_2_28_along_the_contraction
    worst = float((err / scale.clamp_min(1e-300)).max())
    print(f"rows {rows}: max err / scale {worst:.3e} (bound {8 * 2.0 ** -24 * np.sqrt(rows):.3e}); max err {float(err.max()):.3e}, "
          f"unbounded {float(err0.max()):.3e}")
    assert bool((err <= 8 * 2.0 ** -24 * np.sqrt(rows) * scale).all()), worst
    # tests/test_dense_gpu.py::test_two_piece_weight_gradient_ignores_the_rows_past_the_end
    assert float(err.max()) <= 2.0 * float(err0.max()) + 1e-5 * float(ref.abs().max()) + 1e-6
    assert torch.equal(got[1], base[1])                           # the column sums do not go through the split
    if got[2] is not None:
        assert torch.equal(got[2], base[2])
    return ref, scale, xc


def _check_loose_bounds(run, dy, x, mean, invstd, rows, ref, scale, xc):
    """Bounds that are true but loose stay inside the header's contract (include/sn_spmm.h, sn_wgrad_*_bounded_f32): an element
    keeps 22 bits or 2^-39 of ITS OPERAND'S bound; the accumulation is the fp32 sum the tight tolerance already covers.
    Per term dy*xc, relative to |dy||xc|: a = h + l + r with |l| <= 2^-11 |a| (half an ulp of the 11-bit h) and |r| <= 2^-22 |a|
    (half an ulp of the 11-bit l), or |r| <= 2^-25 scaled = 2^-39 bound where l is denormal.  The kernel forms
    (h + l)(h' + l') - l l': the two representation errors give 2^-22 + 2^-22 + 2^-44, the dropped l l' at most
    2^-11 * 2^-11 = 2^-22 — together (3 + 2^-22) 2^-22."""
    top = float(dy.abs().max())
    sx = xc.abs().sum(0)[None, :]
    sdy = dy.double().abs().sum(0)[:, None]
    for fdy, fst in ((2.0, 1), (2.0 ** 10, 1), (1.0, 4), (1.0, 2 ** 20)):
        stat_rows = rows * fst
        G = run((torch.tensor([top * fdy], device=DEV), invstd, stat_rows))[0].double()
        xb = torch.from_numpy(wgrad_xbound(invstd.cpu().numpy(), stat_rows).astype(np.float64)).to(DEV)[None, :]
        allowed = (8 * 2.0 ** -24 * np.sqrt(rows) + (3 + 2.0 ** -22) * 2.0 ** -22) * scale + 2.0 ** -39 * (top * fdy) * sx + 2.0 ** -39 * xb * sdy
        assert bool(torch.isfinite(G).all()) and bool(((G - ref).abs() <= allowed).all()), (fdy, fst)


FLAT_ROWS = [1, 2, 7, 31, 32, 33, 255, 256, 1000, 33333, 400001]


def _flat_cases():
    """Every row count of test_wgrad_mfma with every (J, C) up to 33 333 rows, the operand kinds dealt round-robin; the
    400 001-row case (the expensive one) once per operand kind."""
    out = []
    for i, rows in enumerate(FLAT_ROWS[:-1]):
        for j, (J, C) in enumerate(WGRAD_JC):
            out.append((rows, J, C, KINDS[(i + j) % 3]))
    out += [(400001, 128, 256, "saturated"), (400001, 120, 128, "spread"), (400001, 4, 256, "constant")]
    return out


@pytest.mark.parametrize("rows,J,C,kind", _flat_cases())
def test_bounded_flat_form_against_float64(rows, J, C, kind):
    dy, x, mean, invstd = _wgrad_operands(rows, J, C, kind, rows + J + C)

    def run(bounds):
        G, s = kernels.wgrad(dy, x, mean, want_colsum=True, bounds=bounds)
        return G, s, None

    ref, scale, xc = _check_against_float64(run, dy, x, mean, invstd, rows)
    if rows in (33, 1000):
        _check_loose_bounds(run, dy, x, mean, invstd, rows, ref, scale, xc)


@pytest.mark.parametrize("nseg,per", [(1, 40), (3, 150), (7, 33), (64, 300), (65, 40), (300, 40), (2, 5041)])
@pytest.mark.parametrize("J,C", WGRAD_JC)
def test_bounded_seg_form_against_float64(nseg, per, J, C):
    rows = nseg * per
    dy, x, mean, invstd = _wgrad_operands(rows, J, C, KINDS[(nseg + J + C // 128) % 3], rows + J + C)
    run = lambda bounds: kernels.wgrad_seg(dy, x, mean, per, bounds=bounds)
    ref, scale, xc = _check_against_float64(run, dy, x, mean, invstd, rows)
    want_seg = dy.double().reshape(nseg, per, J).sum(1)
    assert float((run(None)[2].double() - want_seg).abs().max()) <= 1e-5 * float(dy.double().abs().reshape(nseg, per, J).sum(1).max()) + 1e-30
    if (nseg, per) == (3, 150):
        _check_loose_bounds(run, dy, x, mean, invstd, rows, ref, scale, xc)


@pytest.mark.parametrize("lengths", [[32, 700, 45, 33, 2000], [5041] * 3, [40] * 70, [33, 63, 64, 95]])
@pytest.mark.parametrize("J,C", WGRAD_JC)
def test_bounded_slabs_form_against_float64(lengths, J, C):
    from surfacenetworks_amd.operators import PackedSegments

    seg = PackedSegments(lengths, DEV)
    rows = seg.rows
    dy, x, mean, invstd = _wgrad_operands(rows, J, C, KINDS[(len(lengths) + J + C // 128) % 3], rows + J + C)
    run = lambda bounds: kernels.wgrad_slabs(dy, x, mean, seg, bounds=bounds)
    ref, scale, xc = _check_against_float64(run, dy, x, mean, invstd, rows)
    if len(lengths) == 4:
        _check_loose_bounds(run, dy, x, mean, invstd, rows, ref, scale, xc)


# ---- 4. the header's accuracy model, element by element ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("rows,nz_row", [(1, 0), (70, 0), (70, 33), (70, 69), (1000, 517)])
def test_split_keeps_what_the_header_promises(rows, nz_row, C, seed):
    """One non-zero row: G[j, c] = dy[j] * x[c], elements at 2^-k of the power of two below their operand's bound (for x: the
    bound the kernel scales by, 1.0625 sqrt(stat_rows) / xinvstd[c]).  Exact against float64 for k, m <= 17 where one factor
    fits the high piece (h*h, h*l and l*h each needed by some pair: tests/test_wgrad_bounds.py); at most 2^-39 of the bound
    times the other factor for 17 < k <= 39 (include/sn_spmm.h: "2^-25 of the scaled unit (2^-39 of the bound) in absolute
    terms")."""
    p = split_probe_operands(128, C, rows, nz_row, seed)
    bounds = (dev(np.array([p["bound"]], np.float32)), dev(p["xinvstd"]), p["stat_rows"])
    G = kernels.wgrad(dev(p["dy"]), dev(p["x"]), dev(p["center"]), bounds=bounds).cpu().numpy().astype(np.float64)
    assert np.isfinite(G).all()
    ex = p["exact"]
    wrong = np.argwhere(ex & (G != p["ref"]))
    assert wrong.size == 0, [(int(j), int(c), int(p["k"][j]), int(p["m"][c]), int(p["kbits"][j]), int(p["mbits"][c])) for j, c in wrong[:10]]
    err = np.abs(G - p["ref"])
    assert (err <= 2.0 ** -39 * float(p["bound"]) * np.abs(p["x_row"])[None, :])[p["loose_dy"]].all()
    assert (err <= 2.0 ** -39 * p["xbound"].astype(np.float64)[None, :] * np.abs(p["dy_row"])[:, None])[p["loose_x"]].all()
    assert float(pow2_up_for(p["bound"]).reshape(-1)[0]) * float(p["bound"]) >= 2.0 ** 14


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("rows,nz_row", [(1, 0), (40, 7), (1000, 999)])
def test_elements_at_a_bound_at_the_top_of_its_binade(rows, nz_row, C):
    """The upper end of the range contract ("scaled so that their bound lands in [2^14, 2^15)", include/sn_spmm.h): dy elements
    equal to a bound whose mantissa is all ones, x elements equal to their column's bound within 2^-12 of a power of two.  Scaled
    one binary order higher they would pass fp16's 65504 (tests/test_wgrad_bounds.py checks that premise).  Finite, and 22
    significant bits of every element: the tolerances are those the host test derives and the numpy model meets."""
    p = top_of_binade_operands(128, C, rows, nz_row)
    bounds = (dev(np.array([p["bound"]], np.float32)), dev(p["xinvstd"]), p["stat_rows"])
    G = kernels.wgrad(dev(p["dy"]), dev(p["x"]), dev(p["center"]), bounds=bounds).cpu().numpy().astype(np.float64)
    assert np.isfinite(G).all()
    err, ref = np.abs(G - p["ref"]), np.abs(p["ref"])
    assert (err <= 2.0 ** -22 * ref)[:, p["pow2_x"]].all()
    assert (err <= ((3 + 2.0 ** -22) * 2.0 ** -22 + 2 * 2.0 ** -24) * ref).all()


# ---- 5. audit of a real training step -------------------------------------------------------------------------------------------
class _Audit:
    """Wrappers of kernels.wgrad / wgrad_seg / wgrad_slabs that check, on the device, every bound handed over."""

    def __init__(self, monkeypatch):
        self.records, self.unbounded = [], 0
        for name in ("wgrad", "wgrad_seg", "wgrad_slabs"):
            monkeypatch.setattr(kernels, name, self._wrap(name, getattr(kernels, name)))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*args, **kw):
            bound = sig.bind(*args, **kw)
            dy, x, center, bounds = (bound.arguments.get(k) for k in ("dy", "x", "center", "bounds"))
            if bounds is None:
                self.unbounded += 1
            else:
                dyb, invstd, stat_rows = bounds
                top, am = float(dy.abs().max()), float(dyb.max())
                xc = (x.double() - (center.double() if center is not None else 0)).abs().max(0)[0]
                xb = np.sqrt(float(stat_rows)) / invstd.double()
                self.records.append(dict(form=name, rows=dy.shape[0], J=dy.shape[1], C=x.shape[1], true=am >= top, exact=am == top,
                                         x_ok=bool((xc <= xb).all()), rows_ok=stat_rows >= dy.shape[0], top=top, am=am, stat_rows=int(stat_rows),
                                         x_ratio=float((xc / xb).max())))
            return fn(*args, **kw)
        return wrapped

    def assert_all(self, bounded, unbounded):
        bad = [r for r in self.records if not (r["true"] and r["exact"] and r["x_ok"] and r["rows_ok"])]
        assert not bad, bad[:5]
        assert (len(self.records), self.unbounded) == (bounded, unbounded)


def _bn_fc_layers(model):
    return sum(1 for name, _ in model.named_modules() if name.split(".")[-1].startswith("bn_fc"))


def _arap_step(model_name, packed, edit_below=None):
    from helpers import deterministic_init
    from surfacenetworks_amd import arap

    ds_kind = "dir" if model_name == "dir" else "lap"
    ds = arap.ClothSequences([(12, 11), (9, 13), (10, 10)], frames=45, op_frames=2, seed=3, device=DEV, model=ds_kind)
    seq, off = np.array([0, 1, 2, 1]), np.array([0, 0, 0, 0])
    make = {"dir": arap.DirModel, "lap": arap.Model, "avg": arap.AvgModel}[model_name]
    model = deterministic_init(make(), 4).to(DEV).train()
    b = ds.sample_batch(4, None, seq_ids=seq, offsets=off, packed=packed)
    if edit_below is not None:                 # the gradient of this block's output is edited in place before the block reads it
        def doubled(g):
            g.mul_(2)

        getattr(model, edit_below).register_forward_hook(lambda mod, args, out: out.register_hook(doubled) and None)
    loss, _ = arap.forward_loss(model, b, 4)
    loss.backward()
    return model


@pytest.mark.parametrize("model_name,packed", [("dir", False), ("dir", True), ("lap", False), ("avg", False)])
def test_every_bound_a_training_step_hands_over_is_true(model_name, packed, monkeypatch):
    """One forward + backward of the ARAP models on a padded batch of three mesh sizes (masks with padded rows) and on the packed
    ragged batch (wgrad_slabs), launch plans off so that the Python wrappers run: max(dybound) == max |dy| for the operand as it
    arrives, |x - center| within sqrt(stat_rows) / xinvstd per column, stat_rows >= rows.  The models are fifteen residual blocks
    (arap.DirModel: DirResNet2 / AvgResNet2 alternating; arap.Model: LapResNet2 / AvgResNet2) of two BatchNorm+Linear layers
    (bn_fc0, bn_fc1) each (arap.AvgModel: fifteen AvgResNet2): thirty weight gradients, every one fed by a producer that leaves maxima, take the bounded form; the
    last layer (conv2, BatchNorm first) reads the gradient of the loss, which carries none: one unbounded call."""
    from surfacenetworks_amd import plans

    audit = _Audit(monkeypatch)
    plans.set_enabled(False)
    try:
        model = _arap_step(model_name, packed)
    finally:
        plans.set_enabled(True)
    forms = {r["form"] for r in audit.records}
    print(model_name, packed, len(audit.records), "bounded,", audit.unbounded, "unbounded", sorted(forms),
          "max x ratio", max(r["x_ratio"] for r in audit.records))
    assert _bn_fc_layers(model) == 30
    audit.assert_all(bounded=30, unbounded=1)
    if packed:
        assert "wgrad_slabs" in forms
    elif model_name == "dir":
        assert "wgrad_seg" in forms


def test_an_edited_gradient_falls_back_to_the_unbounded_form(monkeypatch):
    """A tensor hook doubles, in place, the gradient that block rn7 of the Laplacian model receives for its output: the maxima
    the producer (the input gradient of rn8) noted describe the tensor before the edit, take_absmax compares the version counter
    and the first weight gradient that reads it (bn_fc1 of rn7) runs unbounded.  Every bound that IS handed over stays true and
    exact — without the version check the stale maximum (half the true one) would arrive.  The gradients of the edited step
    agree with the SAME edited step run with no maxima produced at all (every weight gradient on the three-piece form, itself
    held to float64 by tests/test_dense_gpu.py) to the tolerance two summation orders of one ARAP model are held to
    (tests/test_dense_gpu.py::test_arap_model_with_and_without_tile_sums: 2e-5 of the gradient's norm)."""
    from surfacenetworks_amd import plans

    flat = lambda m: torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double()
    plans.set_enabled(False)
    try:
        clean = flat(_arap_step("lap", False))
        audit = _Audit(monkeypatch)
        got = flat(_arap_step("lap", False, edit_below="rn7"))
        audit.assert_all(bounded=29, unbounded=2)
        audit.records.clear()
        audit.unbounded = 0
        monkeypatch.setattr(kernels, "absmax_wanted", lambda: False)
        want = flat(_arap_step("lap", False, edit_below="rn7"))
        audit.assert_all(bounded=0, unbounded=31)
    finally:
        plans.set_enabled(True)
    assert bool(torch.isfinite(got).all())
    rel = float((got - want).norm() / want.norm())
    print("edited step, bounded with fall-back against all-unbounded:", rel)
    assert rel < 2e-5
    assert float((got - clean).norm()) > 1e-3 * float(clean.norm())        # the edit took place


def _record_step(monkeypatch, step):
    from surfacenetworks_amd import plans

    audit = _Audit(monkeypatch)
    plans.set_enabled(False)
    try:
        model = step()
    finally:
        plans.set_enabled(True)
    shapes = sorted({(r["form"], r["J"], r["C"]) for r in audit.records})
    print(len(audit.records), "bounded,", audit.unbounded, "unbounded", shapes)
    return audit, model


def test_mesh_mnist_dirac_step_hands_over_true_bounds(monkeypatch):
    """mesh_mnist.DirModel: five DirResNet2(64) blocks (two BatchNorm+Linear layers each, 128 -> 64 on the concat buffer) and
    the head bn_conv2, a 64 -> 64 layer whose 64-wide operand takes the paired-rows form of functional._centered_wgrad."""
    from helpers import deterministic_init
    from surfacenetworks_amd import mesh_mnist

    def step():
        ds = mesh_mnist.MeshDigits(4, seed=6, device=DEV, vmin=40, vmax=56, model="dir")
        b = ds.sample_batch(4, np.random.default_rng(1), ids=np.arange(4))
        model = deterministic_init(mesh_mnist.DirModel(), 10).to(DEV).train()
        mesh_mnist.forward_loss(model, b)[0].backward()
        return model

    audit, model = _record_step(monkeypatch, step)
    assert _bn_fc_layers(model) == 10
    audit.assert_all(*MNIST_DIR_CALLS)


def test_faust_laplacian_pair_hands_over_true_bounds(monkeypatch, golden_dir):
    """dense_correspondence.SiameseModel("lap", 15): two towers of fifteen blocks (LapResNet2 / AvgResNet2 alternating, two
    BatchNorm+Linear layers each) that share their weights; each tower's backward runs its own thirty weight gradients."""
    from helpers import deterministic_init
    from product_checks import csr_of, load
    from surfacenetworks_amd import dense_correspondence
    from surfacenetworks_amd.operators import OperatorPool

    def step():
        g = load(golden_dir, "models_reference.npz")
        rb = load(golden_dir, "ragged_batch.npz")
        nv = int(rb["nv"])
        L1 = OperatorPool([csr_of(load(golden_dir, "ops_delaunay150.npz"), "L")], DEV).assemble([0], nv, nv)
        lA, lB = torch.from_numpy(g["faust_lA"]).to(DEV), torch.from_numpy(g["faust_lB"]).to(DEV)
        tX = [(torch.from_numpy(g["faust_GA"]).to(DEV), lA, torch.argsort(lA))]
        tY = [(torch.from_numpy(g["faust_GB"]).to(DEV), lB, torch.argsort(lB))]
        cA = torch.from_numpy(rb["coords"][1:2]).to(DEV)
        cB = torch.from_numpy(rb["coords"][1:2] * 1.1 + 0.02).to(DEV)
        mask = torch.from_numpy(rb["mask"][1:2]).to(DEV)
        model = deterministic_init(dense_correspondence.SiameseModel("lap", 15), 11).train().to(DEV)
        out = model([L1, mask], [L1, mask], cA, cB)
        dense_correspondence.loss_fun_delta_cross_entropy(out, tX, tY).backward()
        return model

    audit, model = _record_step(monkeypatch, step)
    assert _bn_fc_layers(model) == 30
    audit.assert_all(*FAUST_LAP_CALLS)


@pytest.mark.parametrize("rows", [2, 64, 66, 2474, 40000])
def test_paired_rows_form_of_a_64_wide_operand_arrives_with_true_bounds(rows, monkeypatch):
    """functional._centered_wgrad reads a 64-wide x as rows/2 rows of 128 (two consecutive rows side by side, dy likewise) and
    hands the SAME maxima and row count over with the inverse standard deviations repeated: the bound of every column of the
    paired operand must still hold (stat_rows counts the original rows: at least twice the paired ones), and the result is
    held to float64 as the flat form is (tests/test_dense_gpu.py::test_operands_spanning_more_than_2_28_along_the_contraction)."""
    from surfacenetworks_amd import functional as snF

    J = C = 64
    rng = np.random.default_rng(rows)
    dy = dev(rng.standard_normal((rows, J)).astype(np.float32))
    x = dev((rng.standard_normal((rows, C)) * 1.5 + 3 * rng.standard_normal(C)).astype(np.float32))
    x[::2, 7] += 40.0                                # a column whose even and odd rows differ: one statistic covers both halves
    st = kernels.colstats(x)
    mean = (st[0] / rows).float()
    invstd = (1.0 / torch.sqrt((st[1] / rows - (st[0] / rows) ** 2).clamp_min(0) + 1e-5)).float()
    audit = _Audit(monkeypatch)
    G, s = snF._centered_wgrad(dy, x, mean, (dy.abs().max().reshape(1), invstd, rows))
    audit.assert_all(bounded=1, unbounded=0)
    r = audit.records[0]
    assert (r["rows"], r["J"], r["C"]) == (rows // 2, 128, 128) and r["stat_rows"] >= 2 * r["rows"]
    xc = x.double() - mean.double()
    ref = dy.double().t() @ xc
    scale = dy.double().abs().t() @ xc.abs()
    assert bool(torch.isfinite(G).all()) and bool(((G.double() - ref).abs() <= 8 * 2.0 ** -24 * np.sqrt(rows) * scale).all())
    assert torch.allclose(s, dy.double().sum(0), rtol=1e-9, atol=1e-3)            # (tests/test_dense_gpu.py::test_ragged_mesh_entry_points)


# mesh_mnist.DirModel: ten bn_fc layers.  Nine read a gradient written by a kernel that leaves maxima.  Two calls are unbounded:
# bn_fc1 of the last block reads the input gradient of the head bn_conv2, a 64 -> 64 layer that no input-gradient kernel takes
# (C must be 128 or 256: no maxima), and bn_conv2 itself reads a gradient formed by framework ops.  So the paired-rows form of
# functional._centered_wgrad (bn_conv2's 64-wide operand) never receives bounds in a training step: its hand-over is pinned
# directly by test_paired_rows_form_of_a_64_wide_operand_arrives_with_true_bounds.
MNIST_DIR_CALLS = (9, 2)
# SiameseModel("lap", 15): thirty bn_fc layers, run by each of the two towers' backward passes; conv2 of each tower unbounded.
FAUST_LAP_CALLS = (60, 2)
