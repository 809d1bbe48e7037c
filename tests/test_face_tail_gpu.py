"""Raw face gradients (blocks.DEFER_FACE_TAIL): the input-gradient GEMM of a Dirac block's face stage leaves its low half as the
bare product and does not read elu(f); the previous block's DiA^T product (or one finishing launch) applies the BatchNorm tail and
the activation derivative.  Same operations in the same order as the GEMM's own epilogue, so everything here is compared bit for
bit with today's two-kernel result: kernels, the chained blocks (eager, planned, every storage form) and the refusals."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import _lib, blocks, kernels, plans  # noqa: E402
from surfacenetworks_amd import functional as snF  # noqa: E402
from surfacenetworks_amd.kernels import _ld, _p, _stream  # noqa: E402

CANARY = 7.0


@pytest.fixture(autouse=True)
def _clean():
    if not kernels._split_gemm():
        pytest.skip("the fused input gradient exists in the 16-bit matrix-pipe kernels only (SN_GEMM_VARIANT=0 is the A/B baseline)")
    plans.reset()
    plans.set_enabled(True)
    yield
    blocks.DEFER_FACE_TAIL = True
    plans.set_enabled(True)
    snF.set_dirac_format("q3")
    kernels.clear_absmax()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _arena(rows, width, seed=None, fill=float("nan"), pad_rows=3, pad_cols=8):
    """`view` = rows x width (random values with a seed) inside an arena filled with `fill`."""
    a = torch.full((rows + 2 * pad_rows, width + 2 * pad_cols), fill, device=DEV)
    v = a[pad_rows:pad_rows + rows, pad_cols:pad_cols + width]
    if seed is not None:
        v.copy_(torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32)))
    return a, v


def _outside_untouched(arena, rows, width, pad_rows=3, pad_cols=8):
    m = torch.ones_like(arena, dtype=torch.bool)
    m[pad_rows:pad_rows + rows, pad_cols:pad_cols + width] = False
    return bool((arena[m] == CANARY).all())


# ---- the GEMM ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 31, 33, 16391])
@pytest.mark.parametrize("J,C", [(128, 256), (64, 128)])
def test_raw_low_half_input_gradient_equals_the_fused_one(rows, J, C):
    """sn_linear_dgrad_elu_rawlow_f32 against sn_linear_dgrad_elu_absmax_f32 on the same operands (strided views inside canary
    arenas): dx_hi identical; the raw low half, finished in place by sn_elu_tail_finish_f32, identical to gact; nothing written
    around either output; and a NaN-filled x[:, :C/2] changes nothing — the raw form does not read it.  16 391 rows: more than two
    32-row tiles for every workgroup of a 256-workgroup grid, and a ragged last tile."""
    h = C // 2
    rng = np.random.default_rng(rows + J + C)
    W = dev((rng.standard_normal((J, C)) / np.sqrt(J)).astype(np.float32))
    cen, B, Cc = [dev(rng.standard_normal(C).astype(np.float32)) for _ in range(3)]
    _, dy = _arena(rows, J, 1)
    _, x = _arena(rows, C, 2)
    dx0 = torch.empty(rows, h, device=DEV)
    g0 = torch.empty(rows, h, device=DEV)
    _lib.call("sn_linear_dgrad_elu_absmax_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(cen), _p(B), _p(Cc), _p(dx0), h,
              _p(g0), h, None, 0, rows, J, C, None, _stream())
    assert bool(torch.isfinite(dx0).all()) and bool(torch.isfinite(g0).all())
    raws = []
    for nan_low in (False, True):
        xs = x
        if nan_low:
            _, xs = _arena(rows, C)
            xs.copy_(x)
            xs[:, :h] = float("nan")
        ha, dx_hi = _arena(rows, h, fill=CANARY)
        ga, graw = _arena(rows, h, fill=CANARY)
        _lib.call("sn_linear_dgrad_elu_rawlow_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(xs), _ld(xs), _p(cen), _p(B), _p(Cc),
                  _p(dx_hi), _ld(dx_hi), _p(graw), _ld(graw), rows, J, C, _stream())
        assert _outside_untouched(ha, rows, h) and _outside_untouched(ga, rows, h), nan_low
        assert torch.equal(dx_hi, dx0), nan_low
        raws.append(graw.clone())
        e = x[:, :h]
        _lib.call("sn_elu_tail_finish_f32", _p(graw), _ld(graw), _p(e), _ld(e), _p(cen[:h]), _p(B[:h]), _p(Cc[:h]), rows, h, _stream())
        assert _outside_untouched(ga, rows, h), nan_low
        assert torch.equal(graw, g0), nan_low
    assert torch.equal(raws[0], raws[1])


# ---- the product ---------------------------------------------------------------------------------------------------------------------
def _q3_random(Mb, Kb, per_row, seed):
    """Quaternion-packed operator with `per_row` blocks in every block row except every fifth one and the last, which are empty."""
    rng = np.random.default_rng(seed)
    counts = np.full(Mb, per_row, dtype=np.int64)
    if Mb > 1:
        counts[4::5] = 0
        counts[-1] = 0
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nblk = int(rowptr[-1])
    q = np.empty((nblk, 4), dtype=np.float32)
    q[:, :3] = rng.standard_normal((nblk, 3)).astype(np.float32)
    live = int((counts > 0).sum())                         # ascending, distinct block columns: start + 5 j
    cols = (rng.integers(0, Kb - 5 * per_row, size=(live, 1)) + 5 * np.arange(per_row)[None, :]).astype(np.int32).ravel()
    q[:, 3] = cols.view(np.float32)
    return dev(rowptr), dev(q), counts


def _tail_operands(Mb, C, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((Mb, C)).astype(np.float32)
    pick = rng.integers(0, 4, size=(Mb, C))
    e[pick == 0] = 0.0                                     # exactly 0
    e[pick == 1] = np.float32(-1.0 + 1e-4)                 # saturated
    e[0, :4] = [1.5, -0.5, 0.0, np.float32(-1.0 + 1e-4)]   # (every kind is there at the smallest size too)
    p = rng.standard_normal((Mb, C)).astype(np.float32)
    vecs = [(np.where(rng.random(C) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 4, C)).astype(np.float32) for _ in range(3)]
    return dev(e), dev(p), [dev(v) for v in vecs]


def _tail_product_check(Mb, Kb, per_row, N, seed):
    C = 4 * N
    rp, q, counts = _q3_random(Mb, Kb, per_row, seed)
    e, p, (cen, B, Cc) = _tail_operands(Mb, C, seed + 1)
    x = dev(np.random.default_rng(seed + 2).standard_normal((Kb, C)).astype(np.float32))
    blocks_ = int(_lib.load().sn_spmm_q3_absmax_blocks(Mb, N))
    # today's two kernels: the finished gradient (stand-alone finishing launch on a copy), then the product that adds it
    g = p.clone()
    kernels.elu_tail_finish(g, e, (cen, B, Cc))
    y0 = torch.empty(Mb, C, device=DEV)
    am0 = torch.full((blocks_ + 8,), 3e38, device=DEV)
    _lib.call("sn_spmm_q3_elubwd_absmax_f32", _p(rp), _p(q), Mb, Kb, int(q.shape[0]), _p(x), _ld(x), 4, N, _p(e), _ld(e), _p(g), _ld(g),
              _p(y0), _ld(y0), 4, _p(am0), _stream())
    ya = torch.full((Mb, 2 * C), CANARY, device=DEV)
    y = ya[:, C:]
    am = torch.full((blocks_ + 8,), 3e38, device=DEV)
    p_before = p.clone()
    _lib.call("sn_spmm_q3_elubwd_tail_absmax_f32", _p(rp), _p(q), Mb, Kb, int(q.shape[0]), _p(x), _ld(x), 4, N, _p(e), _ld(e), _p(p),
              _ld(p), _p(cen), _p(B), _p(Cc), _p(y), _ld(y), 4, _p(am), _stream())
    assert bool(torch.isfinite(y0).all())
    assert torch.equal(y, y0) and bool((ya[:, :C] == CANARY).all())
    assert torch.equal(am, am0) and bool((am[blocks_:] == 3e38).all())
    assert torch.equal(p, p_before)                        # the raw gradient is an operand: not written
    empty = torch.from_numpy(counts == 0).to(DEV)
    if bool(empty.any()):                                  # block rows without blocks receive the finished gradient (A·X = 0)
        assert torch.equal(y[empty], g[empty])


@pytest.mark.parametrize("Mb", [1, 7, 33, 100])
@pytest.mark.parametrize("per_row", [3, 6])
@pytest.mark.parametrize("N", [32, 16])
def test_product_finishes_a_raw_gradient_in_its_store(Mb, per_row, N):
    """sn_spmm_q3_elubwd_tail_absmax_f32 fed the raw gradient against the plain fused product fed the finished one: Y and the
    per-workgroup maxima identical.  33 and 100 block rows are no multiple of a workgroup's 32; empty block rows included; E
    positive, negative, exactly 0 and saturated; the channel vectors span 1e-6 .. 1e4."""
    _tail_product_check(Mb, 40, per_row, N, seed=Mb + per_row + N)


@pytest.mark.parametrize("N", [32, 16])
def test_product_finishes_a_raw_gradient_in_the_deep_launch_shape(N):
    """The launcher takes the deep shape (spmm_q3_lds_epi, 4 waves per SIMD) only for more than 4 blocks per block row AND a grid
    of at least 8 workgroups per compute unit: the smallest operator that gets there on this device, plus one ragged workgroup."""
    rpb = 256 // (N // 4)
    Mb = 8 * torch.cuda.get_device_properties(0).multi_processor_count * rpb + 5
    _tail_product_check(Mb, 512, 6, N, seed=N)


# ---- chained blocks ------------------------------------------------------------------------------------------------------------------
def _batch_ops(fmt):
    import scipy.sparse as sp

    from surfacenetworks_amd import mesh_ops
    from surfacenetworks_amd.operators import SparseOperator

    snF.set_dirac_format(fmt)
    Dis, DiAs = [], []
    for k in range(2):
        V, F = mesh_ops.grid_cloth(5, 7, np.random.default_rng(k))
        assert V.shape[0] == 35 and F.shape[0] == 48
        ops = mesh_ops.mesh_operators(V, F)
        Dis.append(ops["Di"])
        DiAs.append(ops["DiA"])
    mk = lambda mats: SparseOperator.from_scipy(sp.block_diag(mats, format="csr").astype(np.float32), DEV)  # noqa: E731
    return mk(Dis), mk(DiAs)


def _modules(C):
    from surfacenetworks_amd import utils_pt as U

    torch.manual_seed(C)
    dirs = [U.DirResNet2(C).to(DEV).train() for _ in range(3)]
    avgs = [U.AvgResNet2(C).to(DEV).train() for _ in range(2)]
    return dirs, avgs


def _chain(mods, Di, DiA, C, need_f, seed, hook=None):
    """Three Dirac blocks (the first with f=None) with a global-average block between each pair, as arap.DirModel chains them;
    returns every parameter gradient and the input gradient."""
    dirs, avgs = mods
    for m in dirs + avgs:
        m.zero_grad()
    g = torch.Generator(device=DEV).manual_seed(seed)
    v0 = torch.randn(2, 35, C, device=DEV, generator=g).requires_grad_(True)
    wv = torch.randn(2, 35, C, device=DEV, generator=g)
    wf = torch.randn(2, 48, C, device=DEV, generator=g)
    mask = torch.ones(2, 35, 1, device=DEV)
    v, f = v0, None
    for i in range(3):
        v, f = dirs[i](Di, DiA, v, f, f_out_needed=need_f, num_faces=48, avg_next=i < 2)
        if hook is not None and i == 0:
            f.register_hook(hook)
        if i < 2:
            v = avgs[i](None, mask, v)
    loss = (v * wv).sum()
    if need_f:
        loss = loss + (f * wf).sum()
    loss.backward()
    kernels.clear_absmax()
    return [v0.grad.clone()] + [p.grad.clone() for m in dirs + avgs for p in m.parameters()]


@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("fmt", ["q3", "bsr4", "csr"])
def test_chained_blocks_give_the_same_gradients_with_and_without_deferral(C, fmt):
    """2 grid meshes of 5 x 7 vertices (70 vertex rows, 96 face rows).  Every parameter gradient and the input gradient, bit for
    bit, between DEFER_FACE_TAIL off (eager: today's path) and on — eager, through launch plans on the recording call, and on a
    second planned call with fresh tensors.  bsr4 / csr operators take the finishing-kernel path."""
    Di, DiA = _batch_ops(fmt)
    mods = _modules(C)
    want = {}
    for seed in (1, 2):
        blocks.DEFER_FACE_TAIL = False
        plans.set_enabled(False)
        want[seed] = _chain(mods, Di, DiA, C, False, seed)
        assert all(bool(torch.isfinite(t).all()) for t in want[seed])
    blocks.DEFER_FACE_TAIL = True
    got = _chain(mods, Di, DiA, C, False, 1)
    assert all(torch.equal(a, b) for a, b in zip(got, want[1])), "eager, deferred"
    plans.set_enabled(True)
    for seed in (1, 2, 2):                                  # recorded, recorded (nothing new), replayed on fresh tensors
        got = _chain(mods, Di, DiA, C, False, seed)
        assert all(torch.equal(a, b) for a, b in zip(got, want[seed])), ("planned, deferred", seed)
    st = plans.stats()
    if fmt == "q3" and C == 128:                            # (the headline's form: every block direction ran from its plan)
        assert st["dirac_bwd"]["replayed"] >= 9 and st["dirac_bwd"]["refused"] == 0, st
    blocks.DEFER_FACE_TAIL = False                         # (and the switch is part of a planned block's signature)
    got = _chain(mods, Di, DiA, C, False, 2)
    assert all(torch.equal(a, b) for a, b in zip(got, want[2])), "planned, not deferred"


def _launched(monkeypatch):
    names = []
    orig = _lib.call

    def spy(name, *a):
        names.append(name)
        return orig(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    return names


def test_deferral_needs_a_producer_that_ran_without_f(monkeypatch):
    """need_f=True: the face output has another consumer (here: the loss), so every block finishes its own gradient — no raw
    launch, no tail.  need_f=False: blocks 2 and 3 defer, blocks 1 and 2 finish in their DiA^T product."""
    plans.set_enabled(False)
    Di, DiA = _batch_ops("q3")
    mods = _modules(128)
    names = _launched(monkeypatch)
    _chain(mods, Di, DiA, 128, True, 1)
    assert "sn_linear_dgrad_elu_rawlow_f32" not in names and "sn_spmm_q3_elubwd_tail_absmax_f32" not in names
    assert "sn_elu_tail_finish_f32" not in names and names.count("sn_linear_dgrad_elu_absmax_f32") >= 5
    del names[:]
    _chain(mods, Di, DiA, 128, False, 1)
    assert names.count("sn_linear_dgrad_elu_rawlow_f32") == 2 and names.count("sn_spmm_q3_elubwd_tail_absmax_f32") == 2
    assert "sn_elu_tail_finish_f32" not in names
    del names[:]
    blocks.DEFER_FACE_TAIL = False
    _chain(mods, Di, DiA, 128, False, 1)
    assert "sn_linear_dgrad_elu_rawlow_f32" not in names and "sn_spmm_q3_elubwd_tail_absmax_f32" not in names


@pytest.mark.parametrize("planned", [False, True])
def test_a_raw_gradient_whose_tail_was_dropped_is_an_error(planned):
    """kernels.clear_absmax() between the backward of the block that left its face gradient raw and the backward of the block
    that has to finish it (a tensor hook on the face features in between): loud, never a silent use of an unfinished gradient."""
    plans.set_enabled(planned)
    Di, DiA = _batch_ops("q3")
    mods = _modules(128)
    if planned:
        _chain(mods, Di, DiA, 128, False, 1)               # (the plans exist: the failing call is a pure replay)

    def drop(_g):
        kernels.clear_absmax()

    with pytest.raises(RuntimeError, match="left raw"):
        _chain(mods, Di, DiA, 128, False, 1, hook=drop)
    torch.cuda.synchronize()
