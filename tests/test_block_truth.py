"""block_truth.py on the CPU: the product's host logic (autograd nodes, hand-offs, per-stage functions) on the oracle-backed
kernels of the `cpu_kernels` seam, held to the float64 blocks tensor by tensor with the same helper, truth, metrics and
conditioning asserts as tests/test_block_truth_gpu.py.

Forms run here: whole-block nodes and per-stage functions of chains (a) to (e) at C = 128 and 64 on the 11-mesh batch, in train
and eval mode, f=None and torch.zeros, f_out_needed False and True, avg_next given and not said; the global-average block on the
33-mesh, the padded ragged and the packed batch.
GPU only (the seam has no such kernel or refuses the switch): the storage forms (q3 / bsr4 / csr, rb4 / ring: the host twins
share one arithmetic), blocks.DEFER_FACE_TAIL (a raw face gradient needs the device GEMM), launch plans, the tile-sum
hand-offs (kernels.tile_sums_supported() is False here) and the merged / separate launches of the averaging backward.

Those last two are exercised here for their ORDER only: test_average_block_launches_what_it_always_launched lists the launchers
one AvgResNet2 forward + backward calls, in every branch of the block, with stand-ins composed from the twins for what the seam lacks."""
import pytest
import torch

import block_truth as bt
from block_truth import Case, Form


@pytest.fixture(autouse=True)
def _clean(cpu_kernels):
    yield
    bt.restore()


CASES = [(Case(chain, C, "u11", need_f=(chain == "dir1")), Form(whole=whole))
         for chain in ("dir3", "lap3", "dir1", "avg1", "conv") for C in (128, 64) for whole in (True, False)]
CASES += [
    (Case("dir3", 128, "u11", train=False), Form()),
    (Case("lap3", 128, "u11", train=False), Form()),
    (Case("avg1", 128, "u11", train=False), Form()),
    (Case("dir3", 128, "u11", need_f=True), Form()),
    (Case("dir3", 128, "u11"), Form(fnone=False)),
    (Case("dir3", 128, "u11"), Form(avg_next="none")),
    (Case("lap3", 128, "u11"), Form(avg_next="none", lap="csr")),
    (Case("avg1", 128, "u33"), Form()),
    (Case("avg1", 128, "ragged"), Form()),
    (Case("avg1", 128, "packed"), Form()),
    (Case("avg1", 128, "packed"), Form(whole=False)),
    (Case("dir3", 128, "packed"), Form()),
]


@pytest.mark.parametrize("case,form", CASES, ids=lambda x: "-".join(str(v) for v in x) if isinstance(x, Case) else bt._form_text(x))
def test_blocks_equal_the_float64_blocks_tensor_by_tensor(case, form):
    """Every output, input gradient, parameter gradient and BatchNorm buffer of the chain, whole tensor and worst slice, as close
    to float64 as the float32 reference is (x 4): block_truth.check."""
    rows = bt.check(case, form, "cpu")
    names = {r[1] for r in rows}
    assert "grad.v0" in names and "out.v" in names
    if case.chain in ("dir3", "lap3"):
        assert len(names) == 2 + (1 if case.need_f else 0) + 5 * 14, sorted(names)       # 5 modules x (8 gradients + 6 buffers)
        assert {"blk2.bn_fc1.fc.bias.grad", "blk0.bn_fc0.bn.bias.grad", "avg1.bn_fc0.bn.num_batches_tracked"} <= names


def test_slice_metric_sees_what_the_whole_tensor_metric_hides():
    """A (128, 256) gradient whose second half is 100 times smaller than the first: a 1 % error in one small column is 1e-4 of
    the tensor's maximum and 1e-3 under the 0.1 floor's reduced sensitivity — or 1e-2 where its row or column stands alone."""
    import numpy as np

    from helpers import rel_err

    rng = np.random.default_rng(0)
    t = rng.standard_normal((128, 256))
    t[:, 128:] *= 0.01
    a = t.copy()
    a[:, 200] *= 1.01
    assert rel_err(a, t) < 1e-4 and 3e-4 < bt.slice_err(a, t) <= 1e-3 * 1.01
    z = np.zeros(256)
    z[:128] = rng.standard_normal(128)
    b = z.copy()
    b[200] = 1e-3 * np.abs(z).max()                                  # an exact-zero entry stays in the check
    assert bt.slice_err(b, z) == pytest.approx(1e-2)
    assert bt.slice_err(z, z) == 0.0 and bt.slice_err(np.float64(2.0), np.float64(1.0)) == 1.0


# ---- the launch order of the global-average block --------------------------------------------------------------------------------
_HELPER_PREFIXES, _HELPER_SUFFIXES = ("new_", "take_", "note_", "clear_", "has_"), ("_supported", "_wanted", "_blocks")


def _record_launchers(monkeypatch, ck):
    """Every launcher of surfacenetworks_amd.kernels appends its name to the returned list when the product calls it.  The seam
    has no twin of the merged launches (bn_fold_seg, avg_bn_bwd) nor of the tile-sum statistics, and says so through its
    predicates; here the predicates answer as the device's do and the four launchers are composed from the twins they merge."""
    import types

    from surfacenetworks_amd import kernels

    def bn_fold_seg(stats, rows, gamma, beta, W, b, eps, momentum, running_mean, running_var, m, num_batches_tracked=None):
        r = ck.bn_fold(stats, rows, gamma, beta, W, b, eps, momentum, True, running_mean, running_var, num_batches_tracked)
        return (*r, ck.seg_affine(m, r[4][:, m.shape[1]:], r[5]))

    def avg_bn_bwd(G1, dystats, seg_dy, m, mu2, W, s, invstd, beta, rows, has_bias, Wf2, inv_count, rows_per_seg=0, segoff=None):
        C = G1.shape[1]
        dW, db, dg, dbeta, Bc, Cc = ck.bn_bwd_coeffs(ck.avg_bwd_gc(G1, seg_dy, m, mu2), dystats, W, s, invstd, beta, rows, has_bias)
        per = rows_per_seg if segoff is None else (segoff[1:] - segoff[:-1]).double().reshape(-1, 1)
        v = seg_dy.double() @ Wf2.double() + per * ((m.double() - mu2.double()) * Bc[C:].double() + Cc[C:].double())
        return dW, db, dg, dbeta, Bc, Cc, (v * inv_count.double().reshape(-1, 1)).float()

    def avg_stats_from_tiles(tile_sums, part, e, mask, inv_count, rows_per_seg, nseg):
        return ck.avg_stats(e, mask, inv_count, rows_per_seg, nseg)

    def avg_stats_from_tiles_ragged(tile_sums, part, e, seg):
        m = ck.segment_colsum_ragged(e, seg.tiles, seg.seg_tile_ptr, seg.nseg, seg.inv_count)
        return m, ck.avg_stats_ragged(m, seg, ck.colstats(e).reshape(1, 2, -1), 1)

    def avg_merged_supported(J, C, nseg, which=1):
        return 0 < nseg <= (64 if which == 1 else kernels.AVG_BWD_MERGE_MAX)

    for fn in (bn_fold_seg, avg_bn_bwd, avg_stats_from_tiles, avg_stats_from_tiles_ragged, avg_merged_supported):
        monkeypatch.setattr(kernels, fn.__name__, fn)
    monkeypatch.setattr(kernels, "tile_sums_supported", lambda: True)
    monkeypatch.setattr(kernels, "new_tile_sums", lambda rows, device: torch.zeros(((rows + 31) // 32, 128)))
    calls = []

    def wrap(name, fn):
        def launcher(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return launcher

    for name, fn in list(vars(kernels).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith(("_",) + _HELPER_PREFIXES) and not name.endswith(_HELPER_SUFFIXES):
            monkeypatch.setattr(kernels, name, wrap(name, fn))
    return calls


# One AvgResNet2 forward + backward at C = 128 as the commit before the padded and the packed batch shared one code path launched
# it, written down from runs of that commit.  The lists differ in three places only, so they are kept as those places:
# the statistics of the two stage operands, by batch layout and by what the producer of the input left on its activated hand-off;
_AVG_STATS = {
    ("padded", "none"): (("elu_into", "avg_stats"), ("avg_stats",)),
    ("padded", "partials"): (("avg_stats",), ("avg_stats",)),
    ("padded", "tiles"): (("avg_stats_from_tiles",), ("avg_stats_from_tiles",)),
    ("packed", "none"): (("elu_into", "segment_colsum_ragged", "colstats", "avg_stats_ragged"), ("segment_colsum_ragged", "avg_stats_ragged")),
    ("packed", "partials"): (("segment_colsum_ragged", "avg_stats_ragged"), ("segment_colsum_ragged", "avg_stats_ragged")),
    ("packed", "tiles"): (("avg_stats_from_tiles_ragged",), ("avg_stats_from_tiles_ragged",)),
}
# the fold and the GEMM of a stage, by whether the per-mesh bias is folded in the same launch (up to 64 meshes);
_AVG_FOLD = {True: ("bn_fold_seg",), False: ("bn_fold", "seg_affine")}
_AVG_GEMM = {"padded": ("linear_fwd_segbias",), "packed": ("linear_fwd_segbias_ragged",)}
# and the backward of a stage, by whether its middle trio is one launch (up to kernels.AVG_BWD_MERGE_MAX meshes).
_AVG_BWD = {
    ("padded", True): ("wgrad_seg", "avg_bn_bwd", "linear_dgrad_eluseg"),
    ("padded", False): ("wgrad_seg", "avg_bwd_gc", "bn_bwd_coeffs", "avg_bwd_segvec", "linear_dgrad_eluseg"),
    ("packed", True): ("wgrad_slabs", "avg_bn_bwd", "linear_dgrad_eluseg_ragged"),
    ("packed", False): ("wgrad_slabs", "avg_bwd_gc", "bn_bwd_coeffs", "avg_bwd_segvec_ragged", "linear_dgrad_eluseg_ragged"),
}
# The per-stage functions (full width: the broadcast mean is written) launch the same at every mesh count.
_AVG_PER_STAGE = {
    "padded": (("elu_into", "segment_colsum", "bcast_rows", "colstats", "bn_fold", "linear_fwd"),
               ("wgrad", "bn_bwd_coeffs", "linear_dgrad", "segment_colsum", "elu_bwd_bcast")),
    "packed": (("elu_into", "segment_colsum_ragged", "bcast_rows_ragged", "colstats", "bn_fold", "linear_fwd"),
               ("wgrad", "bn_bwd_coeffs", "linear_dgrad", "segment_colsum_ragged", "bcast_rows_ragged", "elu_bwd")),
}


def _avg_launches(layout, producer, fwd_merged, bwd_merged):
    if producer == "per-stage":
        fwd, bwd = _AVG_PER_STAGE[layout]
        return fwd * 2 + ("backward",) + bwd * 2
    s0, s1 = _AVG_STATS[(layout, producer)]
    stage = _AVG_FOLD[fwd_merged] + _AVG_GEMM[layout]
    return s0 + stage + s1 + stage + ("backward",) + _AVG_BWD[(layout, bwd_merged)] * 2


_AVG_MESHES = {9: (True, True), 33: (True, False), 65: (False, False)}       # meshes: (forward merged, backward merged)


@pytest.mark.parametrize("meshes", list(_AVG_MESHES))
@pytest.mark.parametrize("producer", ["none", "partials", "tiles", "per-stage"])
@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_average_block_launches_what_it_always_launched(layout, producer, meshes, cpu_kernels, monkeypatch):
    """No pass added, none lost, same order: the ordered list of kernels.* launchers of one AvgResNet2 forward + backward, both
    batch layouts; without a producer (an ELU pass, no statistics partials), with a producer's partials, with its tile sums too
    (blocks._TILE_SUMS_MIN_ROWS lowered: the block's own first GEMM then leaves them for its second stage), and through the
    per-stage functions; 9, 33 and 65 meshes of 32 to 45 rows — both sides of the forward limit (64) and of the backward one."""
    import numpy as np

    import surfacenetworks_amd.utils_pt as U
    from helpers import deterministic_init
    from surfacenetworks_amd import blocks, kernels
    from surfacenetworks_amd.operators import PackedSegments

    assert kernels.AVG_BWD_MERGE_MAX == 32
    C = 128
    lengths = np.resize([35, 42, 36, 32, 45], meshes)
    if layout == "packed":
        mask, shape = PackedSegments(lengths, "cpu"), (1, int(lengths.sum()), C)
    else:
        mask = torch.from_numpy((np.arange(45)[None, :, None] < lengths[:, None, None]).astype(np.float32))
        shape = (meshes, 45, C)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(meshes)).requires_grad_(True)
    blk = deterministic_init(U.AvgResNet2(C), 3).train()
    if producer == "per-stage":
        monkeypatch.setattr(U, "USE_WHOLE_BLOCKS", False)
        monkeypatch.setattr(blocks, "avg_block_ok", lambda *a: False)           # (a packed batch asks only this)
    elif producer != "none":
        rows = shape[0] * shape[1]
        cat = torch.empty(rows, 2 * C)
        cat[:, :C] = torch.nn.functional.elu(x.detach().reshape(rows, C))
        cat._sn_part = cpu_kernels.colstats(cat[:, :C]).reshape(1, 2, C)
        if producer == "tiles":
            monkeypatch.setattr(blocks, "_TILE_SUMS_MIN_ROWS", 0)
            cat._sn_tiles = torch.zeros(((rows + 31) // 32, C))
        blocks.attach_activated(x, cat)
    calls = _record_launchers(monkeypatch, cpu_kernels)
    y = blk(None, mask, x)
    calls.append("backward")
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert tuple(calls) == _avg_launches(layout, producer, *_AVG_MESHES[meshes])
