"""block_truth.py on the CPU: the product's host logic (autograd nodes, hand-offs, per-stage functions) on the oracle-backed
kernels of the `cpu_kernels` seam, held to the float64 blocks tensor by tensor with the same helper, truth, metrics and
conditioning asserts as tests/test_block_truth_gpu.py.

Forms run here: whole-block nodes and per-stage functions of chains (a) to (e) at C = 128 and 64 on the 11-mesh batch, in train
and eval mode, f=None and torch.zeros, f_out_needed False and True, avg_next given and not said; the global-average block on the
33-mesh, the padded ragged and the packed batch.
GPU only (the seam has no such kernel or refuses the switch): the storage forms (q3 / bsr4 / csr, rb4 / ring: the host twins
share one arithmetic), blocks.DEFER_FACE_TAIL (a raw face gradient needs the device GEMM), launch plans, the tile-sum
hand-offs (kernels.tile_sums_supported() is False here) and the merged / separate launches of the averaging backward."""
import pytest

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
