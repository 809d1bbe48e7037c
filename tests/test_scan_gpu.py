"""The library's one exclusive scan (sn_kernels.hip, reached by the mesh builders and the sparse product as
sn_internal_scan_i32) at the sizes where it changes path, through two entry points that end in it:

* sn_mesh_compact_i32 scans nF + 1 and nV + 1 marks.  A tile is 2048 items and the pass over the tile sums takes 256 of them per
  round: item counts of 2048 (one full tile), 2049 (a second tile of one item) and 256 * 2048 + 1 (a 257th tile, so the carry of
  the first round is used).  Exact against mesh_ops.compact.
* phase 0 of sn_csr_spgemm_f32 scans the structural row counts; the tile sums are added in int64 and a total past INT_MAX is
  refused (SN_SPGEMM_TOO_LARGE) with the row pointers untouched.  Rows of 131072 entries — the widest the kernels take, see
  test_amplify_gpu.test_row_wider_than_the_window_is_refused_and_nothing_is_written — put the total on either side of 2^31 with
  16385 and 16383 rows.  Only the count phase runs: nothing of that size is allocated."""
import ctypes

import numpy as np
import pytest
import torch

from surfacenetworks_amd import _lib, kernels, mesh_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("nV,nF", [(2047, 2047), (2048, 2048), (2047, 2048), (2048, 2047), (2048, 256 * 2048)])
def test_compact_at_the_scan_boundaries(nV, nF):
    f = np.arange(nF, dtype=np.int64)
    F = (np.stack([f, f + 1, f + 2], axis=1) % nV).astype(np.int32)
    keep = np.random.default_rng(2048).integers(0, 2, nF).astype(np.int32)
    want = mesh_ops.compact(None, F, keep, nV)
    got = kernels.mesh_compact(torch.from_numpy(F).to(DEV), torch.from_numpy(keep).to(DEV), nV)
    nVk, nFk = got.sizes.cpu().tolist()
    assert [nVk, nFk] == want.sizes.tolist() and 0 < nFk < nF
    assert np.array_equal(got.I.cpu().numpy(), want.I)
    assert np.array_equal(got.J.cpu().numpy()[:nVk], want.J)
    assert np.array_equal(got.Fsrc.cpu().numpy()[:nFk], want.Fsrc)
    assert np.array_equal(got.Fnew.cpu().numpy()[:nFk], want.Fnew)


@pytest.mark.parametrize("M,refused", [(16385, True), (16383, False)])
def test_spgemm_count_total_on_either_side_of_int32(M, refused):
    W = kernels.spgemm_max_window()
    assert W == 131072
    total = M * W
    assert (total > 2**31 - 1) == refused and abs(total - 2**31) <= W
    t = lambda a: torch.from_numpy(a).to(DEV)
    a_rp, a_ci, a_v = t(np.arange(M + 1, dtype=np.int32)), t(np.zeros(M, np.int32)), t(np.ones(M, np.float32))      # A: M x 1
    b_rp, b_ci, b_v = t(np.array([0, W], np.int32)), t(np.arange(W, dtype=np.int32)), t(np.ones(W, np.float32))     # B: 1 x W, full
    s_rowptr = torch.full((M + 1,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws_bytes = int(_lib.load().sn_csr_spgemm_workspace_bytes(M))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    _lib.call("sn_csr_spgemm_f32", p(a_rp), p(a_ci), p(a_v), p(b_rp), p(b_ci), p(b_v), M, 1, W, 0, p(s_rowptr), None, None, None,
              None, None, p(status), p(ws), ws_bytes, kernels._stream())
    if refused:
        assert int(status.item()) == kernels.SPGEMM_TOO_LARGE
        assert bool((s_rowptr == -7).all())
    else:
        assert int(status.item()) == 0
        assert int(s_rowptr[M].item()) == total == 2147352576
        assert torch.equal(s_rowptr.long(), torch.arange(M + 1, device=DEV) * W)
