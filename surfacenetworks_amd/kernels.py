"""Tensor-level launchers of the C-ABI (include/sn_spmm.h).  PyTorch is plumbing here: it owns the HBM
allocations and the HIP stream; every byte of the hot path is moved by the kernels in csrc/sn_kernels.hip.

All functions require device ("cuda" = HIP under PyTorch-ROCm) tensors and raise otherwise — there is no
CPU path in the product.  Launches go to torch's current stream and never synchronise, except
csr_to_bsr4 which must read one integer (the block count) back to size its outputs.
"""
from __future__ import annotations

import collections

import torch

from . import _lib, constants
# the status bits and limits of include/sn_spmm.h, kept once in constants.py and exposed here under the same names
from .constants import *  # noqa: F401,F403

__all__ = [
    "note_absmax", "take_absmax", "absmax_wanted", "clear_absmax", "tile_sums_supported", "new_tile_sums", "avg_stats_from_tiles", "spmm_csr", "spmm_bsr4", "spmm_csr_elubwd", "spmm_bsr4_elubwd", "spmm_q3", "spmm_q3_stats", "spmm_q3_stats_supported", "spmm_csr_stats", "spmm_csr_stats_supported", "csr_to_rb4", "spmm_rb4", "spmm_rb4_stats", "spmm_rb4_supported", "spmm_ring", "spmm_ring_stats", "spmm_ring_supported", "ring_half_window", "csr_band", "bsr4_to_q3", "coo_to_csr", "csr_transpose", "csr_to_bsr4", "blockdiag_concat", "blockdiag_concat_ragged", "validate_csr",
    "elu_into", "elu_bwd", "colstats", "wgrad", "wgrad_supported", "affine_cols_acc", "affine_cols_elu_bwd",
    "bn_fold", "bn_bwd_coeffs", "segment_colsum", "bcast_rows", "segment_colsum_ragged", "bcast_rows_ragged", "elu_bwd_bcast", "dirac_from_mesh", "laplacian_from_mesh", "linear_fwd", "linear_fwd_supported", "linear_dgrad",
    "linear_dgrad_supported", "linear_dgrad_elu", "linear_dgrad_elu_supported",
    "avg_stage_supported", "avg_fwd_prep", "avg_stats", "seg_affine", "avg_bwd_gc", "avg_bwd_segvec", "linear_fwd_segbias", "linear_dgrad_eluseg", "wgrad_seg", "wgrad_slabs", "avg_bwd_segvec_ragged", "linear_fwd_segbias_ragged", "linear_dgrad_eluseg_ragged", "avg_stage_ragged_supported", "wgrad_thin", "wgrad_thin_supported", "linear_thin_fwd", "masked_smooth_l1_fwd", "masked_smooth_l1_bwd", "gather_segments", "pair_argmin", "pair_ce_fwd", "pair_ce_bwd", "pair_fused_fwd", "pair_fused_bwd", "colstats_partial", "linear_fwd_stats_blocks", "elu_stats_supported", "new_elu_stats_part", "colstats_halves", "colstats_into", "colstats_from_part", "colstats_merge_into",
    "avg_merged_supported", "avg_stats_ragged", "avg_stats_from_tiles_ragged", "gather_segments_ragged",
]
# (the list above is also what the tests' host twin of this module replaces, name by name.  Launchers that have no host twin —
#  normal_cosine_*: normal_predict computes CPU tensors with its plain-torch reference functions — stay off it.)


def _dev(*tensors) -> None:
    if _lib._recorder is not None and _lib.recorder() is not None and _lib._recorder.allow_cpu:
        return                                # (tests record — never run — launch plans on CPU tensors)
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "surfacenetworks_amd kernels run on the MI355X only: got a CPU tensor. There is no CPU/eager "
                "fallback in this package (the reference's CPU torch.sparse path lives in oracle/ for tests).")


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _workspace(query: str, device, *dims, least: int = 16):
    """(uint8 tensor of max(bytes, least) bytes on `device`, bytes): the scratch buffer of an entry point, sized by its
    sn_*_workspace_bytes query.  Allocated where it is called, so a wrapper's allocations keep their order."""
    nbytes = int(getattr(_lib.load(), query)(*dims))
    return torch.empty(max(nbytes, least), dtype=torch.uint8, device=device), nbytes


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  Through the two C entry points behind
    torch.cuda.current_stream() when this torch has them: the Stream-object route costs ~8 us per call on the host, as
    much as everything else around a launch."""
    if _lib._recorder is not None and _lib.recorder() is not None:      # a launch plan is being recorded: the stream is an
        return 0                                                         # argument of sn_plan_run
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _ld(t: torch.Tensor) -> int:
    """Leading dimension of a 2-D view whose rows are contiguous."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"expected a 2-D tensor with unit column stride, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _check_dense(x: torch.Tensor, rows: int, group: int, N: int, what: str) -> int:
    if x.dtype != torch.float32:
        raise TypeError(f"{what} must be float32")
    if rows % group or x.shape[0] != rows // group or x.shape[1] != group * N:
        raise ValueError(f"{what}: expected ({rows // group}, {group * N}) for {rows} operator rows in groups of {group}, got {tuple(x.shape)}")
    return _ld(x)


def spmm_csr(rowptr, colind, vals, M: int, K: int, x, y, group: int = 1) -> None:
    """y <- A·x.  x: (K/group, group*N) and y: (M/group, group*N) 2-D views with contiguous rows
    (any row stride), e.g. halves of a (rows, 2C) concat buffer.  group=4 is the quaternion view."""
    _dev(rowptr, colind, vals, x, y)
    N = y.shape[1] // group
    ldx = _check_dense(x, K, group, N, "x")
    ldy = _check_dense(y, M, group, N, "y")
    _lib.call("sn_spmm_csr_f32", _p(rowptr), _p(colind), _p(vals), M, K, int(colind.numel()),
              _p(x), ldx, group, N, _p(y), ldy, group, _stream())


def spmm_csr_stats_supported(N: int, group: int) -> bool:
    return N == 128 and group == 1


def spmm_csr_stats(rowptr, colind, vals, M: int, K: int, x, y):
    """y <- A·x as spmm_csr (N = 128, plain row-major operands) and the partial column statistics of y: returns the
    (blocks, 2, 128) float64 partials that colstats_halves merges (sn_spmm_csr_stats_f32)."""
    _dev(rowptr, colind, vals, x, y)
    N = y.shape[1]
    if not spmm_csr_stats_supported(N, 1):
        raise ValueError("spmm_csr_stats: 128-column operands only")
    ldx = _check_dense(x, K, 1, N, "x")
    ldy = _check_dense(y, M, 1, N, "y")
    lib = _lib.load()
    part = torch.empty((int(lib.sn_spmm_q3_stats_blocks()), 2, 128), dtype=torch.float64, device=y.device)
    ws, ws_bytes = _workspace("sn_spmm_csr_stats_workspace_bytes", y.device, M)
    _lib.call("sn_spmm_csr_stats_f32", _p(rowptr), _p(colind), _p(vals), M, K, int(colind.numel()), _p(x), ldx, 1, N, _p(y), ldy, 1,
              _p(part), _p(ws), ws_bytes, _stream())
    return part


def csr_to_rb4(rowptr, colind, vals, M: int, K: int):
    """CSR -> RB4 (4x1 row blocks): (b_ptr [ceil(M/4)+1], b_col [nnz], b_val [nnz, 4]).  No synchronisation: the arrays are
    sized by nnz, an upper bound of the listed-column total (the tail past b_ptr[-1] is never read)."""
    _dev(rowptr, colind, vals)
    dev = rowptr.device
    Mb = (M + 3) // 4
    nnz = int(colind.numel())
    b_ptr = torch.empty(Mb + 1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_scan_workspace_bytes", dev, Mb + 1)
    _lib.call("sn_rb4_count", _p(rowptr), _p(colind), M, K, _p(b_ptr), _p(ws), ws_bytes, _stream())
    b_col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
    b_val = torch.empty((max(nnz, 1), 4), dtype=torch.float32, device=dev)[:nnz]
    if nnz:
        _lib.call("sn_rb4_fill", _p(rowptr), _p(colind), _p(vals), M, K, _p(b_ptr), _p(b_col), _p(b_val), _stream())
    return b_ptr, b_col, b_val


def spmm_rb4_supported(N: int, group: int) -> bool:
    return group == 1 and N in (64, 128)


def spmm_rb4(b_ptr, b_col, b_val, M: int, K: int, x, y, e=None, g=None, want_absmax: bool = False):
    """y <- A·x for an RB4 operator (sn_spmm_rb4_f32); with e: (A·x) * elu'(e) + g (sn_spmm_rb4_elubwd_f32).
    want_absmax (with e): also returns the per-wave maxima of |y| (sn_spmm_rb4_elubwd_absmax_f32), else None."""
    _dev(b_ptr, b_col, b_val, x, y, e, g)
    N = y.shape[1]
    ldx = _check_dense(x, K, 1, N, "x")
    ldy = _check_dense(y, M, 1, N, "y")
    cap = int(b_col.numel())
    if e is None:
        _lib.call("sn_spmm_rb4_f32", _p(b_ptr), _p(b_col), _p(b_val), M, K, cap, _p(x), ldx, N, _p(y), ldy, _stream())
    else:
        lde = _check_dense(e, M, 1, N, "e")
        ldg = _check_dense(g, M, 1, N, "g") if g is not None else 0
        if want_absmax and M > 0:
            am = torch.empty(int(_lib.load().sn_spmm_rb4_absmax_blocks(M, N)), dtype=torch.float32, device=y.device)
            _lib.call("sn_spmm_rb4_elubwd_absmax_f32", _p(b_ptr), _p(b_col), _p(b_val), M, K, cap, _p(x), ldx, N, _p(e), lde, _p(g),
                      ldg, _p(y), ldy, _p(am), _stream())
            return am
        _lib.call("sn_spmm_rb4_elubwd_f32", _p(b_ptr), _p(b_col), _p(b_val), M, K, cap, _p(x), ldx, N, _p(e), lde, _p(g), ldg,
                  _p(y), ldy, _stream())
    return None


def spmm_rb4_stats(b_ptr, b_col, b_val, M: int, K: int, x, y):
    """spmm_rb4 (N = 128) that also returns the (blocks, 2, 128) float64 partial column statistics of y."""
    _dev(b_ptr, b_col, b_val, x, y)
    N = y.shape[1]
    if N != 128:
        raise ValueError("spmm_rb4_stats: 128-column operands only")
    ldx = _check_dense(x, K, 1, N, "x")
    ldy = _check_dense(y, M, 1, N, "y")
    lib = _lib.load()
    part = torch.empty((int(lib.sn_spmm_q3_stats_blocks()), 2, 128), dtype=torch.float64, device=y.device)
    ws, ws_bytes = _workspace("sn_spmm_rb4_stats_workspace_bytes", y.device, M)
    _lib.call("sn_spmm_rb4_stats_f32", _p(b_ptr), _p(b_col), _p(b_val), M, K, int(b_col.numel()), _p(x), ldx, N, _p(y), ldy,
              _p(part), _p(ws), ws_bytes, _stream())
    return part


# Rows below which the ring kernel's persistent strips are mostly prologue (one workgroup per CU, >= 8 steps of 64 rows each)
RING_MIN_ROWS = 131072
# Largest share of rows with an entry outside the window (they gather from global memory inside the kernel: closed meshes'
# wrap-around rows) for which the ring kernel is still the faster one (a 65 x 106 torus batch has 3 %: 0.67-0.83 of the
# roofline against the row-blocked kernel's 0.59-0.69)
RING_MAX_OUTSIDE = 0.05


def spmm_ring_supported(N: int, group: int, M: int, K: int) -> bool:
    from . import kernels as _self      # (RING_MIN_ROWS is read through the module so that tests / tools can lower it)

    return group == 1 and N in (64, 128) and M == K and M >= _self.RING_MIN_ROWS


def ring_half_window() -> int:
    return int(_lib.load().sn_spmm_csr_ring_half_window())


def csr_band(rowptr, colind, M: int, K: int):
    """(max |column - row|, longest row, rows with an entry outside the ring kernel's window) of a CSR operator — reads
    three ints back from the device (once per operator)."""
    _dev(rowptr, colind)
    out = torch.empty(3, dtype=torch.int32, device=rowptr.device)
    _lib.call("sn_csr_band_i32", _p(rowptr), _p(colind), M, K, _p(out), _stream())
    band, longest, outside = out.tolist()
    return int(band), int(longest), int(outside)


def spmm_ring(rowptr, colind, vals, M: int, K: int, x, y, e=None, g=None, want_absmax: bool = False):
    """y <- A·x for a banded square CSR operator through the sliding-window kernel (sn_spmm_csr_ring_f32); with e:
    (A·x) * elu'(e) + g (sn_spmm_csr_ring_elubwd_f32).  Bit-identical to spmm_csr.
    want_absmax (with e): also returns the per-wave maxima of |y| (sn_spmm_csr_ring_elubwd_absmax_f32), else None."""
    _dev(rowptr, colind, vals, x, y, e, g)
    N = y.shape[1]
    ldx = _check_dense(x, K, 1, N, "x")
    ldy = _check_dense(y, M, 1, N, "y")
    nnz = int(colind.numel())
    if e is None:
        _lib.call("sn_spmm_csr_ring_f32", _p(rowptr), _p(colind), _p(vals), M, K, nnz, _p(x), ldx, N, _p(y), ldy, _stream())
    else:
        lde = _check_dense(e, M, 1, N, "e")
        ldg = _check_dense(g, M, 1, N, "g") if g is not None else 0
        if want_absmax and M > 0 and nnz > 0:
            am = torch.empty(int(_lib.load().sn_spmm_csr_ring_absmax_blocks(M, N)), dtype=torch.float32, device=y.device)
            _lib.call("sn_spmm_csr_ring_elubwd_absmax_f32", _p(rowptr), _p(colind), _p(vals), M, K, nnz, _p(x), ldx, N, _p(e), lde,
                      _p(g), ldg, _p(y), ldy, _p(am), _stream())
            return am
        _lib.call("sn_spmm_csr_ring_elubwd_f32", _p(rowptr), _p(colind), _p(vals), M, K, nnz, _p(x), ldx, N, _p(e), lde, _p(g), ldg,
                  _p(y), ldy, _stream())
    return None


def spmm_ring_stats(rowptr, colind, vals, M: int, K: int, x, y):
    """spmm_ring (N = 128) that also returns the (blocks, 2, 128) float64 partial column statistics of y."""
    _dev(rowptr, colind, vals, x, y)
    N = y.shape[1]
    if N != 128:
        raise ValueError("spmm_ring_stats: 128-column operands only")
    ldx = _check_dense(x, K, 1, N, "x")
    ldy = _check_dense(y, M, 1, N, "y")
    lib = _lib.load()
    part = torch.empty((int(lib.sn_spmm_q3_stats_blocks()), 2, 128), dtype=torch.float64, device=y.device)
    ws, ws_bytes = _workspace("sn_spmm_csr_ring_stats_workspace_bytes", y.device, M)
    _lib.call("sn_spmm_csr_ring_stats_f32", _p(rowptr), _p(colind), _p(vals), M, K, int(colind.numel()), _p(x), ldx, N, _p(y), ldy,
              _p(part), _p(ws), ws_bytes, _stream())
    return part


def spmm_bsr4(b_rowptr, b_colind, b_vals, Mb: int, Kb: int, x, y, group: int = 1) -> None:
    _dev(b_rowptr, b_colind, b_vals, x, y)
    N = y.shape[1] // group
    ldx = _check_dense(x, 4 * Kb, group, N, "x")
    ldy = _check_dense(y, 4 * Mb, group, N, "y")
    _lib.call("sn_spmm_bsr4_f32", _p(b_rowptr), _p(b_colind), _p(b_vals), Mb, Kb, int(b_colind.numel()),
              _p(x), ldx, group, N, _p(y), ldy, group, _stream())


def spmm_csr_elubwd(rowptr, colind, vals, M: int, K: int, x, e, g, y, group: int = 1) -> None:
    """y <- (A·x) * elu'(e) + g with elu' taken from the activation output e (sn_spmm_csr_elubwd_f32); g may be None."""
    _dev(rowptr, colind, vals, x, e, g, y)
    N = y.shape[1] // group
    ldx = _check_dense(x, K, group, N, "x")
    ldy = _check_dense(y, M, group, N, "y")
    lde = _check_dense(e, M, group, N, "e")
    ldg = _check_dense(g, M, group, N, "g") if g is not None else 0
    _lib.call("sn_spmm_csr_elubwd_f32", _p(rowptr), _p(colind), _p(vals), M, K, int(colind.numel()),
              _p(x), ldx, group, N, _p(e), lde, _p(g), ldg, _p(y), ldy, group, _stream())


def spmm_bsr4_elubwd(b_rowptr, b_colind, b_vals, Mb: int, Kb: int, x, e, g, y, group: int = 1) -> None:
    _dev(b_rowptr, b_colind, b_vals, x, e, g, y)
    N = y.shape[1] // group
    ldx = _check_dense(x, 4 * Kb, group, N, "x")
    ldy = _check_dense(y, 4 * Mb, group, N, "y")
    lde = _check_dense(e, 4 * Mb, group, N, "e")
    ldg = _check_dense(g, 4 * Mb, group, N, "g") if g is not None else 0
    _lib.call("sn_spmm_bsr4_elubwd_f32", _p(b_rowptr), _p(b_colind), _p(b_vals), Mb, Kb, int(b_colind.numel()),
              _p(x), ldx, group, N, _p(e), lde, _p(g), ldg, _p(y), ldy, group, _stream())


def spmm_q3_tail_supported(N: int, group: int) -> bool:
    """Whether the quaternion-packed product finishes a raw gradient in its store (spmm_q3(tail=...))."""
    return bool(_lib.load().sn_spmm_q3_tail_supported(int(N), int(group)))


def elu_tail_finish(g, e, tail) -> None:
    """g <- the finished input gradient, in place, from the raw one linear_dgrad_elu_raw left (sn_elu_tail_finish_f32): for the
    products whose store cannot do it.  tail = (center, B, Cc), one value per column of g."""
    center, B, Cc = tail
    _dev(g, e, center, B, Cc)
    rows, C = g.shape
    if e.shape != g.shape or any(t.shape != (C,) or not t.is_contiguous() for t in tail):
        raise ValueError(f"elu_tail_finish: g {tuple(g.shape)}, e {tuple(e.shape)} and tail vectors of {C} do not match")
    _lib.call("sn_elu_tail_finish_f32", _p(g), _ld(g), _p(e), _ld(e), _p(center), _p(B), _p(Cc), rows, C, _stream())


def spmm_q3(b_rowptr, q_blk, Mb: int, Kb: int, x, y, group: int = 1, e=None, g=None, want_absmax: bool = False, tail=None):
    """y <- A·x for a quaternion-packed Dirac operator (sn_spmm_q3_f32); with e: (A·x) * elu'(e) + g (sn_spmm_q3_elubwd_f32).
    want_absmax (with e): also returns the per-workgroup maxima of |y| (sn_spmm_q3_elubwd_absmax_f32), else None.
    tail = (center, B, Cc): g is a raw gradient that the store finishes (sn_spmm_q3_elubwd_tail_absmax_f32; the caller has
    asked spmm_q3_tail_supported)."""
    _dev(b_rowptr, q_blk, x, y, e, g)
    N = y.shape[1] // group
    ldx = _check_dense(x, 4 * Kb, group, N, "x")
    ldy = _check_dense(y, 4 * Mb, group, N, "y")
    nblk = int(q_blk.shape[0])
    if e is None:
        _lib.call("sn_spmm_q3_f32", _p(b_rowptr), _p(q_blk), Mb, Kb, nblk, _p(x), ldx, group, N, _p(y), ldy, group, _stream())
    else:
        lde = _check_dense(e, 4 * Mb, group, N, "e")
        ldg = _check_dense(g, 4 * Mb, group, N, "g") if g is not None else 0
        if tail is not None:
            center, B, Cc = tail
            _dev(center, B, Cc)
            if g is None or any(t.shape != (group * N,) or not t.is_contiguous() for t in tail):
                raise ValueError("spmm_q3: a tail needs the raw gradient g and three contiguous vectors of one value per channel")
            am = None
            if want_absmax and Mb > 0:
                am = torch.empty(int(_lib.load().sn_spmm_q3_absmax_blocks(Mb, N)), dtype=torch.float32, device=y.device)
            _lib.call("sn_spmm_q3_elubwd_tail_absmax_f32", _p(b_rowptr), _p(q_blk), Mb, Kb, nblk, _p(x), ldx, group, N, _p(e), lde,
                      _p(g), ldg, _p(center), _p(B), _p(Cc), _p(y), ldy, group, _p(am), _stream())
            return am
        if want_absmax and Mb > 0:
            am = torch.empty(int(_lib.load().sn_spmm_q3_absmax_blocks(Mb, N)), dtype=torch.float32, device=y.device)
            _lib.call("sn_spmm_q3_elubwd_absmax_f32", _p(b_rowptr), _p(q_blk), Mb, Kb, nblk, _p(x), ldx, group, N, _p(e), lde, _p(g),
                      ldg, _p(y), ldy, group, _p(am), _stream())
            return am
        _lib.call("sn_spmm_q3_elubwd_f32", _p(b_rowptr), _p(q_blk), Mb, Kb, nblk, _p(x), ldx, group, N, _p(e), lde, _p(g), ldg,
                  _p(y), ldy, group, _stream())
    return None


def spmm_q3_stats_supported(N: int, group: int) -> bool:
    return N in (16, 32) and group == 4


def spmm_q3_stats(b_rowptr, q_blk, Mb: int, Kb: int, x, y, group: int = 4):
    """y <- A·x as spmm_q3, and the partial column statistics of y viewed as (Mb, 128): returns the (blocks, 2, 128) float64
    partials that colstats_halves / colstats_from_part-style merges combine (sn_spmm_q3_stats_f32)."""
    _dev(b_rowptr, q_blk, x, y)
    N = y.shape[1] // group
    if not spmm_q3_stats_supported(N, group):
        raise ValueError("spmm_q3_stats: 128- or 64-channel operands in the group-4 layout only")
    ldx = _check_dense(x, 4 * Kb, group, N, "x")
    ldy = _check_dense(y, 4 * Mb, group, N, "y")
    lib = _lib.load()
    part = torch.empty((int(lib.sn_spmm_q3_stats_blocks()), 2, 4 * N), dtype=torch.float64, device=y.device)
    ws, ws_bytes = _workspace("sn_spmm_q3_stats_workspace_bytes", y.device, Mb)
    _lib.call("sn_spmm_q3_stats_f32", _p(b_rowptr), _p(q_blk), Mb, Kb, int(q_blk.shape[0]), _p(x), ldx, group, N, _p(y), ldy,
              group, _p(part), _p(ws), ws_bytes, _stream())
    return part


def bsr4_to_q3(b_colind, b_vals):
    """(q_blk (nblocks, 4) fp32 with the block column in the 4th word's bits, flag (1,) int32 device tensor: 1 if some block
    is not a pure-quaternion matrix) — sn_bsr4_to_q3_f32.  The flag is left on the device: the caller decides when to read it."""
    _dev(b_colind, b_vals)
    nblk = int(b_colind.numel())
    q = torch.empty((nblk, 4), dtype=torch.float32, device=b_colind.device)
    flag = torch.empty(1, dtype=torch.int32, device=b_colind.device)
    _lib.call("sn_bsr4_to_q3_f32", _p(b_colind), _p(b_vals), nblk, _p(q), _p(flag), _stream())
    return q, flag


def coo_to_csr(idx_batch, idx_row, idx_col, B: int, R: int, Kb: int):
    """Sorted int64 COO index rows -> (rowptr int32 [B*R+1], colind int32 [nnz]) of the block-diagonal operator."""
    _dev(idx_batch, idx_row, idx_col)
    nnz = int(idx_row.numel())
    dev = idx_row.device
    rowptr = torch.empty(B * R + 1, dtype=torch.int32, device=dev)
    colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    ib = None if idx_batch is None else idx_batch.contiguous()
    _lib.call("sn_coo_to_csr_i32", _p(ib), _p(idx_row.contiguous()), _p(idx_col.contiguous()), nnz, B, R, Kb,
              _p(rowptr), _p(colind), _stream())
    return rowptr, colind


def csr_transpose(rowptr, colind, vals, M: int, K: int):
    _dev(rowptr, colind, vals)
    nnz = int(colind.numel())
    dev = rowptr.device
    t_rowptr = torch.empty(K + 1, dtype=torch.int32, device=dev)
    t_colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    t_vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace("sn_csr_transpose_workspace_bytes", dev, M, K, nnz)
    _lib.call("sn_csr_transpose_f32", _p(rowptr), _p(colind), _p(vals), M, K, nnz, _p(t_rowptr), _p(t_colind),
              _p(t_vals), _p(ws), ws_bytes, _stream())
    return t_rowptr, t_colind, t_vals


def csr_to_bsr4(rowptr, colind, vals, M: int, K: int):
    """CSR -> 4x4-block BSR.  Synchronises once (reads the block count)."""
    _dev(rowptr, colind, vals)
    if M % 4 or K % 4:
        raise ValueError("BSR4 needs M and K to be multiples of 4")
    dev = rowptr.device
    Mb = M // 4
    b_rowptr = torch.empty(Mb + 1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_scan_workspace_bytes", dev, Mb + 1)
    _lib.call("sn_bsr4_count", _p(rowptr), _p(colind), M, K, _p(b_rowptr), _p(ws), ws_bytes, _stream())
    nblocks = int(b_rowptr[-1].item())
    b_colind = torch.empty(nblocks, dtype=torch.int32, device=dev)
    b_vals = torch.empty(max(nblocks, 1) * 16, dtype=torch.float32, device=dev)[: nblocks * 16]
    _lib.call("sn_bsr4_fill", _p(rowptr), _p(colind), _p(vals), M, K, _p(b_rowptr), _p(b_colind), _p(b_vals), _stream())
    return b_rowptr, b_colind, b_vals


def blockdiag_concat(pool_rowptr, pool_colind, pool_vals, desc, size0: int, size1: int, total: int, vpe: int = 1):
    """Batch assembly from the resident pool; `desc` is the (B,4) int64 table of include/sn_spmm.h (device)."""
    _dev(pool_rowptr, pool_colind, pool_vals, desc)
    B = int(desc.shape[0])
    dev = pool_rowptr.device
    out_rowptr = torch.empty(B * size0 + 1, dtype=torch.int32, device=dev)
    out_colind = torch.empty(total, dtype=torch.int32, device=dev) if vpe != 4 else None      # Q3 records carry the column
    out_vals = torch.empty(total * vpe, dtype=torch.float32, device=dev)
    _lib.call("sn_blockdiag_concat_i32", _p(pool_rowptr), _p(pool_colind), _p(pool_vals), _p(desc), B, size0, size1,
              total, vpe, _p(out_rowptr), _p(out_colind), _p(out_vals), _stream())
    return out_rowptr, out_colind, out_vals


def blockdiag_concat_ragged(pool_rowptr, pool_colind, pool_vals, desc, total_rows: int, total_cols: int, total: int, vpe: int = 1):
    """Packed (unpadded) batch assembly; `desc` is the (B,6) int64 table of sn_blockdiag_concat_ragged_i32 (device)."""
    _dev(pool_rowptr, pool_colind, pool_vals, desc)
    B = int(desc.shape[0])
    dev = pool_rowptr.device
    out_rowptr = torch.empty(total_rows + 1, dtype=torch.int32, device=dev)
    out_colind = torch.empty(total, dtype=torch.int32, device=dev) if vpe != 4 else None      # Q3 records carry the column
    out_vals = torch.empty(total * vpe, dtype=torch.float32, device=dev)
    _lib.call("sn_blockdiag_concat_ragged_i32", _p(pool_rowptr), _p(pool_colind), _p(pool_vals), _p(desc), B, total_rows,
              total_cols, total, vpe, _p(out_rowptr), _p(out_colind), _p(out_vals), _stream())
    return out_rowptr, out_colind, out_vals


def validate_csr(rowptr, colind, vals, M: int, K: int) -> int:
    """Bit set of defects of a CSR operator (0 = well formed), see sn_validate_csr_i32.  Synchronises (reads the flags)."""
    _dev(rowptr, colind, vals)
    flags = torch.empty(1, dtype=torch.int32, device=rowptr.device)
    _lib.call("sn_validate_csr_i32", _p(rowptr), _p(colind), _p(vals), M, K, int(colind.numel()), _p(flags), _stream())
    return int(flags.item())


def elu_into(src, dst) -> None:
    """dst <- elu(src); both 2-D (rows, C) views with contiguous rows (dst may be half of a concat buffer)."""
    _dev(src, dst)
    if src.shape != dst.shape:
        raise ValueError("elu_into: shape mismatch")
    _lib.call("sn_elu_into_f32", _p(src), _ld(src), _p(dst), _ld(dst), src.shape[0], src.shape[1], _stream())


def elu_bwd(gdst, out, gsrc, accumulate: bool, gdst2=None, gadd=None) -> None:
    """gsrc (+)= (gdst + gdst2) * elu'(.) + gadd, the derivative expressed through the activation output `out`."""
    _dev(gdst, out, gsrc, gdst2, gadd)
    for t in (gdst2, gadd):
        if t is not None and t.shape != out.shape:
            raise ValueError("elu_bwd: shape mismatch")
    if not (gdst.shape == out.shape == gsrc.shape):
        raise ValueError("elu_bwd: shape mismatch")
    _lib.call("sn_elu_bwd_acc_f32", _p(gdst), _ld(gdst), _p(gdst2), _ld(gdst2) if gdst2 is not None else 0, _p(gadd),
              _ld(gadd) if gadd is not None else 0, _p(out), _ld(out), _p(gsrc), _ld(gsrc), out.shape[0], out.shape[1],
              1 if accumulate else 0, _stream())


def colstats(x):
    """(2, C) float64: column sums and column sums of squares of the 2-D view x (contiguous rows, any row stride)."""
    _dev(x)
    rows, C = x.shape
    out = torch.empty((2, C), dtype=torch.float64, device=x.device)
    ws, ws_bytes = _workspace("sn_colstats_workspace_bytes", x.device, rows, C)
    _lib.call("sn_colstats_f32", _p(x), _ld(x), rows, C, _p(out), _p(ws), ws_bytes, _stream())
    return out


def wgrad_supported(J: int, C: int) -> bool:
    return C in (128, 256) and J <= 128 and J % 4 == 0


# ---- bounds of gradient tensors (max |dy|) for the two-piece weight gradient ------------------------------------------------
# A kernel that PRODUCES a gradient tensor (the input-gradient GEMM through the activation, the transposed quaternion product
# with the fused ELU backward) also leaves the per-workgroup maxima of what it wrote; the weight gradient of the layer below
# reads that tensor as its dy operand and needs the bound before its first row (sn_wgrad_*_bounded_f32).  Between the two
# lie autograd's view nodes (a block returns (rows, C), the next one receives (B, V, C).reshape(...): new tensor objects, same
# memory), so the bound travels in a small table keyed by the data pointer.  An entry holds a strong reference to the tensor it
# describes — its memory cannot be handed to another tensor while the entry lives — and the tensor's version counter (an
# in-place edit invalidates it); only the last few entries are kept (a gradient is consumed within a few launches).
_ABSMAX_KEEP = 8
_absmax_table = {}          # data_ptr -> (tensor, version, maxima)
_absmax_enabled = None


def absmax_wanted() -> bool:
    """Whether producers of gradient tensors should leave their maxima: asked of the library once (sn_wgrad_bounded_enabled —
    the one place that decides whether the bounded two-piece weight gradient runs)."""
    global _absmax_enabled
    if _absmax_enabled is None:
        _absmax_enabled = bool(_lib.load().sn_wgrad_bounded_enabled())
    return _absmax_enabled


def note_absmax(t, maxima) -> None:
    """Record that max |t| <= max(maxima) (a device tensor of per-workgroup maxima left by the kernel that wrote t)."""
    if maxima is None:
        return
    if len(_absmax_table) >= _ABSMAX_KEEP:
        for k in list(_absmax_table)[: len(_absmax_table) - _ABSMAX_KEEP + 1]:      # dicts keep insertion order: oldest first
            del _absmax_table[k]
    _absmax_table.pop(t.data_ptr(), None)
    _absmax_table[t.data_ptr()] = (t, t._version if not t.is_inference() else None, maxima)
    rec = _lib.recorder() if _lib._recorder is not None else None
    if rec is not None:                     # (a launch plan re-attaches what is still noted when its dry run ends)
        rec.notes.append((t, maxima))


def clear_absmax() -> None:
    """Drop every recorded bound (and with it the references to the gradient tensors they describe): called by the train steps
    once a backward pass has run — bounds nobody took (a gradient consumed only as an added term, the gradient into the first
    layer) would otherwise keep up to _ABSMAX_KEEP gradient tensors alive across steps.  The tails of raw gradients go too."""
    _absmax_table.clear()
    _tail_table.clear()


# ---- raw face gradients (blocks.DEFER_FACE_TAIL) ----------------------------------------------------------------------------------
# A Dirac block may return the gradient of its face input RAW (linear_dgrad_elu_raw: the bare GEMM product) for the previous
# block's transposed product to finish.  What that product needs besides the gradient — the low halves of the stage's mean / B /
# C vectors — travels like the maxima above: keyed by the gradient's data pointer, with a strong reference to the tensor and its
# version counter, re-attached by a launch plan through `rec.tail_notes`.
_tail_table = {}            # data_ptr -> (tensor, version, (center, B, Cc))


def note_tail(t, tail) -> None:
    """Record that t is a raw gradient and `tail` = (center, B, Cc) finishes it."""
    if len(_tail_table) >= _ABSMAX_KEEP:
        for k in list(_tail_table)[: len(_tail_table) - _ABSMAX_KEEP + 1]:
            del _tail_table[k]
    _tail_table.pop(t.data_ptr(), None)
    _tail_table[t.data_ptr()] = (t, t._version if not t.is_inference() else None, tuple(tail))
    rec = _lib.recorder() if _lib._recorder is not None else None
    if rec is not None:
        rec.tail_notes.append((t, tuple(tail)))


def has_tail(t) -> bool:
    """Whether take_tail(t) would succeed (nothing is taken)."""
    ent = _tail_table.get(t.data_ptr())
    if ent is None:
        return False
    src, version, _ = ent
    return src.numel() == t.numel() and t.is_contiguous() and src.dtype == t.dtype and \
        (version is None or src._version == version)


def take_tail(t):
    """The tail recorded for exactly this memory (same first element, element count and contents), or None."""
    ent = _tail_table.pop(t.data_ptr(), None)
    if ent is None:
        return None
    src, version, tail = ent
    rec = _lib.recorder() if _lib._recorder is not None else None
    if rec is not None:
        rec.tail_notes[:] = [n for n in rec.tail_notes if n[1] is not tail]
    if src.numel() != t.numel() or not t.is_contiguous() or src.dtype != t.dtype or \
            (version is not None and src._version != version):
        return None
    return tail


def take_absmax(t):
    """The maxima recorded for exactly this memory (same first element, element count and contents), or None."""
    ent = _absmax_table.pop(t.data_ptr(), None)
    if ent is None:
        return None
    src, version, maxima = ent
    rec = _lib.recorder() if _lib._recorder is not None else None
    if rec is not None:
        rec.notes[:] = [n for n in rec.notes if n[1] is not maxima]
    if src.numel() != t.numel() or not t.is_contiguous() or src.dtype != t.dtype or \
            (version is not None and src._version != version):
        return None
    return maxima


def _bounds_args(bounds, C: int):
    """(dybound (n,) fp32, invstd (C,) fp32, stat_rows) -> the trailing arguments of the sn_wgrad_*_bounded_f32 calls."""
    dyb, invstd, stat_rows = bounds
    _dev(dyb, invstd)
    if dyb.dtype != torch.float32 or not dyb.is_contiguous() or invstd.dtype != torch.float32 or invstd.numel() != C or \
            not invstd.is_contiguous():
        raise ValueError("wgrad bounds: fp32 maxima of |dy| (contiguous) and the (C,) fp32 inverse standard deviations of x")
    return _p(dyb), int(dyb.numel()), _p(invstd), int(stat_rows)


def wgrad(dy, x, center=None, want_colsum: bool = False, bounds=None):
    """G = dy^T · (x - center) (J x C, fp32) for tall-skinny operands on the 16-bit matrix pipe (exact splits); see sn_wgrad_f32.
    want_colsum: also return colsum(dy) as a (J,) float64 tensor, accumulated by the same pass.
    bounds = (dybound, invstd, stat_rows): an upper bound of max |dy| (device, one float), BatchNorm's inverse standard
    deviations of x's columns about `center` and the row count behind them — the product then runs on two fp16 pieces
    (sn_wgrad_bounded_f32: half the matrix work of the three-piece bf16 form)."""
    _dev(dy, x, center)
    rows, J = dy.shape
    C = x.shape[1]
    if x.shape[0] != rows:
        raise ValueError("wgrad: row mismatch")
    G = torch.empty((J, C), dtype=torch.float32, device=x.device)
    dysum = torch.empty(J, dtype=torch.float64, device=x.device) if want_colsum else None
    ws, ws_bytes = _workspace("sn_wgrad_workspace_bytes", x.device, rows, J, C)
    if bounds is not None:
        _lib.call("sn_wgrad_bounded_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(center), rows, J, C, _p(G), _p(dysum), _p(ws), ws_bytes,
                  *_bounds_args(bounds, C), _stream())
    else:
        _lib.call("sn_wgrad_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(center), rows, J, C, _p(G), _p(dysum), _p(ws), ws_bytes,
                  _stream())
    return (G, dysum) if want_colsum else G


def affine_cols_acc(dx, x, B, Cc, center=None) -> None:
    """dx[r,c] += (x[r,c] - center[c])*B[c] + Cc[c] in place."""
    _dev(dx, x, B, Cc, center)
    if dx.shape != x.shape or B.numel() != x.shape[1] or Cc.numel() != x.shape[1]:
        raise ValueError("affine_cols_acc: shape mismatch")
    _lib.call("sn_affine_cols_acc_f32", _p(dx), _ld(dx), _p(x), _ld(x), _p(center), _p(B), _p(Cc), x.shape[0], x.shape[1], _stream())


def affine_cols_elu_bwd(dx, x, B=None, Cc=None, center=None) -> None:
    """dx[r,c] = (dx[r,c] + (x[r,c] - center[c])*B[c] + Cc[c]) * elu'(.) in place, x = the ELU OUTPUT that fed the layer
    (sn_affine_cols_elu_bwd_f32); B = Cc = None: only the activation derivative."""
    _dev(dx, x, B, Cc, center)
    if dx.shape != x.shape or (B is not None and (B.numel() != x.shape[1] or Cc is None or Cc.numel() != x.shape[1])):
        raise ValueError("affine_cols_elu_bwd: shape mismatch")
    _lib.call("sn_affine_cols_elu_bwd_f32", _p(dx), _ld(dx), _p(x), _ld(x), _p(center), _p(B), _p(Cc), x.shape[0], x.shape[1],
              _stream())


def bn_fold(stats, rows: int, gamma, beta, W, b, eps: float, momentum: float, training: bool, running_mean, running_var,
            num_batches_tracked=None):
    """Fold BatchNorm into the Linear weights (see sn_bn_fold_f32). Returns (mean, invstd, s, t, Wf, bf); updates the
    running statistics (and the int64 batch counter, when given) in place when training."""
    _dev(stats, gamma, beta, W, b, running_mean, running_var, num_batches_tracked)
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise TypeError("num_batches_tracked must be int64")
    J, C = W.shape
    dev = W.device
    vec = torch.empty((4, C), dtype=torch.float32, device=dev)
    Wf = torch.empty((J, C), dtype=torch.float32, device=dev)
    bf = torch.empty(J, dtype=torch.float32, device=dev)
    _lib.call("sn_bn_fold_f32", _p(stats), rows, _p(gamma), _p(beta), _p(W.contiguous()), _p(b), J, C, float(eps),
              float(momentum), 1 if training else 0, _p(running_mean), _p(running_var), _p(vec[0]), _p(vec[1]),
              _p(vec[2]), _p(vec[3]), _p(Wf), _p(bf), _p(num_batches_tracked), _stream())
    return vec[0], vec[1], vec[2], vec[3], Wf, bf


def linear_fwd_stats_blocks(rows: int) -> int:
    """Partial rows the ELU-statistics epilogue of a forward GEMM over `rows` rows leaves (sn_linear_fwd_stats_blocks)."""
    return int(_lib.load().sn_linear_fwd_stats_blocks(rows))


def colstats_partial(x):
    """(partials (nblk, 2, C) float64, nblk): the statistics pass over the 2-D view x without its final reduction
    (sn_colstats_partial_f32)."""
    _dev(x)
    rows, C = x.shape
    nblk = int(_lib.load().sn_colstats_blocks(rows))
    part = torch.empty((max(nblk, 1), 2, C), dtype=torch.float64, device=x.device)
    _lib.call("sn_colstats_partial_f32", _p(x), _ld(x), rows, C, _p(part), _stream())
    return part, nblk


def bn_bwd_coeffs(Gc, dystats, W, s, invstd, beta, rows: int, has_bias: bool):
    """(dW, db, dgamma, dbeta, Bc, Cc) of the folded BatchNorm+Linear backward (see sn_bn_bwd_coeffs_f32)."""
    _dev(Gc, dystats, W, s, invstd, beta)
    J, C = W.shape
    dev = W.device
    dW = torch.empty((J, C), dtype=torch.float32, device=dev)
    db = torch.empty(J, dtype=torch.float32, device=dev) if has_bias else None
    vec = torch.empty((4, C), dtype=torch.float32, device=dev)
    _lib.call("sn_bn_bwd_coeffs_f32", _p(Gc), _p(dystats), _p(W.contiguous()), _p(s), _p(invstd), _p(beta.contiguous()),
              rows, J, C, _p(dW), _p(db), _p(vec[0]), _p(vec[1]), _p(vec[2]), _p(vec[3]), _stream())
    return dW, db, vec[0], vec[1], vec[2], vec[3]


def segment_colsum(x, mask, rows_per_seg: int, nseg: int):
    """(nseg, C) fp32: per-mesh masked column sums of the 2-D view x (nseg*rows_per_seg rows); mask is (rows,) or None."""
    _dev(x, mask)
    C = x.shape[1]
    if x.shape[0] != rows_per_seg * nseg:
        raise ValueError("segment_colsum: row count mismatch")
    out = torch.empty((nseg, C), dtype=torch.float32, device=x.device)
    ws, ws_bytes = _workspace("sn_segment_colsum_workspace_bytes", x.device, rows_per_seg, nseg, C)
    _lib.call("sn_segment_colsum_f32", _p(x), _ld(x), _p(mask), rows_per_seg, nseg, C, _p(out), _p(ws), ws_bytes, _stream())
    return out


def segment_colsum_ragged(x, tiles, seg_tile_ptr, nseg: int, scale=None):
    """(nseg, C) fp32: per-mesh column sums of the 2-D view x of a PACKED batch, times the optional per-mesh `scale`
    (sn_segment_colsum_ragged_f32); tiles / seg_tile_ptr: the int64 device tables of operators.PackedSegments."""
    _dev(x, tiles, seg_tile_ptr, scale)
    C = x.shape[1]
    nt = int(tiles.shape[0])
    out = torch.empty((nseg, C), dtype=torch.float32, device=x.device)
    ws, ws_bytes = _workspace("sn_segment_colsum_ragged_workspace_bytes", x.device, nt, C)
    _lib.call("sn_segment_colsum_ragged_f32", _p(x), _ld(x), _p(tiles), nt, _p(seg_tile_ptr), nseg, C, _p(scale), _p(out), _p(ws),
              ws_bytes, _stream())
    return out


def bcast_rows_ragged(src, tiles, dst) -> None:
    """dst[r, :] = src[mesh(r), :] for a PACKED batch (sn_bcast_rows_ragged_f32)."""
    _dev(src, tiles, dst)
    if dst.shape[1] != src.shape[1]:
        raise ValueError("bcast_rows_ragged: shape mismatch")
    _lib.call("sn_bcast_rows_ragged_f32", _p(src.contiguous()), _p(tiles), int(tiles.shape[0]), _p(dst), _ld(dst), src.shape[1], _stream())


def bcast_rows(src, dst, rows_per_seg: int) -> None:
    """dst[r, :] = src[r // rows_per_seg, :]."""
    _dev(src, dst)
    nseg, C = src.shape
    if dst.shape[0] != nseg * rows_per_seg or dst.shape[1] != C:
        raise ValueError("bcast_rows: shape mismatch")
    _lib.call("sn_bcast_rows_f32", _p(src), _p(dst), _ld(dst), rows_per_seg, nseg, C, _stream())


def elu_bwd_bcast(gdst, out, bias, mask, gsrc, rows_per_seg: int, gadd=None) -> None:
    """gsrc = (gdst + mask[r] * bias[mesh(r)]) * elu'(out) + gadd."""
    _dev(gdst, out, bias, mask, gsrc, gadd)
    nseg, C = bias.shape
    _lib.call("sn_elu_bwd_bcast_f32", _p(gdst), _ld(gdst), _p(out), _ld(out), _p(bias), _p(mask), _p(gadd),
              _ld(gadd) if gadd is not None else 0, _p(gsrc), _ld(gsrc), rows_per_seg, nseg, C, _stream())


def dirac_from_mesh(V, F):
    """Dirac operators of one triangle mesh (or of a batch laid out as one disjoint mesh) built on the device.
    V: (nV, 3) fp32, F: (nF, 3) int32.  Returns four BSR4 triples (rowptr, colind, vals):
    Di (4nF x 4nV), DiAT (= DiA^T, Di's structure), DiA (4nV x 4nF), DiT (= Di^T, DiA's structure)."""
    _dev(V, F)
    if V.dtype != torch.float32 or F.dtype != torch.int32 or V.shape[1] != 3 or F.shape[1] != 3:
        raise TypeError("dirac_from_mesh wants V (nV,3) float32 and F (nF,3) int32")
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
    di_rp, di_ci, di_v, diat_v = i32(nF + 1), i32(3 * nF), f32(48 * nF), f32(48 * nF)
    dia_rp, dia_ci, dia_v, dit_v = i32(nV + 1), i32(3 * nF), f32(48 * nF), f32(48 * nF)
    ws, ws_bytes = _workspace("sn_dirac_workspace_bytes", dev, nV, nF)
    _lib.call("sn_dirac_bsr4_from_mesh", _p(V), _p(F), nV, nF, _p(di_rp), _p(di_ci), _p(di_v), _p(diat_v), _p(dia_rp),
              _p(dia_ci), _p(dia_v), _p(dit_v), _p(ws), ws_bytes, _stream())
    return (di_rp, di_ci, di_v), (di_rp, di_ci, diat_v), (dia_rp, dia_ci, dia_v), (dia_rp, dia_ci, dit_v)


def laplacian_from_mesh(V, F):
    """Mass-normalised cotangent Laplacian of one mesh (or a batch laid out as one disjoint mesh) built on the device:
    (rowptr, colind, vals) CSR.  Synchronises once (reads nnz).  V: (nV,3) fp32, F: (nF,3) int32."""
    _dev(V, F)
    if V.dtype != torch.float32 or F.dtype != torch.int32:
        raise TypeError("laplacian_from_mesh wants V float32 and F int32")
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    rowptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_laplacian_workspace_bytes", dev, nV, nF)
    _lib.call("sn_laplacian_csr_from_mesh", _p(V), _p(F), nV, nF, 0, _p(rowptr), None, None, _p(flag), _p(ws), ws_bytes, _stream())
    nnz, bad = int(rowptr[-1].item()), int(flag.item())
    if bad:
        raise _lib.SnError("laplacian_from_mesh: a vertex has more incident faces than SN_LAP_MAX_DEGREE")
    colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.call("sn_laplacian_csr_from_mesh", _p(V), _p(F), nV, nF, 1, _p(rowptr), _p(colind), _p(vals), None, _p(ws), ws_bytes, _stream())
    return rowptr, colind, vals


def spgemm_max_window() -> int:
    """The widest result row csr_spgemm takes: columns between its first and last candidate, one bit each in LDS."""
    return int(_lib.load().sn_csr_spgemm_max_window())


def _check_csr(who: str, arrays, rows: int):
    rowptr, colind, vals = arrays
    _dev(rowptr, colind, vals)
    if rowptr.dtype != torch.int32 or colind.dtype != torch.int32 or vals.dtype != torch.float32:
        raise TypeError(f"{who} wants int32 rowptr/colind and float32 vals")
    if rowptr.dim() != 1 or rowptr.numel() != rows + 1 or colind.dim() != 1 or colind.shape != vals.shape:
        raise ValueError(f"{who}: inconsistent CSR arrays for {rows} rows")
    return rowptr.contiguous(), colind.contiguous(), vals.contiguous()


def raise_for_status(who: str, family: str, st: int, errors) -> None:
    """Raise for the first bit of `errors` — ((bit, exception type), ...), in the order they are tested — that is set in the
    status word st, with the sentence constants.STATUS_FAMILIES has for it."""
    for bit, exc in errors:
        if st & bit:
            raise exc(f"{who}: {constants.status_sentences(family, bit)[0]}")


def _raise_for_spgemm_status(who: str, st: int) -> None:
    raise_for_status(who, "spgemm", st, ((SPGEMM_BAD_COLUMN, ValueError), (CSR_NO_OFFDIAGONAL, ValueError),
                                         (SPGEMM_TOO_WIDE, RuntimeError), (SPGEMM_TOO_LARGE, RuntimeError)))


def csr_spgemm(A_arrays, B_arrays, shape, keep_zeros: bool = False):
    """C = A B of two CSR operands (sn_csr_spgemm_f32; the definition is in include/sn_spmm.h): A_arrays, B_arrays =
    (rowptr, colind, vals) int32/int32/fp32 with columns ascending inside a row, shape = (M, K, N).  Returns (rowptr, colind,
    vals), columns ascending, every sum sequential in fp32 over A's row, bit-reproducible.  An entry whose sum is exactly zero is
    dropped as scipy drops it; keep_zeros=True returns the structural result.  Synchronises twice (reads the two sizes and the
    status word).  ValueError for a column out of range, RuntimeError for a row wider than spgemm_max_window()."""
    M, K, N = (int(s) for s in shape)
    a_rp, a_ci, a_v = _check_csr("csr_spgemm (A)", A_arrays, M)
    b_rp, b_ci, b_v = _check_csr("csr_spgemm (B)", B_arrays, K)
    dev = a_rp.device
    ws, ws_bytes = _workspace("sn_csr_spgemm_workspace_bytes", dev, M)
    heads = torch.zeros(2, M + 1, dtype=torch.int32, device=dev)             # structural and final row pointers
    s_rp, rp = heads[0], heads[1]
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ops = (_p(a_rp), _p(a_ci), _p(a_v), _p(b_rp), _p(b_ci), _p(b_v), M, K, N)
    tail = (status.data_ptr(), _p(ws), ws_bytes, _stream())
    _lib.call("sn_csr_spgemm_f32", *ops, 0, s_rp.data_ptr(), None, None, None, None, None, *tail)
    st, nnz_s = int(status.item()), int(s_rp[-1].item())
    _raise_for_spgemm_status("csr_spgemm", st)
    s_ci = torch.empty(nnz_s, dtype=torch.int32, device=dev)
    s_v = torch.empty(nnz_s, dtype=torch.float32, device=dev)
    _lib.call("sn_csr_spgemm_f32", *ops, 1, s_rp.data_ptr(), _p(s_ci), _p(s_v), rp.data_ptr(), None, None, *tail)
    if keep_zeros:
        return s_rp, s_ci, s_v
    nnz = int(rp[-1].item())
    if nnz == nnz_s:                                                         # nothing cancelled: the structural arrays are the result
        return s_rp, s_ci, s_v
    ci = torch.empty(nnz, dtype=torch.int32, device=dev)
    v = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.call("sn_csr_spgemm_f32", *ops, 2, s_rp.data_ptr(), _p(s_ci), _p(s_v), rp.data_ptr(), _p(ci), _p(v), *tail)
    return rp, ci, v


def csr_inv_sqrt_degree(rowptr, check: bool = True):
    """d[i] = (float)(1 / sqrt(entries of row i - 1)) in fp64, numpy's value (sn_csr_inv_sqrt_degree_f32): the D^-1/2 of
    src/dense_correspondence/main.py:77.  check: read the status word (one synchronisation) and raise ValueError for a row
    with fewer than two entries, where the host divides by zero; else the 1-element status tensor is returned with d."""
    _dev(rowptr)
    if rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise TypeError("csr_inv_sqrt_degree wants an int32 rowptr of M + 1 entries")
    rowptr = rowptr.contiguous()
    M = rowptr.numel() - 1
    d = torch.empty(M, dtype=torch.float32, device=rowptr.device)
    status = torch.empty(1, dtype=torch.int32, device=rowptr.device)
    _lib.call("sn_csr_inv_sqrt_degree_f32", rowptr.data_ptr(), M, _p(d), status.data_ptr(), _stream())
    if not check:
        return d, status
    _raise_for_spgemm_status("csr_inv_sqrt_degree", int(status.item()))
    return d


def csr_scale_sym(A_arrays, d, M: int):
    """out_ij = fl(fl(d_i a_ij) d_j) of a square CSR matrix (sn_csr_scale_sym_f32): what `Dsq.dot(L).dot(Dsq)` gives
    (main.py:78, 82), exact-zero results dropped as scipy's two diagonal products drop them.  Returns (rowptr, colind, vals);
    colind is A's own tensor when nothing was dropped.  Synchronises once."""
    M = int(M)
    a_rp, a_ci, a_v = _check_csr("csr_scale_sym", A_arrays, M)
    _dev(d)
    if d.dtype != torch.float32 or d.dim() != 1 or d.numel() != M:
        raise TypeError(f"csr_scale_sym wants d float32 of {M} entries")
    d = d.contiguous()
    dev = a_rp.device
    ws, ws_bytes = _workspace("sn_csr_spgemm_workspace_bytes", dev, M)
    rp = torch.empty(M + 1, dtype=torch.int32, device=dev)
    s_v = torch.empty_like(a_v)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    args = (_p(a_rp), _p(a_ci), _p(a_v), _p(d), M)
    tail = (status.data_ptr(), _p(ws), ws_bytes, _stream())
    _lib.call("sn_csr_scale_sym_f32", *args, 0, _p(s_v), rp.data_ptr(), None, None, *tail)
    st, nnz = int(status.item()), int(rp[-1].item())
    _raise_for_spgemm_status("csr_scale_sym", st)
    if nnz == a_ci.numel():
        return rp, a_ci, s_v
    ci = torch.empty(nnz, dtype=torch.int32, device=dev)
    v = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.call("sn_csr_scale_sym_f32", *args, 1, _p(s_v), rp.data_ptr(), _p(ci), _p(v), *tail)
    return rp, ci, v


IDT_CHUNK = 8                 # flip rounds enqueued between two reads of the counters


def _check_mesh(who: str, V, F) -> None:
    if F.dtype != torch.int32 or F.dim() != 2 or F.shape[1] != 3:
        raise TypeError(f"{who} wants F (nF, 3) int32")
    if V is not None and (V.dtype != torch.float32 or V.dim() != 2 or V.shape[1] != 3):
        raise TypeError(f"{who} wants V (nV, 3) float32")


def mesh_glue(F, num_vertices: int, V=None):
    """Glue map of a triangle mesh built on the device (sn_mesh_glue_i32; the definition is in include/sn_spmm.h, "Intrinsic
    Delaunay Laplacian"): G (nF, 3) int32 of face-side codes 3 g + t, -1 on the boundary, and the status word (1-element int32
    device tensor, not read here: IDT_BAD_FACE / IDT_NON_MANIFOLD / IDT_ORIENTATION).  With V (nV, 3) fp32 also the fp64 side
    lengths (nF, 3): returns (G, status, l)."""
    _dev(F, V)
    _check_mesh("mesh_glue", V, F)
    F = F.contiguous()
    nV, nF = int(num_vertices), F.shape[0]
    dev = F.device
    G = torch.empty(nF, 3, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    l = None
    if V is not None:
        if V.shape[0] != nV:
            raise ValueError(f"mesh_glue: V has {V.shape[0]} rows for {nV} vertices")
        V = V.contiguous()
        l = torch.empty(nF, 3, dtype=torch.float64, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_glue_workspace_bytes", dev, nV, nF)
    _lib.call("sn_mesh_glue_i32", _p(V) if V is not None else None, _p(F), nV, nF, _p(G), _p(l) if l is not None else None,
              status.data_ptr(), _p(ws), ws_bytes, _stream())
    return (G, status) if V is None else (G, status, l)


def intrinsic_delaunay(V, F, max_rounds: int = 1024):
    """Intrinsic Delaunay triangulation of one mesh (or a batch laid out as one disjoint mesh) by edge flips on the device
    (sn_mesh_glue_i32, sn_mesh_idt_rounds_f64; the definition is in include/sn_spmm.h).  V: (nV, 3) fp32, F: (nF, 3) int32.
    Returns (F', l', G, status, rounds, flips): faces (nF, 3) int32, fp64 side lengths (nF, 3), glue map (nF, 3) int32, the
    status word as a Python int (IDT_* bits; with a refusal bit nothing was flipped), the number of rounds run (the last one
    found nothing unless IDT_NOT_CONVERGED is set) and of flips done.  Rounds are enqueued IDT_CHUNK at a time; synchronises
    once per chunk (reads the counters and the status word).  Two runs give bit-identical results."""
    _dev(V, F)
    _check_mesh("intrinsic_delaunay", V, F)
    max_rounds = int(max_rounds)
    if not 1 <= max_rounds <= 1 << 20:
        raise ValueError("intrinsic_delaunay: max_rounds must be between 1 and 2**20")
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    G, status, l = mesh_glue(F, nV, V)
    Fp = F.contiguous().clone()
    counters = torch.empty(max_rounds, 2, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_idt_workspace_bytes", dev, nF)
    rounds = flips = 0
    while rounds < max_rounds:
        n = min(IDT_CHUNK, max_rounds - rounds)
        _lib.call("sn_mesh_idt_rounds_f64", _p(Fp), _p(l), _p(G), nF, rounds, n, max_rounds, counters.data_ptr(), status.data_ptr(),
                  _p(ws), ws_bytes, _stream())
        got = counters[rounds:rounds + n].cpu()
        idle = (got[:, 0] == 0).nonzero()
        flips += int(got[:, 1].sum())
        if idle.numel():
            rounds += int(idle[0]) + 1
            break
        rounds += n
    return Fp, l, G, int(status.item()), rounds, flips


def _raise_for_idt_status(who: str, st: int) -> None:
    raise_for_status(who, "idt", st,
                     ((IDT_BAD_FACE, ValueError), (IDT_NON_MANIFOLD, ValueError), (IDT_ORIENTATION, ValueError),
                      (IDT_NOT_CONVERGED, RuntimeError)))


def intrinsic_laplacian_from_mesh(V, F, max_rounds: int = 1024, state=None):
    """Mass-normalised cotangent Laplacian A^-1 (D - W) on the intrinsic Delaunay triangulation of one mesh (or a batch laid
    out as one disjoint mesh), built on the device: (rowptr, colind, vals) CSR, columns ascending, explicit zeros kept (the
    pattern is every intrinsic edge plus the diagonal).  Not the reference's unpublished seism matrix: its scaling and sign are
    unknown (include/sn_spmm.h).  state: the (F', l', ...) tuple of intrinsic_delaunay to build from, else it is run here.
    Raises ValueError for a refused mesh (naming the refusal) and RuntimeError when max_rounds rounds did not reach the fixed
    point.  torch.sort orders the contribution keys; everything else is this library's kernels."""
    _dev(V, F)
    _check_mesh("intrinsic_laplacian_from_mesh", V, F)
    if state is None:
        state = intrinsic_delaunay(V, F, max_rounds)
    Fp, l, _, st = state[:4]
    _raise_for_idt_status("intrinsic_laplacian_from_mesh", st)
    nV, nF = V.shape[0], Fp.shape[0]
    dev = V.device
    lib = _lib.load()
    N = int(lib.sn_mesh_idt_laplacian_items(nV, nF))
    ws, ws_bytes = _workspace("sn_mesh_idt_laplacian_workspace_bytes", dev, nV, nF)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    rowptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    args = (_p(Fp), _p(l), nV, nF)
    _lib.call("sn_mesh_idt_laplacian_f32", *args, 0, _p(keys), None, None, None, None, None, _p(ws), ws_bytes, _stream())
    skeys, order = torch.sort(keys)
    _lib.call("sn_mesh_idt_laplacian_f32", *args, 1, _p(skeys), _p(order), rowptr.data_ptr(), None, None, None, _p(ws), ws_bytes, _stream())
    nnz = int(rowptr[-1].item())
    colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.call("sn_mesh_idt_laplacian_f32", *args, 2, _p(skeys), _p(order), rowptr.data_ptr(), _p(colind), _p(vals), None, _p(ws), ws_bytes,
              _stream())
    return rowptr, colind, vals


_CC_MODES = {"edge": CC_EDGE, "vertex": CC_VERTEX}

MeshComponents = collections.namedtuple("MeshComponents", "vlabel flabel count summary status")
MeshCompacted = collections.namedtuple("MeshCompacted", "I J Fsrc Fnew Vnew sizes")


def mesh_components(F, num_vertices: int, mode: str = "edge") -> MeshComponents:
    """Connected components of a triangle mesh on the device (sn_mesh_components_i32; the definition is in include/sn_spmm.h,
    "Mesh clean-up", the host statement is mesh_ops.components).  F: (nF, 3) int32.  mode "edge": faces joined across shared
    edges (igl.facet_components), labels are face ids; "vertex": vertices joined by faces, labels are vertex ids.
    Returns MeshComponents(vlabel, flabel, count, summary, status), int32 device tensors: vlabel (nV,) in vertex mode, None in
    edge mode; flabel (nF,), -1 for a bad face; count (nV,) or (nF,); summary (3,) = labels with a face, the winning label,
    its face count; status (1,) with the CC_BAD_FACE / CC_INTERNAL bits.  Does not synchronise; two runs are bit-identical."""
    _dev(F)
    _check_mesh("mesh_components", None, F)
    if mode not in _CC_MODES:
        raise ValueError(f'mesh_components: mode must be "edge" or "vertex", got {mode!r}')
    F = F.contiguous()
    nV, nF = int(num_vertices), F.shape[0]
    if nV < 0:
        raise ValueError("mesh_components: num_vertices is negative")
    dev = F.device
    vertex = mode == "vertex"
    vlabel = torch.empty(nV, dtype=torch.int32, device=dev) if vertex else None
    flabel = torch.empty(nF, dtype=torch.int32, device=dev)
    count = torch.empty(nV if vertex else nF, dtype=torch.int32, device=dev)
    summary = torch.empty(3, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_components_workspace_bytes", dev, nV, nF, _CC_MODES[mode])
    _lib.call("sn_mesh_components_i32", _p(F), nV, nF, _CC_MODES[mode], _p(vlabel), _p(flabel), _p(count), summary.data_ptr(),
              status.data_ptr(), _p(ws), ws_bytes, _stream())
    return MeshComponents(vlabel, flabel, count, summary, status)


def mesh_label_mask(flabel, label):
    """keep (nF,) int32 = (flabel == label) with label a 1-element int32 DEVICE tensor (e.g. summary[1:2] of mesh_components:
    the winner's faces without reading the label back); a negative label keeps nothing.  sn_mesh_label_mask_i32."""
    _dev(flabel, label)
    if flabel.dtype != torch.int32 or flabel.dim() != 1 or label.dtype != torch.int32 or label.numel() != 1:
        raise TypeError("mesh_label_mask wants flabel (nF,) int32 and a 1-element int32 label tensor")
    flabel = flabel.contiguous()
    keep = torch.empty_like(flabel)
    _lib.call("sn_mesh_label_mask_i32", _p(flabel), flabel.shape[0], label.data_ptr(), _p(keep), _stream())
    return keep


def mesh_compact(F, keep, num_vertices: int, V=None) -> MeshCompacted:
    """Keep the good faces with keep[f] != 0 and the vertices they still use (igl.slice + igl.remove_unreferenced) on the device:
    sn_mesh_compact_i32, host statement mesh_ops.compact.  F: (nF, 3) int32, keep: (nF,) int32, V: (nV, 3) fp32 or None.
    Returns MeshCompacted(I, J, Fsrc, Fnew, Vnew, sizes), device tensors SIZED FOR THE WORST CASE: I (nV,) old -> new vertex id
    or -1; J (nV,) new -> old, ascending; Fsrc (nF,) original index of each kept face, ascending; Fnew (nF, 3) renumbered;
    Vnew (nV, 3) = V[J] (None without V); sizes (2,) int32 = (nV', nF'): the first nV' entries of J and Vnew and the first nF'
    of Fsrc and Fnew are written.  Does not synchronise: the caller reads `sizes` when it needs the lengths."""
    _dev(F, keep, V)
    _check_mesh("mesh_compact", V, F)
    if keep.dtype != torch.int32 or keep.dim() != 1:
        raise TypeError("mesh_compact wants keep (nF,) int32")
    nV, nF = int(num_vertices), F.shape[0]
    if keep.shape[0] != nF:
        raise ValueError(f"mesh_compact: keep has {keep.shape[0]} entries for {nF} faces")
    if nV < 0 or (V is not None and V.shape[0] != nV):
        raise ValueError(f"mesh_compact: V has {None if V is None else V.shape[0]} rows for {nV} vertices")
    F, keep = F.contiguous(), keep.contiguous()
    dev = F.device
    I = torch.empty(nV, dtype=torch.int32, device=dev)
    J = torch.empty(nV, dtype=torch.int32, device=dev)
    Fsrc = torch.empty(nF, dtype=torch.int32, device=dev)
    Fnew = torch.empty(nF, 3, dtype=torch.int32, device=dev)
    Vnew = None
    if V is not None:
        V = V.contiguous()
        Vnew = torch.empty(nV, 3, dtype=torch.float32, device=dev)
    sizes = torch.empty(2, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_compact_workspace_bytes", dev, nV, nF)
    _lib.call("sn_mesh_compact_i32", _p(V), _p(F), _p(keep), nV, nF, _p(I), _p(J), _p(Fsrc), _p(Fnew), _p(Vnew), sizes.data_ptr(),
              _p(ws), ws_bytes, _stream())
    return MeshCompacted(I, J, Fsrc, Fnew, Vnew, sizes)


MeshWeld = collections.namedtuple("MeshWeld", "rep F counts status")
MeshUniqueFaces = collections.namedtuple("MeshUniqueFaces", "keep counts status")
MeshOrient = collections.namedtuple("MeshOrient", "flip label F counts status")


def mesh_weld(V, F, tol: float = 0.0, weld: bool = True) -> MeshWeld:
    """Weld the vertices with equal keys on the device (sn_mesh_weld_f32; the definition is in include/sn_spmm.h, "Mesh
    repair", the host statement is mesh_ops.weld_vertices).  V: (nV, 3) fp32, F: (nF, 3) int32.  tol == 0: equal coordinates
    (-0.0 == +0.0); tol > 0: equal cells of the grid rint(x / tol).  weld=False welds nothing and only marks the vertices with a
    non-finite coordinate.  Returns MeshWeld(rep, F, counts, status), int32 device tensors: rep (nV,) the smallest vertex id of
    each vertex's class; F (nF, 3) rewritten through rep, -1 for an unweldable vertex; counts (1,) = vertices with rep != id;
    status (1,) with the REPAIR_* bits.  Does not synchronise; two runs are bit-identical."""
    _dev(V, F)
    _check_mesh("mesh_weld", V, F)
    tol = float(tol)
    if not 0.0 <= tol < float("inf"):
        raise ValueError(f"mesh_weld: tol must be finite and >= 0, got {tol!r}")
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    rep = torch.empty(nV, dtype=torch.int32, device=dev)
    Fw = torch.empty(nF, 3, dtype=torch.int32, device=dev)
    counts = torch.empty(1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_weld_workspace_bytes", dev, nV)
    _lib.call("sn_mesh_weld_f32", _p(V), _p(F), nV, nF, tol, 1 if weld else 0, _p(rep), _p(Fw), counts.data_ptr(), status.data_ptr(),
              _p(ws), ws_bytes, _stream())
    return MeshWeld(rep, Fw, counts, status)


def mesh_unique_faces(F, num_vertices: int, V=None, unique: bool = True) -> MeshUniqueFaces:
    """The faces that stay (sn_mesh_unique_faces_i32, host statement mesh_ops.unique_faces): keep (nF,) int32 = 1 for a good face
    that has the smallest face id on its unordered vertex triple (unique=False: for every good face); counts (3,) int32 = bad
    faces, duplicate faces, kept faces of fp64 double-area exactly 0 (0 without V); status (1,).  F: (nF, 3) int32, as a rule
    the F of mesh_weld; V: (nV, 3) fp32 or None.  Does not synchronise; two runs are bit-identical."""
    _dev(F, V)
    _check_mesh("mesh_unique_faces", V, F)
    nV, nF = int(num_vertices), F.shape[0]
    if nV < 0 or (V is not None and V.shape[0] != nV):
        raise ValueError(f"mesh_unique_faces: V has {None if V is None else V.shape[0]} rows for {nV} vertices")
    F = F.contiguous()
    V = None if V is None else V.contiguous()
    dev = F.device
    keep = torch.empty(nF, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_unique_faces_workspace_bytes", dev, nF)
    _lib.call("sn_mesh_unique_faces_i32", _p(V), _p(F), nV, nF, 1 if unique else 0, _p(keep), counts.data_ptr(), status.data_ptr(),
              _p(ws), ws_bytes, _stream())
    return MeshUniqueFaces(keep, counts, status)


def mesh_orient(F, keep, num_vertices: int) -> MeshOrient:
    """A consistent winding for every orientation class of the kept faces (sn_mesh_orient_i32, host statement
    mesh_ops.orient_faces).  F: (nF, 3) int32, keep: (nF,) int32.  Returns MeshOrient(flip, label, F, counts, status), int32
    device tensors: flip (nF,) 1 where (a, b, c) became (a, c, b); label (nF,) the smallest face id of the face's class, -1 for
    a face that is not kept; F (nF, 3) the faces after the turns; counts (3,) = edges with three and more faces, classes without
    a consistent winding (left as they came), classes; status (1,).  Does not synchronise; two runs are bit-identical."""
    _dev(F, keep)
    _check_mesh("mesh_orient", None, F)
    if keep.dtype != torch.int32 or keep.dim() != 1:
        raise TypeError("mesh_orient wants keep (nF,) int32")
    nV, nF = int(num_vertices), F.shape[0]
    if keep.shape[0] != nF:
        raise ValueError(f"mesh_orient: keep has {keep.shape[0]} entries for {nF} faces")
    if nV < 0:
        raise ValueError("mesh_orient: num_vertices is negative")
    F, keep = F.contiguous(), keep.contiguous()
    dev = F.device
    flip = torch.empty(nF, dtype=torch.int32, device=dev)
    label = torch.empty(nF, dtype=torch.int32, device=dev)
    Fout = torch.empty(nF, 3, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_orient_workspace_bytes", dev, nV, nF)
    _lib.call("sn_mesh_orient_i32", _p(F), _p(keep), nV, nF, _p(flip), _p(label), _p(Fout), counts.data_ptr(), status.data_ptr(),
              _p(ws), ws_bytes, _stream())
    return MeshOrient(flip, label, Fout, counts, status)


# output name -> (per face?, trailing width) in the argument order of sn_mesh_descriptors_f32
DESCRIPTOR_FIELDS = {"face_area": (True, 1), "face_normal": (True, 3), "n_area": (False, 3), "n_uniform": (False, 3),
                     "n_angle": (False, 3), "mass_bary": (False, 1), "mass_voronoi": (False, 1), "gauss": (False, 1),
                     "mean": (False, 1)}
_DESC_MASS = {"barycentric": DESC_MASS_BARYCENTRIC, "voronoi": DESC_MASS_VORONOI}


def _new_outputs(who: str, fields: dict, want, layout, dev) -> dict:
    """The optional outputs of an entry point over its FIELDS table: a new device tensor for every name of `want` (None: all of
    `fields`), None for the others, and "status", a 1-element int32 tensor.  layout(entry) = (rows, trailing width, dtype)."""
    names = list(fields) if want is None else list(want)
    unknown = [n for n in names if n not in fields]
    if unknown:
        raise ValueError(f"{who}: unknown output {unknown[0]!r}; the outputs are {', '.join(fields)}")
    out = {}
    for name, entry in fields.items():
        rows, width, dtype = layout(entry)
        out[name] = torch.empty((rows,) if width == 1 else (rows, width), dtype=dtype, device=dev) if name in names else None
    out["status"] = torch.empty(1, dtype=torch.int32, device=dev)
    return out


def mesh_descriptors(V, F, want=None) -> dict:
    """Per-face and per-vertex geometry of one triangle mesh (or a batch laid out as one disjoint mesh) on the device:
    sn_mesh_descriptors_f32, definition in include/sn_spmm.h ("Mesh descriptors"), host statement mesh_ops.vertex_descriptors.
    V: (nV, 3) fp32, F: (nF, 3) int32.  want: the names of DESCRIPTOR_FIELDS to compute, None = all.  Returns a dict with every
    name of DESCRIPTOR_FIELDS — an fp32 device tensor (nF,), (nF, 3), (nV,) or (nV, 3), or None when it was not asked for — plus
    "status": a 1-element int32 device tensor of DESC_* bits, not read here.  Any number of faces at a vertex.  Does not
    synchronise; two runs are bit-identical."""
    _dev(V, F)
    _check_mesh("mesh_descriptors", V, F)
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    out = _new_outputs("mesh_descriptors", DESCRIPTOR_FIELDS, want, lambda f: (nF if f[0] else nV, f[1], torch.float32), dev)
    ws, ws_bytes = _workspace("sn_mesh_descriptors_workspace_bytes", dev, nV, nF)
    _lib.call("sn_mesh_descriptors_f32", _p(V), _p(F), nV, nF, *[_p(out[n]) for n in DESCRIPTOR_FIELDS], out["status"].data_ptr(),
              _p(ws), ws_bytes, _stream())
    return out


# output name -> (dtype, trailing width) in the argument order of sn_mesh_principal_curvature_f32
CURVATURE_FIELDS = {"k1": (torch.float32, 1), "k2": (torch.float32, 1), "d1": (torch.float32, 3), "d2": (torch.float32, 3),
                    "ring_size": (torch.int32, 1)}


def mesh_principal_curvature(V, F, radius: int = 5, want=None) -> dict:
    """Principal curvatures k1 >= k2 and their directions from a quadric fitted over the `radius`-ring patch of every vertex of
    one triangle mesh (or a batch laid out as one disjoint mesh) on the device: sn_mesh_principal_curvature_f32, definition in
    include/sn_spmm.h ("Principal curvatures"), host statement mesh_ops.principal_curvatures, equal to it bit for bit.
    V: (nV, 3) fp32, F: (nF, 3) int32.  want: the names of CURVATURE_FIELDS to compute, None = all.  Returns a dict with every
    name of CURVATURE_FIELDS — k1, k2 (nV,) fp32, d1, d2 (nV, 3) fp32, ring_size (nV,) int32, or None when it was not asked
    for — plus "status": a 1-element int32 device tensor of DESC_BAD_FACE and CURV_* bits, not read here.  A vertex that failed
    holds NaN.  Does not synchronise; two runs are bit-identical."""
    _dev(V, F)
    _check_mesh("mesh_principal_curvature", V, F)
    radius = int(radius)
    if radius < 1:
        raise ValueError(f"mesh_principal_curvature: radius must be at least 1, got {radius}")
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    out = _new_outputs("mesh_principal_curvature", CURVATURE_FIELDS, want, lambda f: (nV, f[1], f[0]), dev)
    ws, ws_bytes = _workspace("sn_mesh_curvature_workspace_bytes", dev, nV, nF)
    _lib.call("sn_mesh_principal_curvature_f32", _p(V), _p(F), nV, nF, radius, *[_p(out[n]) for n in CURVATURE_FIELDS],
              out["status"].data_ptr(), _p(ws), ws_bytes, _stream())
    return out


def cot_laplacian_from_mesh(V, F, mass: str = "barycentric", hack=None):
    """The libigl-convention Laplacian L = M^-1 C of one mesh (or a batch laid out as one disjoint mesh) built on the device:
    (rowptr, colind, vals, status) — CSR with ascending columns and explicit zeros kept, and the status word as a Python int
    (DESC_BAD_FACE / DESC_FLAT_FACE / DESC_CLAMPED).  sn_mesh_cot_laplacian_f32; host statement mesh_ops.libigl_laplacian.
    mass: "barycentric" | "voronoi".  hack: None, or the value put in place of every entry that is not finite or exceeds 1e10 in
    magnitude.  Synchronises twice (nnz and the status after each phase).  Raises SnError when a vertex has more than
    SN_LAP_MAX_DEGREE incident faces (DESC_DEGREE): nothing further is launched, there is no other path."""
    _dev(V, F)
    _check_mesh("cot_laplacian_from_mesh", V, F)
    if mass not in _DESC_MASS:
        raise ValueError(f'cot_laplacian_from_mesh: mass must be "barycentric" or "voronoi", got {mass!r}')
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    rowptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_cot_laplacian_workspace_bytes", dev, nV, nF)
    head = (_p(V), _p(F), nV, nF)
    tail = (_DESC_MASS[mass], int(hack is not None), float(0 if hack is None else hack))
    _lib.call("sn_mesh_cot_laplacian_f32", *head, 0, *tail, _p(rowptr), None, None, status.data_ptr(), _p(ws), ws_bytes, _stream())
    nnz, st = torch.cat([rowptr[-1:], status]).tolist()
    raise_for_status("cot_laplacian_from_mesh", "descriptors", st, ((DESC_DEGREE, _lib.SnError),))
    colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    vals = torch.empty(nnz, dtype=torch.float32, device=dev)
    _lib.call("sn_mesh_cot_laplacian_f32", *head, 1, *tail, _p(rowptr), _p(colind), _p(vals), status.data_ptr(), _p(ws), ws_bytes,
              _stream())
    return rowptr, colind, vals, int(status.item())


def cot_pencil_from_mesh(V, F):
    """The cotangent pencil of one mesh (or a batch laid out as one disjoint mesh) in fp64, built on the device:
    (rowptr, colind, S, mass, status) — S = -C in CSR with ascending columns, the diagonal and explicit zeros kept, symmetric bit
    for bit; mass (nV,) the unrounded Voronoi mass; status a Python int (DESC_BAD_FACE / DESC_FLAT_FACE).
    sn_mesh_cot_pencil_f64; host statement mesh_ops.cot_pencil.  Synchronises once (nnz and the status of phase 0).  When a
    vertex has more than SN_LAP_MAX_DEGREE incident faces the status carries DESC_DEGREE, nothing further is launched and
    colind, S and mass are None: there is no other path, the caller refuses."""
    _dev(V, F)
    _check_mesh("cot_pencil_from_mesh", V, F)
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    rowptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_cot_laplacian_workspace_bytes", dev, nV, nF)      # the pencil shares the query
    head = (_p(V), _p(F), nV, nF)
    _lib.call("sn_mesh_cot_pencil_f64", *head, 0, _p(rowptr), None, None, None, status.data_ptr(), _p(ws), ws_bytes, _stream())
    nnz, st = torch.cat([rowptr[-1:], status]).tolist()
    if st & DESC_DEGREE:
        return rowptr, None, None, None, st
    colind = torch.empty(nnz, dtype=torch.int32, device=dev)
    S = torch.empty(nnz, dtype=torch.float64, device=dev)
    mass = torch.empty(nV, dtype=torch.float64, device=dev)
    _lib.call("sn_mesh_cot_pencil_f64", *head, 1, _p(rowptr), _p(colind), _p(S), _p(mass), status.data_ptr(), _p(ws), ws_bytes,
              _stream())
    return rowptr, colind, S, mass, st


def _check_voff(who: str, voff) -> int:
    if voff.dtype != torch.int32 or voff.dim() != 1 or voff.numel() < 2 or not voff.is_contiguous():
        raise TypeError(f"{who} wants voff (B + 1,) int32, contiguous")
    return voff.numel() - 1


def spectral_start(seed: int, voff, n: int, m: int):
    """The (n, m) fp64 start block of the eigen-solver, a fixed function of (seed, row in its mesh, column)
    (sn_spectral_start_f64; host statement mesh_ops.spectral_start).  voff (B + 1,) int32 on the device, voff[B] = n."""
    _dev(voff)
    B = _check_voff("spectral_start", voff)
    if n < 0 or m < 1:
        raise ValueError(f"spectral_start: n >= 0 and m >= 1 are required, got {n} and {m}")
    X = torch.empty(n, m, dtype=torch.float64, device=voff.device)
    _lib.call("sn_spectral_start_f64", int(seed) & ((1 << 64) - 1), _p(voff), B, n, m, _p(X), _stream())
    return X


def cheb_filter_step(rowptr, colind, vals, voff, alpha, beta, shift, X, Y, out=None):
    """Z = alpha_b (A Y - shift_b Y) - beta_b X, one launch over a block-diagonal batch (sn_cheb_filter_step_f64; host statement
    mesh_ops.cheb_filter_step): A fp64 CSR with int32 rowptr / colind, X and Y (n, m) fp64, alpha / beta / shift (B,) fp64 on
    the device, b the mesh of a row through voff (B + 1,) int32.  out: where Z goes (a new tensor when None); it may be X, it
    must not be Y (SnError, SN_E_SHAPE).  Does not synchronise; two runs are bit-identical."""
    _dev(rowptr, colind, vals, voff, alpha, beta, shift, X, Y, out)
    n = rowptr.numel() - 1
    B = _check_voff("cheb_filter_step", voff)
    _check_graph("cheb_filter_step", rowptr, colind, n)
    Z = torch.empty_like(Y) if out is None else out
    for name, t in (("X", X), ("Y", Y), ("out", Z)):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape != Y.shape or not t.is_contiguous():
            raise TypeError(f"cheb_filter_step wants {name} (n, m) float64, contiguous, all of one shape; got {tuple(t.shape)} {t.dtype}")
    if Y.shape[0] != n or Y.shape[1] < 1:
        raise ValueError(f"cheb_filter_step: the matrix has {n} rows, the blocks are {tuple(Y.shape)}")
    if vals.dtype != torch.float64 or vals.shape != colind.shape or not vals.is_contiguous():
        raise TypeError("cheb_filter_step wants vals (nnz,) float64, contiguous")
    for name, t in (("alpha", alpha), ("beta", beta), ("shift", shift)):
        if t.dtype != torch.float64 or t.shape != (B,) or not t.is_contiguous():
            raise TypeError(f"cheb_filter_step wants {name} (B,) = ({B},) float64, contiguous")
    _lib.call("sn_cheb_filter_step_f64", _p(rowptr), _p(colind), _p(vals), _p(voff), B, n, Y.shape[1], _p(alpha), _p(beta), _p(shift),
              _p(X), _p(Y), _p(Z), _stream())
    return Z


def wks_contract(phi, voff, W, C, dtype=torch.float32):
    """WKS[v, i] = (sum_k phi[v, k]^2 W[b, k, i]) / C[b, i] (sn_wks_f64; host statement mesh_ops.wks_contract): phi (nV, k),
    W (B, k, N), C (B, N) fp64 on the device, b the mesh of vertex v through voff (B + 1,) int32.  Returns (nV, N) in dtype
    (torch.float32: the quotient rounded once, or torch.float64).  Does not synchronise; two runs are bit-identical."""
    _dev(phi, voff, W, C)
    nV = phi.shape[0]
    B = _check_voff("wks_contract", voff)
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("wks_contract returns torch.float32 or torch.float64")
    if phi.dtype != torch.float64 or phi.dim() != 2 or W.dtype != torch.float64 or W.dim() != 3 or C.dtype != torch.float64:
        raise TypeError("wks_contract wants phi (nV, k), W (B, k, N) and C (B, N) float64")
    k, N = phi.shape[1], W.shape[2]
    if W.shape != (B, k, N) or C.shape != (B, N) or k < 1 or N < 1:
        raise ValueError(f"wks_contract: phi {tuple(phi.shape)}, W {tuple(W.shape)} and C {tuple(C.shape)} do not fit {B} meshes")
    phi, W, C = phi.contiguous(), W.contiguous(), C.contiguous()
    out = torch.empty(nV, N, dtype=dtype, device=phi.device)
    _lib.call("sn_wks_f64", _p(phi), _p(voff), B, nV, k, N, _p(W), _p(C), int(dtype == torch.float32), _p(out), _stream())
    return out


def _check_graph(who: str, rowptr, colind, n: int) -> None:
    if rowptr.dtype != torch.int32 or colind.dtype != torch.int32:
        raise TypeError(f"{who} wants int32 rowptr and colind")
    if rowptr.dim() != 1 or colind.dim() != 1 or rowptr.numel() != n + 1:
        raise ValueError(f"{who}: rowptr must hold n + 1 = {n + 1} entries, got {tuple(rowptr.shape)}")
    if not (rowptr.is_contiguous() and colind.is_contiguous()):
        raise ValueError(f"{who} wants contiguous CSR arrays")


def edge_lengths_csr(V, rowptr, colind):
    """Euclidean length of every stored entry (i, colind[e]) of an n x n CSR pattern over the vertices V (n, 3) fp32:
    (float) sqrt((dx*dx + dy*dy) + dz*dz) in fp64 without fused multiply-add (sn_edge_lengths_csr_f32), numpy's value bit for bit."""
    _dev(V, rowptr, colind)
    if V.dtype != torch.float32 or V.dim() != 2 or V.shape[1] != 3:
        raise TypeError("edge_lengths_csr wants V (n, 3) float32")
    n = V.shape[0]
    _check_graph("edge_lengths_csr", rowptr, colind, n)
    V = V.contiguous()
    w = torch.empty(colind.numel(), dtype=torch.float32, device=V.device)
    _lib.call("sn_edge_lengths_csr_f32", _p(V), _p(rowptr), _p(colind), n, _p(w), _stream())
    return w


def graph_apsp_max_vertices() -> int:
    """The largest graph graph_apsp takes: one fp32 distance vector has to fit the LDS of a CU."""
    return int(_lib.load().sn_graph_apsp_max_vertices())


def graph_apsp(rowptr, colind, w, n: int, sources=None, out=None, sweeps=None):
    """Shortest-path distances along the edges of a CSR graph with fp32 weights w >= 0 (sn_graph_apsp_f32; the definition is
    in include/sn_spmm.h: path lengths accumulate in fp32 from the source outward, +inf where there is no path).
    sources: None = every vertex, or a range(begin, end) of consecutive sources; row k of the result belongs to source
    sources[k].  out: a (>= len(sources), >= n) float32 tensor with unit column stride to write into (its other elements are
    left alone), else a new (len(sources), n) tensor.  sweeps: an int32 tensor that takes the sweep count of every workgroup.
    Returns (D, unreached): unreached is a 1-element int32 device tensor, non-zero when a row holds +inf (not read here).
    Raises for n > graph_apsp_max_vertices(): there is no other path."""
    _dev(rowptr, colind, w, out, sweeps)
    n = int(n)
    _check_graph("graph_apsp", rowptr, colind, n)
    if w.dtype != torch.float32 or w.shape != colind.shape or not w.is_contiguous():
        raise TypeError("graph_apsp wants contiguous float32 weights, one per stored entry")
    if sources is None:
        sources = range(n)
    if not isinstance(sources, range) or sources.step != 1:
        raise TypeError("graph_apsp: sources must be None or a range of consecutive vertices")
    begin, count = (sources.start, len(sources)) if len(sources) else (0, 0)
    if begin < 0 or begin + count > n:
        raise ValueError(f"graph_apsp: sources {sources} outside 0..{n}")
    if n > graph_apsp_max_vertices():
        raise _lib.SnError(f"graph_apsp: {n} vertices, the kernel holds at most {graph_apsp_max_vertices()} "
                           "(one distance vector per LDS); there is no fallback")
    if _debug_validate() and w.numel() and not bool((w >= 0).all()):
        raise ValueError("graph_apsp: negative or NaN edge weight")
    if out is None:
        out = torch.empty(count, n, dtype=torch.float32, device=rowptr.device)
    elif out.dtype != torch.float32 or out.shape[0] < count or out.shape[1] < n:
        raise ValueError(f"graph_apsp: out must be float32 and at least ({count}, {n}), got {out.dtype} {tuple(out.shape)}")
    unreached = torch.zeros(1, dtype=torch.int32, device=rowptr.device)
    if sweeps is not None:
        groups = -(-count // max(int(_lib.load().sn_graph_apsp_group(n)), 1))
        if sweeps.dtype != torch.int32 or not sweeps.is_contiguous() or sweeps.numel() < groups:
            raise ValueError(f"graph_apsp: sweeps must be contiguous int32 with at least {groups} entries")
        _lib.call("sn_graph_apsp_sweeps_f32", _p(rowptr), _p(colind), _p(w), n, begin, count, _p(out), _ld(out), _p(unreached),
                  _p(sweeps), _stream())
    else:
        _lib.call("sn_graph_apsp_f32", _p(rowptr), _p(colind), _p(w), n, begin, count, _p(out), _ld(out), _p(unreached), _stream())
    return out, unreached


def symmetrize_min_(G, n: int = None):
    """In place G[i][j] = G[j][i] = min(G[i][j], G[j][i]) on the leading n x n block (default: all rows) of a float32 matrix
    with unit column stride (sn_symmetrize_min_f32: tile pairs through LDS, no second matrix).  Returns G."""
    _dev(G)
    if G.dtype != torch.float32 or G.dim() != 2:
        raise TypeError("symmetrize_min_ wants a 2-D float32 tensor")
    n = G.shape[0] if n is None else int(n)
    if n > G.shape[0] or n > G.shape[1]:
        raise ValueError(f"symmetrize_min_: n = {n} exceeds the matrix {tuple(G.shape)}")
    _lib.call("sn_symmetrize_min_f32", _p(G), n, _ld(G), _stream())
    return G


class MeshCorners:
    """Corner table of a triangle mesh (include/sn_spmm.h, "Geodesic distance matrices that cross triangles"): a CSR by
    vertex.  cptr: (n + 1,) int32; records: (3 * nF, 40) uint8, the first cptr[n] rows are written, one record per corner
    (v; a, b): int32 a, b; float l_a, l_b; double c, s_b, h."""

    def __init__(self, cptr, records):
        self.cptr, self.records = cptr, records

    @property
    def n(self) -> int:
        return self.cptr.numel() - 1


def _mesh_corner_table(V, F):
    """(MeshCorners, flag): flag is a 1-element int32 device tensor, 1 when a face was dropped (not read here)."""
    _dev(V, F)
    if V.dtype != torch.float32 or F.dtype != torch.int32 or V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise TypeError("mesh_corners wants V (nV, 3) float32 and F (nF, 3) int32")
    V, F = V.contiguous(), F.contiguous()
    nV, nF = V.shape[0], F.shape[0]
    dev = V.device
    cptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    records = torch.empty(3 * nF, MESH_CORNER_BYTES, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_corners_workspace_bytes", dev, nV)
    _lib.call("sn_mesh_corners_f32", _p(V), _p(F), nV, nF, _p(cptr), _p(records), _p(flag), _p(ws), ws_bytes, _stream())
    return MeshCorners(cptr, records), flag


def mesh_corners(V, F) -> MeshCorners:
    """Corner table of one mesh built on the device (sn_mesh_corners_f32): what mesh_geodesics sweeps over.  V: (nV, 3) fp32,
    F: (nF, 3) int32.  Synchronises once (reads the flag); a face with an index outside the mesh or a repeated index raises."""
    corners, flag = _mesh_corner_table(V, F)
    if int(flag.item()):
        raise _lib.SnError(f"mesh_corners: {constants.BAD_FACE_SENTENCE}")
    return corners


def mesh_geodesics(corners: MeshCorners, n: int, sources=None, out=None, sweeps=None):
    """Geodesic distances that cross triangles: first-order Eikonal sweeps over a corner table (sn_mesh_geodesics_f32; the
    definition is in include/sn_spmm.h).  sources / out / sweeps as graph_apsp.  Returns (D, flags): flags is a 1-element int32
    device tensor, bit 1 when a row holds +inf, bit 2 when a workgroup's n-th sweep still changed something (not read here).
    Raises for n > graph_apsp_max_vertices(): there is no other path."""
    _dev(corners.cptr, corners.records, out, sweeps)
    n = int(n)
    cptr, rec = corners.cptr, corners.records
    if cptr.dtype != torch.int32 or cptr.dim() != 1 or cptr.numel() != n + 1 or not cptr.is_contiguous():
        raise ValueError(f"mesh_geodesics: cptr must be contiguous int32 with n + 1 = {n + 1} entries, got {tuple(cptr.shape)}")
    if rec.dtype != torch.uint8 or rec.dim() != 2 or rec.shape[1] != MESH_CORNER_BYTES or not rec.is_contiguous():
        raise TypeError(f"mesh_geodesics wants contiguous (corners, {MESH_CORNER_BYTES}) uint8 records")
    if sources is None:
        sources = range(n)
    if not isinstance(sources, range) or sources.step != 1:
        raise TypeError("mesh_geodesics: sources must be None or a range of consecutive vertices")
    begin, count = (sources.start, len(sources)) if len(sources) else (0, 0)
    if begin < 0 or begin + count > n:
        raise ValueError(f"mesh_geodesics: sources {sources} outside 0..{n}")
    if n > graph_apsp_max_vertices():
        raise _lib.SnError(f"mesh_geodesics: {n} vertices, the kernel holds at most {graph_apsp_max_vertices()} "
                           "(one distance vector per LDS); there is no fallback")
    if out is None:
        out = torch.empty(count, n, dtype=torch.float32, device=cptr.device)
    elif out.dtype != torch.float32 or out.shape[0] < count or out.shape[1] < n:
        raise ValueError(f"mesh_geodesics: out must be float32 and at least ({count}, {n}), got {out.dtype} {tuple(out.shape)}")
    flags = torch.zeros(1, dtype=torch.int32, device=cptr.device)
    if sweeps is not None:
        groups = -(-count // max(int(_lib.load().sn_graph_apsp_group(n)), 1))
        if sweeps.dtype != torch.int32 or not sweeps.is_contiguous() or sweeps.numel() < groups:
            raise ValueError(f"mesh_geodesics: sweeps must be contiguous int32 with at least {groups} entries")
        _lib.call("sn_mesh_geodesics_sweeps_f32", _p(cptr), _p(rec), n, begin, count, _p(out), _ld(out), _p(flags), _p(sweeps), _stream())
    else:
        _lib.call("sn_mesh_geodesics_f32", _p(cptr), _p(rec), n, begin, count, _p(out), _ld(out), _p(flags), _stream())
    return out, flags


def _debug_validate() -> bool:
    from . import operators

    return operators._DEBUG_VALIDATE


_gemm_variant = None


def _split_gemm() -> bool:
    """True unless the process runs the fp32-MFMA A/B baseline of the Linear kernels (SN_GEMM_VARIANT=0) — asked of the library
    (sn_gemm_variant), which reads the switch once: the fused epilogues exist in the 16-bit matrix-pipe kernels only."""
    global _gemm_variant
    if _gemm_variant is None:
        _gemm_variant = int(_lib.load().sn_gemm_variant())
    return _gemm_variant != 0


def linear_fwd_supported(K: int, J: int) -> bool:
    """J = 128, or — split kernels only — any multiple of 4 up to 128 (the models' last layer has 120 outputs)."""
    return K in (128, 256) and (J == 128 or (_split_gemm() and 0 < J < 128 and J % 4 == 0))


def elu_stats_supported() -> bool:
    """Column statistics of the ELU output from the GEMM epilogue exist only in the 16-bit matrix-pipe kernels."""
    return _split_gemm()


def new_elu_stats_part(rows: int, device):
    """Workspace for the per-workgroup column sums / sums of squares of a forward GEMM's ELU output (128 columns)."""
    nblk = int(_lib.load().sn_linear_fwd_stats_blocks(rows))
    return torch.empty((max(nblk, 1), 2, 128), dtype=torch.float64, device=device)


def tile_sums_supported() -> bool:
    """The forward kernels can leave per-tile column sums of their ELU output (sn_linear_fwd_tiles_f32): split kernels only."""
    return elu_stats_supported()


def new_tile_sums(rows: int, device):
    """Buffer for the per-tile column sums of a forward GEMM's ELU output: ((rows + 31) // 32, 128) fp32."""
    return torch.empty(((rows + 31) // 32, 128), dtype=torch.float32, device=device)


def linear_small_rows() -> int:
    """Operands of at most this many rows take the Linear kernels' one-pass weight prologue (sn_linear_small_rows)."""
    return int(_lib.load().sn_linear_small_rows())


def linear_fwd_form(rows: int, K: int, J: int, residual: bool = False, want_y: bool = True, y_elu: bool = False,
                    tile_sums: bool = False) -> int:
    """The kernel form linear_fwd launches for these arguments (sn_linear_fwd_form): 0 the fp32-MFMA A/B baseline, 1 split with
    the one-pass weight prologue (small operand), 2 split with the two-pass prologue (large operand), 3 the eight-wave kernel."""
    return int(_lib.load().sn_linear_fwd_form(rows, K, J, int(bool(residual)), int(bool(want_y)), int(bool(y_elu)),
                                              int(bool(tile_sums))))


def linear_fwd(x, W, bias, residual=None, y_elu=None, want_y: bool = True, elu_stats=None, tile_sums=None):
    """y = x·Wᵀ + bias (+ residual); optionally also writes elu(y) into the 2-D view `y_elu` (sn_linear_fwd_f32).
    want_y=False (with y_elu): only the activated copy is written and None is returned.
    elu_stats (from new_elu_stats_part): receives the column statistics of elu(y), see colstats_halves.
    tile_sums (from new_tile_sums, with elu_stats): receives the column sums of elu(y) per 32-row tile (avg_stats_from_tiles)."""
    _dev(x, W, bias, residual, y_elu, elu_stats, tile_sums)
    rows, K = x.shape
    J = W.shape[0]
    # (the fp32-MFMA A/B kernels, SN_GEMM_VARIANT=0, always write y)
    keep = want_y or y_elu is None
    y = torch.empty((rows, J), dtype=torch.float32, device=x.device) if (keep or not elu_stats_supported()) else None
    _lib.call("sn_linear_fwd_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), _p(residual),
              _ld(residual) if residual is not None else 0, _p(y), J, _p(y_elu), _ld(y_elu) if y_elu is not None else 0,
              rows, K, J, _p(elu_stats), _p(tile_sums), _stream())
    return y if keep else None


def linear_fwd_frame_supported(K: int, J: int) -> bool:
    """linear_fwd_frame covers a K -> J layer: J/3 frames of 3 coordinates, J a multiple of 12 (split kernels only)."""
    return bool(_lib.load().sn_linear_fwd_frame_supported(int(K), int(J)))


def linear_fwd_frame(x, W, bias, frame):
    """y[r, 3t + c] = (x·Wᵀ + bias)[r, 3t + c] + frame[r, c]: linear_fwd's plain launch with the per-row frame (a (rows, 3) view of
    any row stride, 4-byte aligned) added in the store — the bits of linear_fwd followed by the broadcast add
    (sn_linear_fwd_frame_f32)."""
    _dev(x, W, bias, frame)
    rows, K = x.shape
    J = W.shape[0]
    if frame.shape != (rows, 3) or frame.dtype != torch.float32:
        raise ValueError(f"linear_fwd_frame: frame must be a ({rows}, 3) float32 view, got {tuple(frame.shape)} {frame.dtype}")
    y = torch.empty((rows, J), dtype=torch.float32, device=x.device)
    _lib.call("sn_linear_fwd_frame_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), _p(frame), _ld(frame), _p(y), J, rows, K, J, _stream())
    return y


def avg_stats_from_tiles(tile_sums, part, e, mask, inv_count, rows_per_seg: int, nseg: int):
    """(m, stats) of avg_stats WITHOUT a pass over e: from the per-tile column sums and the statistics partials the GEMM that
    wrote e left (sn_avg_stats_from_tiles_f32)."""
    _dev(tile_sums, part, e, mask, inv_count)
    rows, C = e.shape
    if tile_sums.shape != ((rows + 31) // 32, 128) or part.dim() != 3 or part.shape[1:] != (2, 128) or part.dtype != torch.float64:
        raise ValueError("avg_stats_from_tiles: tile sums / statistics partials of another operand")
    nblk = int(_lib.load().sn_linear_fwd_stats_blocks(rows))
    if part.shape[0] < nblk:
        raise ValueError("avg_stats_from_tiles: partial buffer smaller than the producing launch's grid")
    m = torch.empty((nseg, C), dtype=torch.float32, device=e.device)
    stats = torch.empty((2, 2 * C), dtype=torch.float64, device=e.device)
    ws = torch.empty((nseg, C), dtype=torch.float32, device=e.device)
    _lib.call("sn_avg_stats_from_tiles_f32", _p(tile_sums), _p(part), nblk, _p(e), _ld(e), _p(mask), _p(inv_count.contiguous()),
              rows_per_seg, nseg, C, _p(m), _p(stats), _p(ws), _stream())
    return m, stats


def avg_stats_from_tiles_ragged(tile_sums, part, e, seg):
    """(m, stats) of a global-average stage on a packed batch WITHOUT a pass over e (sn_avg_stats_from_tiles_ragged_f32): from the
    per-tile column sums and the statistics partials the GEMM that wrote e left; seg = operators.PackedSegments."""
    _dev(tile_sums, part, e)
    rows, C = e.shape
    if tile_sums.shape != ((rows + 31) // 32, 128) or part.dim() != 3 or part.shape[1:] != (2, 128) or part.dtype != torch.float64:
        raise ValueError("avg_stats_from_tiles_ragged: tile sums / statistics partials of another operand")
    nblk = int(_lib.load().sn_linear_fwd_stats_blocks(rows))
    if part.shape[0] < nblk or seg.rows != rows:
        raise ValueError("avg_stats_from_tiles_ragged: partial buffer smaller than the producing launch's grid / another batch")
    m = torch.empty((seg.nseg, C), dtype=torch.float32, device=e.device)
    stats = torch.empty((2, 2 * C), dtype=torch.float64, device=e.device)
    ws = torch.empty((seg.nseg, C), dtype=torch.float32, device=e.device)
    _lib.call("sn_avg_stats_from_tiles_ragged_f32", _p(tile_sums), _p(part), nblk, _p(e), _ld(e), _p(seg.off_dev), _p(seg.inv_count),
              seg.nseg, C, _p(m), _p(stats), _p(ws), _stream())
    return m, stats


def colstats_from_part(part, rows: int):
    """(2, 128) float64 statistics of a forward GEMM's ELU output from the partials it left (sn_colstats_merge_f64)."""
    _dev(part)
    if part.dim() != 3 or part.shape[1:] != (2, 128) or part.dtype != torch.float64:
        raise ValueError("colstats_from_part: expected (nblk, 2, 128) float64 partials")
    nblk = int(_lib.load().sn_linear_fwd_stats_blocks(rows))
    if part.shape[0] < nblk:
        raise ValueError("colstats_from_part: partial buffer smaller than the producing launch's grid")
    out = torch.empty((2, 128), dtype=torch.float64, device=part.device)
    _lib.call("sn_colstats_merge_f64", _p(part), nblk, 128, _p(out), 128, 0, _stream())
    return out


def colstats_merge_into(part, out, offset: int) -> None:
    """Combine (nblk, 2, C) float64 partials into columns offset .. offset+C of the (2, width) statistics tensor `out`
    (sn_colstats_merge_f64)."""
    _dev(part, out)
    C = part.shape[2]
    if part.dim() != 3 or part.shape[1] != 2 or part.dtype != torch.float64 or out.dtype != torch.float64 or \
            not out.is_contiguous() or offset + C > out.shape[1]:
        raise ValueError("colstats_merge_into: (nblk, 2, C) float64 partials into a contiguous (2, width >= offset + C) tensor")
    _lib.call("sn_colstats_merge_f64", _p(part), int(part.shape[0]), C, _p(out), out.shape[1], offset, _stream())


def colstats_into(x, out, offset: int):
    """Column sums / sums of squares of the 2-D view x written into columns offset .. offset+C of the (2, width) float64
    statistics tensor `out` (sn_colstats_into_f32)."""
    _dev(x, out)
    rows, C = x.shape
    if out.dim() != 2 or out.shape[0] != 2 or out.dtype != torch.float64 or not out.is_contiguous() or offset + C > out.shape[1]:
        raise ValueError("colstats_into: out must be a contiguous (2, width) float64 tensor with width >= offset + C")
    ws, ws_bytes = _workspace("sn_colstats_workspace_bytes", x.device, rows, C)
    _lib.call("sn_colstats_into_f32", _p(x), _ld(x), rows, C, _p(out), out.shape[1], offset, _p(ws), ws_bytes, _stream())
    return out


def colstats_halves(x, part, part_hi=None):
    """(2, 2C) float64 statistics of a stage's concat buffer x = [e | P·e] (rows, 2C), C = 128 or 64: the first half from the
    partials `part` the GEMM that wrote e left behind ((nblk, 2, 128) in the kernel's 128-column layout, of which the first C
    count); the second half from the partials `part_hi` ((nb, 2, C)) of the SpMM that wrote P·e (spmm_q3_stats) or, without
    them, from one pass over x[:, C:] only (sn_colstats_into_f32).  part=None: the first half by a pass over x[:, :C]."""
    _dev(x, part, part_hi)
    rows, C2 = x.shape
    C = C2 // 2
    if part is not None and (C not in (64, 128) or part.dim() != 3 or part.shape[1:] != (2, 128) or part.dtype != torch.float64):
        raise ValueError("colstats_halves: expected a (rows, 256 | 128) buffer and (nblk, 2, 128) float64 GEMM partials")
    if part_hi is not None and (C not in (64, 128) or part_hi.dim() != 3 or part_hi.shape[1:] != (2, C) or part_hi.dtype != torch.float64):
        raise ValueError("colstats_halves: expected (nb, 2, C) float64 partials for the propagated half")
    lib = _lib.load()
    out = torch.empty((2, C2), dtype=torch.float64, device=x.device)
    nlo = int(lib.sn_linear_fwd_stats_blocks(rows)) if part is not None else 0
    if part is not None and part.shape[0] < nlo:
        raise ValueError("colstats_halves: partial buffer smaller than the producing launch's grid")
    if part is not None and part_hi is not None:            # both producers left partials: one launch for the two halves
        _lib.call("sn_colstats_merge2_f64", _p(part), nlo, C, 128, _p(part_hi), int(part_hi.shape[0]), C, C, _p(out), _stream())
        return out
    for half, p_ in ((0, part), (1, part_hi)):
        if p_ is not None and (half == 1 or C == 128):
            nb = nlo if half == 0 else int(p_.shape[0])
            _lib.call("sn_colstats_merge_f64", _p(p_), nb, C, _p(out), C2, half * C, _stream())
        elif p_ is not None:                                 # (GEMM partials of a 64-channel half are read by the two-source launch only)
            raise ValueError("colstats_halves: 64-channel GEMM partials need the SpMM's partials too")
        else:
            xs = x[:, half * C:(half + 1) * C]
            ws, ws_bytes = _workspace("sn_colstats_workspace_bytes", x.device, rows, C)
            _lib.call("sn_colstats_into_f32", _p(xs), _ld(xs), rows, C, _p(out), C2, half * C, _p(ws), ws_bytes, _stream())
    return out


def linear_dgrad_supported(J: int, C: int) -> bool:
    return C in (128, 256) and (J == 128 or (_split_gemm() and 0 < J < 128 and J % 4 == 0))


def linear_dgrad_elu_supported(J: int, C: int) -> bool:
    """The fused form exists only in the 16-bit matrix-pipe kernels (SN_GEMM_VARIANT != 0)."""
    return 0 < J <= 128 and J % 4 == 0 and C in (128, 256) and _split_gemm()


def linear_dgrad_elu(dy, W, x, center, B, Cc, gadd=None):
    """Input gradient of the folded BatchNorm+Linear whose operand x is a stage's concat buffer [e | P·e]
    (sn_linear_dgrad_elu_f32): returns (dx_hi, gact) with dx_hi = dx[:, C/2:] and gact = dx[:, :C/2] * elu'(e) + gadd."""
    _dev(dy, W, x, center, B, Cc, gadd)
    rows, J = dy.shape
    C = W.shape[1]
    h = C // 2
    dx_hi = torch.empty((rows, h), dtype=torch.float32, device=dy.device)
    gact = torch.empty((rows, h), dtype=torch.float32, device=dy.device)
    am = _new_dgrad_absmax(dy.device)
    _lib.call("sn_linear_dgrad_elu_absmax_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(center), _p(B), _p(Cc),
              _p(dx_hi), h, _p(gact), h, _p(gadd), _ld(gadd) if gadd is not None else 0, rows, J, C, _p(am), _stream())
    note_absmax(gact, am)                # gact is the dy operand of the layer below
    return dx_hi, gact


def linear_dgrad_elu_raw(dy, W, x, center, B, Cc):
    """As linear_dgrad_elu without gadd, but the low half leaves RAW (sn_linear_dgrad_elu_rawlow_f32): returns (dx_hi, graw),
    graw = dy·W[:, :C/2], and x[:, :C/2] is not read.  The caller hands (center[:C/2], B[:C/2], Cc[:C/2]) to the consumer of
    graw (note_tail); no maxima are left for it."""
    _dev(dy, W, x, center, B, Cc)
    rows, J = dy.shape
    C = W.shape[1]
    h = C // 2
    dx_hi = torch.empty((rows, h), dtype=torch.float32, device=dy.device)
    graw = torch.empty((rows, h), dtype=torch.float32, device=dy.device)
    _lib.call("sn_linear_dgrad_elu_rawlow_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(center), _p(B), _p(Cc),
              _p(dx_hi), h, _p(graw), h, rows, J, C, _stream())
    return dx_hi, graw


def _new_dgrad_absmax(device):
    """Buffer for the per-workgroup maxima an input-gradient launch leaves (None when the two-piece weight gradient is off)."""
    if not absmax_wanted():
        return None
    return torch.empty(int(_lib.load().sn_linear_dgrad_absmax_blocks()), dtype=torch.float32, device=device)


def linear_dgrad(dy, W, x=None, center=None, B=None, Cc=None):
    """dx = dy·W (+ (x - center)*B + Cc): input gradient of the folded BatchNorm+Linear (sn_linear_dgrad_f32)."""
    _dev(dy, W, x, center, B, Cc)
    rows, J = dy.shape
    C = W.shape[1]
    dx = torch.empty((rows, C), dtype=torch.float32, device=dy.device)
    _lib.call("sn_linear_dgrad_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x) if x is not None else 0, _p(center),
              _p(B), _p(Cc), _p(dx), C, rows, J, C, _stream())
    return dx


# ---- half-width global-average stage (see include/sn_spmm.h) ----------------------------------------------------------
def avg_stage_supported(C: int, J: int, rows_per_seg: int) -> bool:
    return C == 128 and J == 128 and rows_per_seg >= 32 and _split_gemm()


def avg_fwd_prep(segsum, inv_count, rows_per_seg: int, stats1):
    """(m (nseg, C) fp32, stats (2, 2C) fp64): per-mesh mean and the BatchNorm statistics of [e | mean broadcast]."""
    _dev(segsum, inv_count, stats1)
    nseg, C = segsum.shape
    m = torch.empty((nseg, C), dtype=torch.float32, device=segsum.device)
    stats = torch.empty((2, 2 * C), dtype=torch.float64, device=segsum.device)
    _lib.call("sn_avg_fwd_prep_f32", _p(segsum), _p(inv_count.contiguous()), nseg, C, rows_per_seg, _p(stats1), _p(m), _p(stats),
              _stream())
    return m, stats


def avg_stats(e, mask, inv_count, rows_per_seg: int, nseg: int):
    """(m, stats) of avg_fwd_prep from ONE pass over e (sn_avg_stats_f32)."""
    _dev(e, mask, inv_count)
    C = e.shape[1]
    m = torch.empty((nseg, C), dtype=torch.float32, device=e.device)
    stats = torch.empty((2, 2 * C), dtype=torch.float64, device=e.device)
    ws, ws_bytes = _workspace("sn_avg_stats_workspace_bytes", e.device, rows_per_seg, nseg, C)
    _lib.call("sn_avg_stats_f32", _p(e), _ld(e), _p(mask), _p(inv_count.contiguous()), rows_per_seg, nseg, C, _p(m), _p(stats),
              _p(ws), ws_bytes, _stream())
    return m, stats


def seg_affine(A, W, bias):
    """out[g, j] = bias[j] + sum_c A[g, c] * W[j, c]; W may be a column slice (row stride kept)."""
    _dev(A, W, bias)
    nseg, K = A.shape
    J = W.shape[0]
    out = torch.empty((nseg, J), dtype=torch.float32, device=A.device)
    _lib.call("sn_seg_affine_f32", _p(A), nseg, K, _p(W), _ld(W), _p(bias), J, _p(out), _stream())
    return out


def avg_stats_ragged(m, seg, part, nblk: int):
    """(2, 2C) float64 BatchNorm statistics of [e | per-mesh mean broadcast] on a packed batch (sn_avg_prep_ragged_f32): m (nseg, C)
    the per-mesh means, seg = operators.PackedSegments, part the (>= nblk, 2, C) float64 statistics partials of e (ready (2, C)
    statistics: pass them as one block)."""
    _dev(m, part)
    nseg, C = m.shape
    if part.dtype != torch.float64 or part.shape[-1] != C or not part.is_contiguous() or not m.is_contiguous():
        raise ValueError("avg_stats_ragged: float64 partials (nblk, 2, C) and contiguous means (nseg, C)")
    stats = torch.empty((2, 2 * C), dtype=torch.float64, device=m.device)
    _lib.call("sn_avg_prep_ragged_f32", _p(m), _p(seg.off_dev), nseg, C, _p(part), nblk, _p(stats), _stream())
    return stats


AVG_BWD_MERGE_MAX = 32        # meshes up to which a global-average stage's backward trio runs as one launch (A/B below)


def avg_merged_supported(J: int, C: int, nseg: int, which: int = 1) -> bool:
    """Shapes for which a global-average stage folds its per-mesh bias into the fold launch (bn_fold_seg, which = 1) / runs gc +
    coefficients + per-mesh vector of its backward as one launch (avg_bn_bwd, which = 2).

    The merged launches run per-channel (backward) / per-output-row (forward) work that the separate kernels spread over many
    more workgroups: they win while the per-mesh algebra is small.  Forward: up to 64 meshes (round 4: config-3 step 18.94 ->
    18.89 ms).  Backward: round 4's kernel lost beyond 8 meshes (57 us at 64 against 19.7 us for the three launches); round 6
    found why — a branch per row serialised its LDS reads and its operand loads, one workgroup per channel block walked every
    mesh's dot product — and the kernel now costs 10 us at one mesh (15), 21 us at 64: same-box config-3 steps 6.84 -> 6.79 ms at
    16 meshes, 10.97 -> 10.94 at 32, FAUST pair replayed 3.39 -> 3.28 ms.  At 64 meshes the one launch (21.0 us) and the three
    (19.6 us) are level within the noise of a step (19.26 / 19.25 ms) and the trace puts the three 1.3 us ahead per stage: the
    limit stays at 32."""
    from . import kernels as _self      # (the limit is read through the module so that tests / tools can move it)

    lim = 64 if which == 1 else _self.AVG_BWD_MERGE_MAX
    return J <= 128 and C % 32 == 0 and 2 * C <= 256 and 0 < nseg <= lim


def bn_fold_seg(stats, rows: int, gamma, beta, W, b, eps: float, momentum: float, running_mean, running_var, m, num_batches_tracked=None):
    """bn_fold (training mode) of a global-average stage's 2C-wide layer and its per-mesh bias m·Wf[:, C:]ᵀ + bf in one launch
    (sn_bn_fold_seg_f32).  Returns (mean, invstd, s, t, Wf, bf, segbias (nseg, J))."""
    _dev(stats, gamma, beta, W, b, running_mean, running_var, num_batches_tracked, m)
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise TypeError("num_batches_tracked must be int64")
    J, C = W.shape
    nseg = m.shape[0]
    if m.shape[1] * 2 != C or not m.is_contiguous():
        raise ValueError("bn_fold_seg: per-mesh means of half the layer's width, contiguous")
    dev = W.device
    vec = torch.empty((4, C), dtype=torch.float32, device=dev)
    Wf = torch.empty((J, C), dtype=torch.float32, device=dev)
    bf = torch.empty(J, dtype=torch.float32, device=dev)
    segb = torch.empty((nseg, J), dtype=torch.float32, device=dev)
    _lib.call("sn_bn_fold_seg_f32", _p(stats), rows, _p(gamma), _p(beta), _p(W.contiguous()), _p(b), J, C, float(eps), float(momentum),
              _p(running_mean), _p(running_var), _p(vec[0]), _p(vec[1]), _p(vec[2]), _p(vec[3]), _p(Wf), _p(bf),
              _p(num_batches_tracked), _p(m), nseg, _p(segb), _stream())
    return vec[0], vec[1], vec[2], vec[3], Wf, bf, segb


def avg_bn_bwd(G1, dystats, seg_dy, m, mu2, W, s, invstd, beta, rows: int, has_bias: bool, Wf2, inv_count, rows_per_seg: int = 0,
               segoff=None):
    """(dW, db, dgamma, dbeta, Bc, Cc, segvec) of a global-average stage's backward from the first half's weight gradient G1, the
    column sums of dy and their per-mesh parts: avg_bwd_gc + bn_bwd_coeffs + avg_bwd_segvec[_ragged] in one launch
    (sn_avg_bn_bwd_f32; segoff: the row offsets of ragged meshes)."""
    _dev(G1, dystats, seg_dy, m, mu2, W, s, invstd, beta, Wf2, inv_count, segoff)
    J, C = G1.shape
    nseg = m.shape[0]
    dev = W.device
    dW = torch.empty((J, 2 * C), dtype=torch.float32, device=dev)
    db = torch.empty(J, dtype=torch.float32, device=dev) if has_bias else None
    vec = torch.empty((4, 2 * C), dtype=torch.float32, device=dev)
    segvec = torch.empty((nseg, C), dtype=torch.float32, device=dev)
    _lib.call("sn_avg_bn_bwd_f32", _p(G1), _p(dystats), _p(seg_dy), _p(m), _p(mu2), _p(W.contiguous()), _p(s), _p(invstd),
              _p(beta.contiguous()), rows, J, C, nseg, _p(Wf2), _ld(Wf2), _p(inv_count.contiguous()), rows_per_seg, _p(segoff),
              _p(dW), _p(db), _p(vec[0]), _p(vec[1]), _p(vec[2]), _p(vec[3]), _p(segvec), _stream())
    return dW, db, vec[0], vec[1], vec[2], vec[3], segvec


def avg_bwd_gc(G1, seg_dy, m, mu2):
    _dev(G1, seg_dy, m, mu2)
    J, C = G1.shape
    Gc = torch.empty((J, 2 * C), dtype=torch.float32, device=G1.device)
    _lib.call("sn_avg_bwd_gc_f32", _p(G1), _p(seg_dy), _p(m), _p(mu2), m.shape[0], J, C, _p(Gc), _stream())
    return Gc


def avg_bwd_segvec(seg_dy, Wf2, m, mu2, B2, C2, inv_count, rows_per_seg: int):
    _dev(seg_dy, Wf2, m, mu2, B2, C2, inv_count)
    nseg, C = m.shape
    J = seg_dy.shape[1]
    out = torch.empty((nseg, C), dtype=torch.float32, device=m.device)
    _lib.call("sn_avg_bwd_segvec_f32", _p(seg_dy), _p(Wf2), _ld(Wf2), _p(m), _p(mu2), _p(B2), _p(C2), _p(inv_count.contiguous()),
              rows_per_seg, nseg, J, C, _p(out), _stream())
    return out


def wgrad_seg(dy, x, center, rows_per_seg: int, bounds=None):
    """(G, colsum(dy) fp64, per-mesh colsum(dy) (nseg, J) fp32) in one pass (sn_wgrad_seg_f32; bounds: as kernels.wgrad)."""
    _dev(dy, x, center)
    rows, J = dy.shape
    C = x.shape[1]
    nseg = rows // rows_per_seg
    dev = dy.device
    G = torch.empty((J, C), dtype=torch.float32, device=dev)
    dysum = torch.empty(J, dtype=torch.float64, device=dev)
    seg = torch.empty((nseg, J), dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace("sn_wgrad_seg_workspace_bytes", dev, rows, rows_per_seg, J, C)
    if bounds is not None:
        _lib.call("sn_wgrad_seg_bounded_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(center), rows, rows_per_seg, J, C, _p(G), _p(dysum),
                  _p(seg), _p(ws), ws_bytes, *_bounds_args(bounds, C), _stream())
    else:
        _lib.call("sn_wgrad_seg_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(center), rows, rows_per_seg, J, C, _p(G), _p(dysum), _p(seg),
                  _p(ws), ws_bytes, _stream())
    return G, dysum, seg


def wgrad_slabs(dy, x, center, seg, bounds=None):
    """wgrad_seg for RAGGED meshes (`seg`: operators.PackedSegments): (G, colsum(dy) fp64, per-mesh colsum(dy) (nseg, J))
    from one pass, the row slabs taken from seg's table (sn_wgrad_slabs_f32)."""
    _dev(dy, x, center)
    rows, J = dy.shape
    C = x.shape[1]
    dev = dy.device
    G = torch.empty((J, C), dtype=torch.float32, device=dev)
    dysum = torch.empty(J, dtype=torch.float64, device=dev)
    segsum = torch.empty((seg.nseg, J), dtype=torch.float32, device=dev)
    ws_bytes = seg.nslab * 128 * (C + 1) * 4
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if bounds is not None:
        _lib.call("sn_wgrad_slabs_bounded_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(center), rows, _p(seg.slab_off), seg.nslab,
                  _p(seg.seg_slab_ptr), seg.nseg, J, C, _p(G), _p(dysum), _p(segsum), _p(ws), ws_bytes, *_bounds_args(bounds, C),
                  _stream())
    else:
        _lib.call("sn_wgrad_slabs_f32", _p(dy), _ld(dy), _p(x), _ld(x), _p(center), rows, _p(seg.slab_off), seg.nslab,
                  _p(seg.seg_slab_ptr), seg.nseg, J, C, _p(G), _p(dysum), _p(segsum), _p(ws), ws_bytes, _stream())
    return G, dysum, segsum


def avg_bwd_segvec_ragged(seg_dy, Wf2, m, mu2, B2, C2, seg):
    _dev(seg_dy, Wf2, m, mu2, B2, C2)
    nseg, C = m.shape
    J = seg_dy.shape[1]
    out = torch.empty((nseg, C), dtype=torch.float32, device=m.device)
    _lib.call("sn_avg_bwd_segvec_ragged_f32", _p(seg_dy), _p(Wf2), _ld(Wf2), _p(m), _p(mu2), _p(B2), _p(C2), _p(seg.inv_count),
              _p(seg.off_dev), nseg, J, C, _p(out), _stream())
    return out


def linear_fwd_segbias_ragged(x, W, segbias, seg, residual=None, y_elu=None, want_y: bool = True, elu_stats=None, tile_sums=None):
    """linear_fwd_segbias with the bias row of each RAGGED mesh (`seg`: operators.PackedSegments); tile_sums: as linear_fwd."""
    _dev(x, W, segbias, residual, y_elu, tile_sums)
    rows, K = x.shape
    J = W.shape[0]
    y = torch.empty((rows, J), dtype=torch.float32, device=x.device) if want_y else None
    _lib.call("sn_linear_fwd_segbias_ragged_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(segbias), _p(seg.off_dev), seg.nseg,
              _p(residual), _ld(residual) if residual is not None else 0, _p(y), J, _p(y_elu),
              _ld(y_elu) if y_elu is not None else 0, rows, K, J, _p(elu_stats), _p(tile_sums), _stream())
    return y


def linear_dgrad_eluseg_ragged(dy, W, x, center, B, Cc, segvec, seg, gadd=None):
    """linear_dgrad_eluseg with the vector of each RAGGED mesh, no row mask (a packed batch has no padding rows)."""
    _dev(dy, W, x, center, B, Cc, segvec, gadd)
    rows, J = dy.shape
    C = x.shape[1]
    gact = torch.empty((rows, C), dtype=torch.float32, device=dy.device)
    am = _new_dgrad_absmax(dy.device)
    _lib.call("sn_linear_dgrad_eluseg_ragged_absmax_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(center), _p(B), _p(Cc),
              _p(segvec), _p(seg.off_dev), seg.nseg, _p(gact), C, _p(gadd), _ld(gadd) if gadd is not None else 0, rows, J, C,
              _p(am), _stream())
    note_absmax(gact, am)
    return gact


def avg_stage_ragged_supported(C: int, J: int, seg) -> bool:
    return C == 128 and J == 128 and seg.min_len >= 32 and _split_gemm()


def wgrad_thin_supported(J: int, C: int) -> bool:
    return 1 <= C <= 8 and J % 4 == 0 and 256 % (J // 4) == 0


def linear_thin_fwd(x, W, bias, y_elu=None):
    """y = x·W^T + bias for 1..8 input channels; optionally elu(y) into the 2-D view y_elu (sn_linear_thin_fwd_f32)."""
    _dev(x, W, bias, y_elu)
    rows, C = x.shape
    J = W.shape[0]
    y = torch.empty((rows, J), dtype=torch.float32, device=x.device)
    _lib.call("sn_linear_thin_fwd_f32", _p(x), _ld(x), _p(W), _ld(W), _p(bias), rows, C, J, _p(y), J, _p(y_elu),
              _ld(y_elu) if y_elu is not None else 0, _stream())
    return y


def wgrad_thin(dy, x, want_bias: bool = True):
    """(dW (J, C), db (J) | None) of a Linear with 1..8 input channels: dy^T x and colsum(dy) in one pass (sn_wgrad_thin_f32)."""
    _dev(dy, x)
    rows, J = dy.shape
    C = x.shape[1]
    dev = dy.device
    G = torch.empty((J, C), dtype=torch.float32, device=dev)
    db = torch.empty(J, dtype=torch.float32, device=dev) if want_bias else None
    ws, ws_bytes = _workspace("sn_wgrad_thin_workspace_bytes", dev, rows, J, C)
    _lib.call("sn_wgrad_thin_f32", _p(dy), _ld(dy), _p(x), _ld(x), rows, J, C, _p(G), _p(db), _p(ws), ws_bytes, _stream())
    return G, db


def gather_segments(src, base, rows_per_item: int, row_stride: int, length: int):
    """(nitems, rows_per_item, length) fp32: row r of item i = src.flatten()[base[i] + r*row_stride : ... + length]
    (sn_gather_segments_f32); base: int64 device tensor of element offsets into the contiguous src."""
    _dev(src, base)
    if not src.is_contiguous() or src.dtype != torch.float32 or base.dtype != torch.int64:
        raise TypeError("gather_segments: contiguous float32 source and int64 offsets expected")
    n = base.numel()
    out = torch.empty((n, rows_per_item, length), dtype=torch.float32, device=src.device)
    _lib.call("sn_gather_segments_f32", _p(src), _p(base.contiguous()), n, rows_per_item, row_stride, length, _p(out), _stream())
    return out


def gather_segments_ragged(src, base, seg, row_stride: int, length: int):
    """(seg.rows, length) fp32: the packed counterpart of gather_segments — item i supplies its first len_i rows, stored at the
    rows of mesh i of the packed batch `seg` (operators.PackedSegments); sn_gather_segments_ragged_f32."""
    _dev(src, base)
    if not src.is_contiguous() or src.dtype != torch.float32 or base.dtype != torch.int64 or base.numel() != seg.nseg:
        raise TypeError("gather_segments_ragged: contiguous float32 source and one int64 offset per mesh expected")
    out = torch.empty((seg.rows, length), dtype=torch.float32, device=src.device)
    _lib.call("sn_gather_segments_ragged_f32", _p(src), _p(base.contiguous()), _p(seg.off_dev), seg.nseg, seg.rows, row_stride, length,
              _p(out), _stream())
    return out


def pair_argmin(GA, pa, GB, pb):
    """argmin_j (GA[r, pa[j]] + GB[pb[r], j]) for every r (sn_pair_argmin_f32): the target of the dense-correspondence
    loss, main.py:236-237, without the two gathered (NA, NB) matrices.  GA, GB: row-major fp32 matrices; pa (NB,), pb (NA,)
    int64.  Returns (NA,) int64."""
    _dev(GA, pa, GB, pb)
    if GA.dtype != torch.float32 or GB.dtype != torch.float32 or pa.dtype != torch.int64 or pb.dtype != torch.int64:
        raise TypeError("pair_argmin: float32 matrices and int64 index vectors expected")
    if GA.dim() != 2 or GB.dim() != 2 or GA.stride(1) != 1 or GB.stride(1) != 1:
        raise ValueError("pair_argmin: row-major 2-D matrices expected")
    NA, NB = pb.numel(), pa.numel()
    if NA > GA.shape[0] or NB > GB.shape[1]:
        raise ValueError("pair_argmin: more rows / columns asked for than the matrices hold")
    out = torch.empty(NA, dtype=torch.int64, device=GA.device)
    _lib.call("sn_pair_argmin_f32", _p(GA), GA.stride(0), GA.shape[1], _p(pa.contiguous()), _p(GB), GB.stride(0), _p(pb.contiguous()), NA, NB,
              _p(out), _stream())
    return out


def pair_ce_fwd(S, target, NA: int, NB: int):
    """(lse, rowloss), NA floats each, of the cross entropy over S[:NA, :NB] (sn_pair_ce_fwd_f32; main.py:238-239)."""
    _dev(S, target)
    if S.dtype != torch.float32 or target.dtype != torch.int64 or S.dim() != 2 or S.stride(1) != 1:
        raise TypeError("pair_ce_fwd: row-major float32 scores and int64 targets expected")
    if NA > S.shape[0] or NB > S.shape[1] or target.numel() != NA:
        raise ValueError("pair_ce_fwd: NA x NB does not fit the score matrix / target vector")
    lse = torch.empty(NA, dtype=torch.float32, device=S.device)
    rowloss = torch.empty(NA, dtype=torch.float32, device=S.device)
    _lib.call("sn_pair_ce_fwd_f32", _p(S), S.stride(0), _p(target.contiguous()), NA, NB, _p(lse), _p(rowloss), _stream())
    return lse, rowloss


def pair_ce_bwd(S, target, lse, gloss, NA: int, NB: int):
    """Gradient of mean_r rowloss[r] times the device scalar gloss, for the WHOLE score matrix (zeros outside NA x NB)."""
    _dev(S, target, lse, gloss)
    dS = torch.empty((S.shape[0], S.shape[1]), dtype=torch.float32, device=S.device)
    _lib.call("sn_pair_ce_bwd_f32", _p(S), S.stride(0), _p(target.contiguous()), _p(lse), _p(gloss), NA, NB, S.shape[0], S.shape[1],
              _p(dS), dS.stride(0), _stream())
    return dS


def pair_fused_fwd(FA, FB, target, NA: int, NB: int):
    """(lse, rowloss, workspace) of the correspondence cross entropy computed from the tower features FA (rowsA x K), FB
    (rowsB x K): the scores FA·FBᵀ (models.py:203) are formed tile by tile on the matrix pipe and never written
    (sn_pair_fused_fwd_f32).  `workspace` holds the split features for pair_fused_bwd."""
    _dev(FA, FB, target)
    for t in (FA, FB):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise TypeError("pair_fused_fwd: row-major float32 feature matrices expected")
    if target.dtype != torch.int64 or FA.shape[1] != FB.shape[1]:
        raise TypeError("pair_fused_fwd: int64 targets and features of one width expected")
    if not (0 < NA <= FA.shape[0] and 0 < NB <= FB.shape[0]) or target.numel() != NA:
        raise ValueError("pair_fused_fwd: NA / NB do not fit the feature matrices / target vector")
    ws, nbytes = _workspace("sn_pair_fused_workspace_bytes", FA.device, FA.shape[0], FB.shape[0], least=0)
    lse = torch.empty(NA, dtype=torch.float32, device=FA.device)
    rowloss = torch.empty(NA, dtype=torch.float32, device=FA.device)
    _lib.call("sn_pair_fused_fwd_f32", _p(FA), FA.stride(0), _p(FB), FB.stride(0), _p(target.contiguous()), NA, NB, FA.shape[0], FB.shape[0],
              FA.shape[1], _p(lse), _p(rowloss), _p(ws), nbytes, _stream())
    return lse, rowloss, ws


def pair_fused_bwd(target, lse, gloss, ws, NA: int, NB: int, rowsA: int, rowsB: int, K: int):
    """(dFA, dFB) of mean_r rowloss[r] times the device scalar gloss (sn_pair_fused_bwd_f32); rows past NA / NB are zero."""
    _dev(target, lse, gloss, ws)
    dFA = torch.empty((rowsA, K), dtype=torch.float32, device=lse.device)
    dFB = torch.empty((rowsB, K), dtype=torch.float32, device=lse.device)
    _lib.call("sn_pair_fused_bwd_f32", _p(target.contiguous()), _p(lse), _p(gloss), NA, NB, rowsA, rowsB, K, _p(dFA), K, _p(dFB), K,
              _p(ws), ws.numel(), _stream())
    return dFA, dFB


def _pair_loss_args(who, FA, FB, mapA, mapB, geo, NA, NB):
    _dev(FA, FB, mapA, mapB, geo)
    for t in (FA, FB):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise TypeError(f"{who}: row-major float32 feature matrices expected")
    if FA.shape[1] != FB.shape[1] or geo.dtype != torch.int64 or geo.numel() != 2 or not geo.is_contiguous():
        raise TypeError(f"{who}: features of one width and a table of two device addresses (int64) expected")
    for m, n in ((mapA, NA), (mapB, NB)):
        if m is not None and (m.dtype != torch.int64 or m.numel() != n or not m.is_contiguous()):
            raise TypeError(f"{who}: row maps are contiguous int64 permutations of the scored rows")
    if not (0 < NA <= FA.shape[0] and 0 < NB <= FB.shape[0]):
        raise ValueError(f"{who}: NA / NB do not fit the feature matrices")


def pair_soft_fwd(FA, FB, mapA, mapB, geo, ldgA: int, ldgB: int, NA: int, NB: int):
    """(stats, rowloss, workspace) of the soft-target cross entropy (main.py:216-227) from the tower features FA (rowsA x K),
    FB (rowsB x K) and the two label-order geodesic matrices whose device addresses `geo` (int64[2] on the device) holds
    (sn_pair_soft_fwd_f32).  stats = lse | softmin offset, 2 NA floats; the loss is rowloss.sum()."""
    _pair_loss_args("pair_soft_fwd", FA, FB, mapA, mapB, geo, NA, NB)
    ws, nbytes = _workspace("sn_pair_loss_workspace_bytes", FA.device, FA.shape[0], FB.shape[0], least=0)
    stats = torch.empty(2 * NA, dtype=torch.float32, device=FA.device)
    rowloss = torch.empty(NA, dtype=torch.float32, device=FA.device)
    _lib.call("sn_pair_soft_fwd_f32", _p(FA), FA.stride(0), _p(FB), FB.stride(0), _p(mapA), _p(mapB), _p(geo), ldgA, ldgB, NA, NB,
              FA.shape[0], FB.shape[0], FA.shape[1], _p(stats), _p(rowloss), _p(ws), nbytes, _stream())
    return stats, rowloss, ws


def pair_soft_bwd(mapA, mapB, geo, ldgA: int, ldgB: int, stats, gloss, ws, NA: int, NB: int, rowsA: int, rowsB: int, K: int):
    """(dFA, dFB) of rowloss.sum() times the device scalar gloss (sn_pair_soft_bwd_f32); rows past NA / NB are zero."""
    _dev(mapA, mapB, geo, stats, gloss, ws)
    dFA = torch.empty((rowsA, K), dtype=torch.float32, device=stats.device)
    dFB = torch.empty((rowsB, K), dtype=torch.float32, device=stats.device)
    _lib.call("sn_pair_soft_bwd_f32", _p(mapA), _p(mapB), _p(geo), ldgA, ldgB, _p(stats), _p(gloss), NA, NB, rowsA, rowsB, K, _p(dFA), K,
              _p(dFB), K, _p(ws), ws.numel(), _stream())
    return dFA, dFB


def pair_sl1_fwd(FA, FB, mapA, mapB, geo, ldgA: int, ldgB: int, NA: int, NB: int):
    """(rowloss (fp64, rowsA), workspace) of the smooth-L1 loss against the zero-padded geodesic sum (main.py:197-214):
    sn_pair_sl1_fwd_f32; the loss is rowloss.sum() / (rowsA rowsB)."""
    _pair_loss_args("pair_sl1_fwd", FA, FB, mapA, mapB, geo, NA, NB)
    ws, nbytes = _workspace("sn_pair_loss_workspace_bytes", FA.device, FA.shape[0], FB.shape[0], least=0)
    rowloss = torch.empty(FA.shape[0], dtype=torch.float64, device=FA.device)
    _lib.call("sn_pair_sl1_fwd_f32", _p(FA), FA.stride(0), _p(FB), FB.stride(0), _p(mapA), _p(mapB), _p(geo), ldgA, ldgB, NA, NB,
              FA.shape[0], FB.shape[0], FA.shape[1], _p(rowloss), _p(ws), nbytes, _stream())
    return rowloss, ws


def pair_sl1_bwd(mapA, mapB, geo, ldgA: int, ldgB: int, gloss, ws, NA: int, NB: int, rowsA: int, rowsB: int, K: int):
    """(dFA, dFB) of the mean smooth-L1 times the device scalar gloss (sn_pair_sl1_bwd_f32); the padding rows are scored too."""
    _dev(mapA, mapB, geo, gloss, ws)
    dFA = torch.empty((rowsA, K), dtype=torch.float32, device=gloss.device)
    dFB = torch.empty((rowsB, K), dtype=torch.float32, device=gloss.device)
    _lib.call("sn_pair_sl1_bwd_f32", _p(mapA), _p(mapB), _p(geo), ldgA, ldgB, _p(gloss), NA, NB, rowsA, rowsB, K, _p(dFA), K, _p(dFB), K,
              _p(ws), ws.numel(), _stream())
    return dFA, dFB


def pair_match(FA, FB, NA: int, NB: int, both: bool = True, geoB=None, truthA=None):
    """(colA, bestA, rowB, bestB, errA) from the tower features FA (rowsA x K), FB (rowsB x K): colA[r] = argmax_j S[r][j] over
    the NA x NB corner of S = FA·FBᵀ (models.py:203) and bestA[r] that score; with `both`, rowB[j] = argmax_r S[r][j] and
    bestB[j]; with geoB (fp32, at least NB x NB) and truthA (int64[NA], the true vertex of B per row, -1 = none),
    errA[r] = geoB[truthA[r], colA[r]] (NaN where there is no truth).  None where not asked for.  Ties go to the smaller index
    (numpy.argmax).  The scores are never written (sn_pair_match_f32)."""
    _dev(FA, FB, geoB, truthA)
    for t in (FA, FB):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise TypeError("pair_match: row-major float32 feature matrices expected")
    if FA.shape[1] != FB.shape[1]:
        raise TypeError("pair_match: features of one width expected")
    if not (0 < NA <= FA.shape[0] and 0 < NB <= FB.shape[0]):
        raise ValueError("pair_match: NA / NB do not fit the feature matrices")
    if (geoB is None) != (truthA is None):
        raise ValueError("pair_match: geoB and truthA come together")
    if geoB is not None:
        if geoB.dtype != torch.float32 or geoB.dim() != 2 or geoB.stride(1) != 1 or truthA.dtype != torch.int64:
            raise TypeError("pair_match: a row-major float32 geodesic matrix and int64 true matches expected")
        if geoB.shape[0] < NB or geoB.shape[1] < NB or truthA.numel() != NA:
            raise ValueError("pair_match: geoB holds fewer than NB x NB entries, or truthA not NA")
        truthA = truthA.contiguous()
    dev = FA.device
    ws, nbytes = _workspace("sn_pair_match_workspace_bytes", dev, FA.shape[0], FB.shape[0], least=0)
    colA = torch.empty(NA, dtype=torch.int64, device=dev)
    bestA = torch.empty(NA, dtype=torch.float32, device=dev)
    rowB = torch.empty(NB, dtype=torch.int64, device=dev) if both else None
    bestB = torch.empty(NB, dtype=torch.float32, device=dev) if both else None
    errA = torch.empty(NA, dtype=torch.float32, device=dev) if geoB is not None else None
    _lib.call("sn_pair_match_f32", _p(FA), FA.stride(0), _p(FB), FB.stride(0), NA, NB, FA.shape[0], FB.shape[0], FA.shape[1], _p(colA),
              _p(bestA), _p(rowB), _p(bestB), _p(geoB), geoB.stride(0) if geoB is not None else 0, _p(truthA), _p(errA), _p(ws), nbytes,
              _stream())
    return colA, bestA, rowB, bestB, errA


def masked_smooth_l1_fwd(out2d, target2d, rowmask, scale: float):
    """scale * sum smooth_l1(out*rowmask - target) as a 0-dim fp32 tensor (sn_masked_smooth_l1_fwd_f32)."""
    _dev(out2d, target2d, rowmask)
    rows, C = out2d.shape
    loss = torch.empty((), dtype=torch.float32, device=out2d.device)
    ws, ws_bytes = _workspace("sn_masked_smooth_l1_workspace_bytes", out2d.device, rows, C, least=0)
    _lib.call("sn_masked_smooth_l1_fwd_f32", _p(out2d), _ld(out2d), _p(target2d), _ld(target2d), _p(rowmask), rows, C,
              float(scale), _p(loss), _p(ws), ws_bytes, _stream())
    return loss


def masked_smooth_l1_bwd(out2d, target2d, rowmask, scale: float, gloss):
    """Gradient of masked_smooth_l1_fwd w.r.t. out2d, times the device scalar gloss (sn_masked_smooth_l1_bwd_f32)."""
    _dev(out2d, target2d, rowmask, gloss)
    rows, C = out2d.shape
    g = torch.empty((rows, C), dtype=torch.float32, device=out2d.device)
    _lib.call("sn_masked_smooth_l1_bwd_f32", _p(out2d), _ld(out2d), _p(target2d), _ld(target2d), _p(rowmask), rows, C,
              float(scale), _p(gloss), _p(g), C, _stream())
    return g


def masked_smooth_l1_fwdg(out2d, target2d, rowmask, scale: float):
    """(loss, g): masked_smooth_l1_fwd's loss — same bits — and, from the same pass over out2d and target2d, the gradient
    masked_smooth_l1_bwd returns for gloss == 1 (sn_masked_smooth_l1_fwdg_f32).  masked_smooth_l1_bwdg finishes g for any gloss."""
    _dev(out2d, target2d, rowmask)
    rows, C = out2d.shape
    loss = torch.empty((), dtype=torch.float32, device=out2d.device)
    g = torch.empty((rows, C), dtype=torch.float32, device=out2d.device)
    ws, ws_bytes = _workspace("sn_masked_smooth_l1_workspace_bytes", out2d.device, rows, C, least=0)
    _lib.call("sn_masked_smooth_l1_fwdg_f32", _p(out2d), _ld(out2d), _p(target2d), _ld(target2d), _p(rowmask), rows, C,
              float(scale), _p(loss), _p(g), C, _p(ws), ws_bytes, _stream())
    return loss, g


def masked_smooth_l1_bwdg(out2d, target2d, rowmask, scale: float, gloss, g):
    """masked_smooth_l1_bwd into the buffer masked_smooth_l1_fwdg left for the same operands: the launch returns at once when
    the device scalar gloss is 1 and recomputes g otherwise — the same bits either way (sn_masked_smooth_l1_bwdg_f32)."""
    _dev(out2d, target2d, rowmask, gloss, g)
    rows, C = out2d.shape
    if g.shape != (rows, C) or g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("masked_smooth_l1_bwdg: g must be the contiguous (rows, C) float32 buffer of masked_smooth_l1_fwdg")
    _lib.call("sn_masked_smooth_l1_bwdg_f32", _p(out2d), _ld(out2d), _p(target2d), _ld(target2d), _p(rowmask), rows, C,
              float(scale), _p(gloss), _p(g), C, _stream())
    return g


def _cos_rows(y2d, target2d, rowmask, frame2d, what: str):
    """Operand checks shared by the normal_cosine_* launchers: (rows, ldy, ldt, ldf).  y2d: (rows, 3) with a row pitch of 3 or 4
    floats, or a contiguous (rows, 4) buffer whose first three columns are the operand (pitch 4 whatever the row count)."""
    _dev(y2d, target2d, rowmask, frame2d)
    for t in (y2d, target2d, rowmask, frame2d):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{what}: float32 operands expected")
    if y2d.dim() != 2 or y2d.shape[1] not in (3, 4) or (y2d.shape[1] == 4 and not y2d.is_contiguous()):
        raise ValueError(f"{what}: y is (rows, 3) or a contiguous (rows, 4) buffer, got {tuple(y2d.shape)} stride {y2d.stride()}")
    rows = y2d.shape[0]
    if tuple(target2d.shape) != (rows, 3) or (frame2d is not None and tuple(frame2d.shape) != (rows, 3)):
        raise ValueError(f"{what}: target and frame are (rows, 3) for y {tuple(y2d.shape)}")
    if rowmask is not None and (rowmask.numel() != rows or not rowmask.is_contiguous()):
        raise ValueError(f"{what}: rowmask must hold one contiguous float per row")
    ldy = 4 if y2d.shape[1] == 4 else _ld(y2d)
    if ldy not in (3, 4):
        raise ValueError(f"{what}: a row pitch of 3 or 4 floats expected, got {ldy}")
    if ldy == 4 and rows and (y2d.storage_offset() + 4 * rows) * 4 > y2d.untyped_storage().nbytes():
        raise ValueError(f"{what}: the fourth float of the last pitch-4 row lies outside the tensor's storage")
    return rows, ldy, _ld(target2d), (_ld(frame2d) if frame2d is not None else 0)


def normal_cosine_grid_rows() -> int:
    """Rows one sweep of the loss grid covers (sn_normal_cosine_grid_rows): past it every thread takes more than one row."""
    return int(_lib.load().sn_normal_cosine_grid_rows())


def normal_cosine_fwd(y2d, target2d, rowmask=None, frame2d=None):
    """float32[3] on the device: squared-cosine loss, mean angle deviation and |S| of the rows rowmask selects (None: all) —
    sn_normal_cosine_fwd_f32, the definition in include/sn_spmm.h ("Normal prediction")."""
    rows, ldy, ldt, ldf = _cos_rows(y2d, target2d, rowmask, frame2d, "normal_cosine_fwd")
    out = torch.empty(3, dtype=torch.float32, device=y2d.device)
    ws, ws_bytes = _workspace("sn_normal_cosine_workspace_bytes", y2d.device, rows, least=0)
    _lib.call("sn_normal_cosine_fwd_f32", _p(y2d), ldy, _p(frame2d), ldf, _p(target2d), ldt, _p(rowmask), rows, _p(out), _p(ws),
              ws_bytes, _stream())
    return out


def normal_cosine_fwdg(y2d, target2d, rowmask=None, frame2d=None, pitch: int = 0):
    """(out, g): normal_cosine_fwd's three numbers — the same bits — and, from the same pass, the gradient of the loss w.r.t. y for
    gloss == 1 (sn_normal_cosine_fwdg_f32).  g: a fresh contiguous (rows, pitch) buffer, pitch 3 or 4 (0: that of y2d); the fourth
    column of a pitch-4 buffer is written 0.  normal_cosine_bwd(..., g=g) finishes it for any gloss."""
    rows, ldy, ldt, ldf = _cos_rows(y2d, target2d, rowmask, frame2d, "normal_cosine_fwdg")
    pitch = pitch or ldy
    if pitch not in (3, 4):
        raise ValueError("normal_cosine_fwdg: pitch 3 or 4")
    out = torch.empty(3, dtype=torch.float32, device=y2d.device)
    g = torch.empty((rows, pitch), dtype=torch.float32, device=y2d.device)
    ws, ws_bytes = _workspace("sn_normal_cosine_workspace_bytes", y2d.device, rows, least=0)
    _lib.call("sn_normal_cosine_fwdg_f32", _p(y2d), ldy, _p(frame2d), ldf, _p(target2d), ldt, _p(rowmask), rows, _p(out), _p(g),
              pitch, _p(ws), ws_bytes, _stream())
    return out, g


def normal_cosine_bwd(y2d, target2d, rowmask, frame2d, out, gloss, g=None, pitch: int = 0):
    """Gradient of the loss w.r.t. y times the device scalar gloss, a contiguous (rows, pitch) buffer.  g=None: a fresh one
    (sn_normal_cosine_bwd_f32; pitch as normal_cosine_fwdg).  g = the buffer normal_cosine_fwdg returned for the same operands, out
    its three numbers: kept when gloss is 1 — tested on the device — and recomputed otherwise, the same bits either way
    (sn_normal_cosine_bwdg_f32)."""
    rows, ldy, ldt, ldf = _cos_rows(y2d, target2d, rowmask, frame2d, "normal_cosine_bwd")
    _dev(out, gloss, g)
    if out.dtype != torch.float32 or out.numel() != 3 or not out.is_contiguous() or gloss.dtype != torch.float32 or gloss.numel() != 1:
        raise ValueError("normal_cosine_bwd: out is the float32[3] of a forward call, gloss one float32")
    name = "sn_normal_cosine_bwdg_f32"
    if g is None:
        name = "sn_normal_cosine_bwd_f32"
        pitch = pitch or ldy
        if pitch not in (3, 4):
            raise ValueError("normal_cosine_bwd: pitch 3 or 4")
        g = torch.empty((rows, pitch), dtype=torch.float32, device=y2d.device)
    elif g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != rows or g.shape[1] not in (3, 4) or not g.is_contiguous():
        raise ValueError("normal_cosine_bwd: g must be the contiguous (rows, 3 | 4) float32 buffer normal_cosine_fwdg returned")
    _lib.call(name, _p(y2d), ldy, _p(frame2d), ldf, _p(target2d), ldt, _p(rowmask), rows, _p(out[2:]), _p(gloss), _p(g), g.shape[1],
              _stream())
    return g


def mesh_match(rowptr, colind, vals, n: int, mass=None, max_rounds: int = 1024):
    """(mate int32[n], r fp32[n], msum fp32[n], out int32[2]) of one coarsening step of a square CSR operator
    (sn_mesh_match_f32; include/sn_spmm.h "Mesh hierarchy"): the handshake matching on the edge scores, the restriction
    weights and the merged masses; out = (rounds, status word) stays on the device — the caller reads it."""
    _dev(rowptr, colind, vals, mass)
    if rowptr.dtype != torch.int32 or colind.dtype != torch.int32 or vals.dtype != torch.float32 or rowptr.numel() != n + 1:
        raise ValueError("mesh_match: int32 rowptr[n + 1] / colind and float32 vals expected")
    if mass is not None and (mass.dtype != torch.float32 or mass.numel() != n or not mass.is_contiguous()):
        raise ValueError(f"mesh_match: mass must hold {n} contiguous float32 values")
    dev = rowptr.device
    nnz = int(colind.numel())
    mate = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    r = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    msum = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    out = torch.empty(2, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_mesh_match_workspace_bytes", dev, n, nnz)
    _lib.call("sn_mesh_match_f32", _p(rowptr), _p(colind), _p(vals), _p(mass), n, nnz, int(max_rounds), _p(mate), _p(r), _p(msum),
              _p(out), _p(ws), ws_bytes, _stream())
    return mate, r, msum, out


def _pool_rows(what: str, *tensors):
    """Operand checks shared by the sibling-pair pooling launchers (include/sn_spmm.h, "Sibling-pair pooling"): fp32 (B, V, C)
    device tensors with C >= 1; returns them as (B * V, C) matrices with contiguous rows — views where the rows have one pitch
    (a contiguous tensor, a column slice of one), else copies."""
    _dev(*tensors)
    out = []
    for t in tensors:
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: float32 operands expected, got {t.dtype}")
        if t.dim() != 3 or t.shape[2] < 1:
            raise ValueError(f"{what}: (B, V, C) operands with C >= 1 expected, got {tuple(t.shape)}")
        B, V, C = t.shape
        pitch = C
        if not t.is_contiguous():
            if V > 1 and (C == 1 or t.stride(2) == 1) and t.stride(1) >= C and (B == 1 or t.stride(0) == V * t.stride(1)):
                pitch = t.stride(1)
            else:
                t = t.contiguous()
        out.append(t.as_strided((B * V, C), (pitch, 1)))
    return out


def _even_nodes(what: str, t) -> None:
    if t.dim() == 3 and t.shape[1] % 2:
        raise ValueError(f"{what}: the node axis holds sibling pairs, so its length must be even; got {tuple(t.shape)}")


def pool_max2_fwd(x):
    """(B, V / 2, C): the larger of each sibling pair of rows of x (B, V, C), torch's MaxPool1d(2) choice (sn_pool_max2_fwd_f32)."""
    _even_nodes("pool_max2_fwd", x)
    (x2,) = _pool_rows("pool_max2_fwd", x)
    B, V, C = x.shape
    y = torch.empty((B, V // 2, C), dtype=torch.float32, device=x.device)
    _lib.call("sn_pool_max2_fwd_f32", _p(x2), _ld(x2), B * V // 2, C, _p(y), C, _stream())
    return y


def pool_max2_bwd(x, g):
    """(B, V, C): g (B, V / 2, C) routed to the row of each pair that pool_max2_fwd chose, zero to the other; the choice is made
    again from x (sn_pool_max2_bwd_f32)."""
    _even_nodes("pool_max2_bwd", x)
    x2, g2 = _pool_rows("pool_max2_bwd", x, g)
    B, V, C = x.shape
    if tuple(g.shape) != (B, V // 2, C):
        raise ValueError(f"pool_max2_bwd: g must be {(B, V // 2, C)} for x {tuple(x.shape)}, got {tuple(g.shape)}")
    gx = torch.empty((B, V, C), dtype=torch.float32, device=x.device)
    _lib.call("sn_pool_max2_bwd_f32", _p(x2), _ld(x2), _p(g2), _ld(g2), B * V // 2, C, _p(gx), C, _stream())
    return gx


def unpool2_add_fwd(x, skip):
    """(B, V, C): y[b, 2 j + s] = x[b, j] + skip[b, 2 j + s] for x (B, V / 2, C) and skip (B, V, C) (sn_unpool2_add_fwd_f32)."""
    _even_nodes("unpool2_add_fwd", skip)
    x2, s2 = _pool_rows("unpool2_add_fwd", x, skip)
    B, V, C = skip.shape
    if tuple(x.shape) != (B, V // 2, C):
        raise ValueError(f"unpool2_add_fwd: x must be {(B, V // 2, C)} for skip {tuple(skip.shape)}, got {tuple(x.shape)}")
    y = torch.empty((B, V, C), dtype=torch.float32, device=x.device)
    _lib.call("sn_unpool2_add_fwd_f32", _p(x2), _ld(x2), _p(s2), _ld(s2), B * V // 2, C, _p(y), C, _stream())
    return y


def unpool2_bwd(g):
    """(B, V / 2, C): gx[b, j] = g[b, 2 j] + g[b, 2 j + 1] for g (B, V, C) (sn_unpool2_bwd_f32)."""
    _even_nodes("unpool2_bwd", g)
    (g2,) = _pool_rows("unpool2_bwd", g)
    B, V, C = g.shape
    gx = torch.empty((B, V // 2, C), dtype=torch.float32, device=g.device)
    _lib.call("sn_unpool2_bwd_f32", _p(g2), _ld(g2), B * V // 2, C, _p(gx), C, _stream())
    return gx


def linear_fwd_segbias(x, W, segbias, rows_per_seg: int, residual=None, y_elu=None, want_y: bool = True, elu_stats=None,
                       tile_sums=None):
    """y = x·W^T + segbias[row // rows_per_seg] (+ residual), optionally elu(y) into y_elu; want_y=False: only y_elu is written.
    tile_sums: as linear_fwd."""
    _dev(x, W, segbias, residual, y_elu, tile_sums)
    rows, K = x.shape
    J = W.shape[0]
    y = torch.empty((rows, J), dtype=torch.float32, device=x.device) if want_y else None
    _lib.call("sn_linear_fwd_segbias_tiles_f32", _p(x), _ld(x), _p(W), _ld(W), _p(segbias), rows_per_seg, _p(residual),
              _ld(residual) if residual is not None else 0, _p(y), J, _p(y_elu), _ld(y_elu) if y_elu is not None else 0,
              rows, K, J, _p(elu_stats), _p(tile_sums), _stream())
    return y


def linear_dgrad_eluseg(dy, W, x, center, B, Cc, segvec, rows_per_seg: int, rowmask=None, gadd=None):
    """(dy·W + (x - center) B + Cc + rowmask * segvec[row // rows_per_seg]) * elu'(x) + gadd for all C columns
    (segvec=None: no per-mesh vector)."""
    _dev(dy, W, x, center, B, Cc, segvec, rowmask, gadd)
    rows, J = dy.shape
    C = x.shape[1]
    gact = torch.empty((rows, C), dtype=torch.float32, device=dy.device)
    am = _new_dgrad_absmax(dy.device)
    _lib.call("sn_linear_dgrad_eluseg_absmax_f32", _p(dy), _ld(dy), _p(W), _ld(W), _p(x), _ld(x), _p(center), _p(B), _p(Cc),
              _p(segvec), rows_per_seg, _p(rowmask), _p(gact), C, _p(gadd), _ld(gadd) if gadd is not None else 0, rows, J, C,
              _p(am), _stream())
    note_absmax(gact, am)
    return gact


# ---- lattice Delaunay, Poisson-disc sampling, the Mesh-MNIST maker (csrc/sn_delaunay.hip) -------------------------------------
DT_MAX_ROUNDS = 4096                             # default flip-round budget (210 random points take about 50 rounds)

Delaunay2D = collections.namedtuple("Delaunay2D", "F nF status counts")
PoissonDisc = collections.namedtuple("PoissonDisc", "P count steps")
MeshDigitsOut = collections.namedtuple("MeshDigitsOut", "P count V F nF status attempts counts")


def delaunay_max_points() -> int:
    return int(_lib.load().sn_delaunay2d_max_points())


def delaunay_2d(P, count=None, max_rounds: int = DT_MAX_ROUNDS) -> Delaunay2D:
    """Delaunay triangulations of a padded batch of lattice point sets on the device (sn_delaunay2d_i32; definition in
    include/sn_spmm.h, "Lattice Delaunay and the Mesh-MNIST maker"; host statement mesh_ops.delaunay_2d).  P: (B, Nmax, 2) int32,
    count: (B,) int32 or None (every set has Nmax points).  Returns Delaunay2D of int32 device tensors: F (B, 2 Nmax, 3) canonical
    faces with -1 past nF, nF (B,), status (B,) of DT_* bits, counts (B, 4) = flips, cocircular, rounds, boundary vertices.  A
    refused set has nF = 0 and does not disturb the others.  Does not synchronise; two runs are bit-identical."""
    _dev(P, count)
    if P.dtype != torch.int32 or P.dim() != 3 or P.shape[2] != 2:
        raise TypeError("delaunay_2d wants P (B, Nmax, 2) int32")
    B, nmax = P.shape[0], P.shape[1]
    if count is not None and (count.dtype != torch.int32 or count.shape != (B,)):
        raise TypeError("delaunay_2d wants count (B,) int32")
    P = P.contiguous()
    count = None if count is None else count.contiguous()
    dev = P.device
    F = torch.empty(B, 2 * nmax, 3, dtype=torch.int32, device=dev)
    nF = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
    _lib.call("sn_delaunay2d_i32", _p(P), _p(count), B, nmax, int(max_rounds), _p(F), _p(nF), _p(status), _p(counts), _stream())
    return Delaunay2D(F, nF, status, counts)


def poisson_disc_cells(width: int, height: int, R: int) -> int:
    """Cells of the sampler's grid for a width x height pixel domain and radius R lattice units: the most samples one image can
    get.  ValueError for parameters outside the lattice or with more cells than SN_DELAUNAY_MAX_POINTS."""
    cells = int(_lib.load().sn_poisson_disc_cells(int(width), int(height), int(R)))
    if cells < 0:
        raise ValueError(f"poisson_disc: domain {width} x {height} with R = {R} is refused "
                         f"({_lib.load().sn_status_string(cells).decode()}; at most {delaunay_max_points()} cells)")
    return cells


def poisson_disc(batch: int, seed: int = 0, image_base: int = 0, attempt: int = 0, R: int = 98304, width: int = 27, height: int = 27,
                 device="cuda") -> PoissonDisc:
    """Bridson Poisson-disc samples in integers for images image_base .. image_base + batch - 1 (sn_poisson_disc_i32, host
    statement mesh_ops.poisson_disc).  R: the radius in lattice units (2^16 per pixel).  Returns PoissonDisc(P (B, cells, 2) int32
    in the order the samples were made, count (B,), steps (B,)) on the device.  Does not synchronise."""
    cells = poisson_disc_cells(width, height, R)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("surfacenetworks_amd kernels run on the MI355X only: there is no CPU/eager fallback in this package")
    P = torch.empty(batch, cells, 2, dtype=torch.int32, device=dev)
    count = torch.empty(batch, dtype=torch.int32, device=dev)
    steps = torch.empty(batch, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("sn_poisson_disc_i32", int(seed) & (2 ** 64 - 1), int(image_base), int(attempt), int(width), int(height), int(R),
                  int(batch), cells, _p(P), _p(count), _p(steps), _stream())
    return PoissonDisc(P, count, steps)


def mesh_digits(images, seed: int = 0, R: int = 98304, min_points: int = 101, min_det: int = MESHDIGITS_MIN_DET, image_base: int = 0,
                max_attempts: int = MESHDIGITS_MAX_ATTEMPTS, max_rounds: int = DT_MAX_ROUNDS) -> MeshDigitsOut:
    """Images to meshes in one launch: sampler, Delaunay, quality test, retries and intensity (sn_mesh_digits_u8, host statement
    mesh_ops.mesh_digits).  images: (B, rows, cols) uint8 on the device.  Returns MeshDigitsOut of device tensors padded to the
    sampler's cell count Nmax: P (B, Nmax, 2) int32, count (B,), V (B, Nmax, 3) fp32, F (B, 2 Nmax, 3) int32 (-1 past nF), nF,
    status (0 or DT_REJECTED), attempts, counts (B, 4).  Does not synchronise; two runs are bit-identical."""
    _dev(images)
    if images.dtype != torch.uint8 or images.dim() != 3:
        raise TypeError("mesh_digits wants images (B, rows, cols) uint8")
    B, rows, cols = images.shape
    cells = poisson_disc_cells(cols - 1, rows - 1, R)
    images = images.contiguous()
    dev = images.device
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = MeshDigitsOut(i32(B, cells, 2), i32(B), torch.empty(B, cells, 3, dtype=torch.float32, device=dev), i32(B, 2 * cells, 3),
                        i32(B), i32(B), i32(B), i32(B, 4))
    _lib.call("sn_mesh_digits_u8", _p(images), B, rows, cols, int(seed) & (2 ** 64 - 1), int(image_base), int(R), int(min_points),
              int(min_det), int(max_attempts), int(max_rounds), cells, _p(out.P), _p(out.count), _p(out.V), _p(out.F), _p(out.nF),
              _p(out.status), _p(out.attempts), _p(out.counts), _stream())
    return out


# ---- ARAP deformation (include/sn_spmm.h, "ARAP deformation"; host statement mesh_ops.arap_*) ------------------------------------
ARAP_FRAMES_PER_LAUNCH = 5               # LABNOTES.md#arapdeform: one launch stays a bounded piece of work

ArapWeights = collections.namedtuple("ArapWeights", "rowptr colind w d status")
ArapFrames = collections.namedtuple("ArapFrames", "frames cg_iters energy status R_first rhs_first")


def arap_max_vertices() -> int:
    """The largest mesh sn_arap_frames_f64 takes (its search direction lives in the LDS of one compute unit)."""
    return int(_lib.load().sn_arap_max_vertices())


def arap_weights(V0, F) -> ArapWeights:
    """The ARAP weights of a rest mesh, or of a disjoint union of rest meshes, on the device (sn_arap_weights_f64): rowptr
    (nV + 1,) int32, colind and w sized for 6 nF entries of which rowptr[nV] are used, d (nV,) fp64, status (1,) int32
    (ARAP_BAD_FACE / ARAP_DEGREE).  V0 (nV, 3) fp32, F (nF, 3) int32.  Does not synchronise."""
    _dev(V0, F)
    _check_mesh("arap_weights", V0, F)
    V0, F = V0.contiguous(), F.contiguous()
    nV, nF = V0.shape[0], F.shape[0]
    dev = V0.device
    rowptr = torch.empty(nV + 1, dtype=torch.int32, device=dev)
    colind = torch.empty(6 * nF, dtype=torch.int32, device=dev)
    w = torch.empty(6 * nF, dtype=torch.float64, device=dev)
    d = torch.empty(nV, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace("sn_arap_weights_workspace_bytes", dev, nV, nF)
    _lib.call("sn_arap_weights_f64", _p(V0), _p(F), nV, nF, rowptr.data_ptr(), _p(colind), _p(w), _p(d), status.data_ptr(), _p(ws),
              ws_bytes, _stream())
    return ArapWeights(rowptr, colind, w, d, status)


def arap_frames(V0, weights: ArapWeights, voff, hoff, handles, H, max_mesh_vertices: int, iters: int = 2, tol: float = 1e-10,
                max_cg: int = 4096, frames_per_launch: int = None, first_step: bool = False) -> ArapFrames:
    """The frames of a batch of ARAP sequences (sn_arap_frames_f64), one workgroup per mesh, enqueued in chunks of
    frames_per_launch frames (default: ARAP_FRAMES_PER_LAUNCH) that carry their state in one workspace.  V0 (nV, 3) fp32 and handles (nH,) int32 index the disjoint
    union; voff, hoff (B + 1,) int32 device tensors cut it into meshes; H (T, nH, 3) fp32; max_mesh_vertices: the largest mesh
    (a host number: nothing is read back).  Returns ArapFrames of device tensors: frames (T, nV, 3) fp32, cg_iters (B, T, iters)
    int32, energy (B, T) fp64, status (B,) int32, and with first_step the rotations (nV, 3, 3) and right-hand side (nV, 3) of the
    first local step of frame 0 (else None).  Does not synchronise."""
    _dev(V0, voff, hoff, handles, H, *weights)
    if V0.dtype != torch.float32 or V0.dim() != 2 or V0.shape[1] != 3:
        raise TypeError("arap_frames wants V0 (nV, 3) float32")
    if H.dtype != torch.float32 or H.dim() != 3 or H.shape[2] != 3 or handles.dtype != torch.int32 or H.shape[1] != handles.numel():
        raise TypeError("arap_frames wants handles (nH,) int32 and H (T, nH, 3) float32")
    if voff.dtype != torch.int32 or hoff.dtype != torch.int32 or voff.numel() != hoff.numel() or voff.numel() < 1:
        raise TypeError("arap_frames wants voff and hoff (B + 1,) int32")
    iters, max_cg, chunk = int(iters), int(max_cg), int(ARAP_FRAMES_PER_LAUNCH if frames_per_launch is None else frames_per_launch)
    if iters < 1 or not 0 <= max_cg <= ARAP_MAX_CG or chunk < 1 or not float(tol) >= 0:
        raise ValueError(f"arap_frames: iters >= 1, 0 <= max_cg <= {ARAP_MAX_CG}, frames_per_launch >= 1 and tol >= 0 are required")
    if int(max_mesh_vertices) > arap_max_vertices():
        raise ValueError(f"arap_frames: a mesh of {int(max_mesh_vertices)} vertices, at most {arap_max_vertices()} are supported")
    V0, H, handles, voff, hoff = V0.contiguous(), H.contiguous(), handles.contiguous(), voff.contiguous(), hoff.contiguous()
    nV, nH, T, B = V0.shape[0], handles.numel(), H.shape[0], voff.numel() - 1
    dev = V0.device
    frames = torch.empty(T, nV, 3, dtype=torch.float32, device=dev)
    cg_iters = torch.empty(B, T, iters, dtype=torch.int32, device=dev)
    energy = torch.empty(B, T, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    R_first = torch.empty(nV, 3, 3, dtype=torch.float64, device=dev) if first_step else None
    rhs_first = torch.empty(nV, 3, dtype=torch.float64, device=dev) if first_step else None
    ws, ws_bytes = _workspace("sn_arap_frames_workspace_bytes", dev, nV)
    for begin in range(0, T, chunk):
        _lib.call("sn_arap_frames_f64", _p(V0), weights.rowptr.data_ptr(), _p(weights.colind), _p(weights.w), _p(weights.d),
                  voff.data_ptr(), hoff.data_ptr(), _p(handles), _p(H), B, nV, nH, T, int(max_mesh_vertices), begin,
                  min(chunk, T - begin), iters, float(tol), max_cg, _p(frames), _p(cg_iters), _p(energy), _p(status), _p(R_first),
                  _p(rhs_first), _p(ws), ws_bytes, _stream())
    return ArapFrames(frames, cg_iters, energy, status, R_first, rhs_first)


# ---- graph attention (include/sn_spmm.h, "Graph attention"; torch statement attention.attn_propagate_reference) --------------------
def attn_supported(C: int, heads: int) -> bool:
    """Whether the attention kernels take C channels in `heads` heads (sn_attn_supported)."""
    return bool(_lib.load().sn_attn_supported(int(C), int(heads)))


def _attn_check(what: str, rows: int, C: int, heads: int, a, *dense) -> None:
    if not attn_supported(C, heads):
        raise ValueError(f"{what}: C = {C} channels in {heads} heads is outside the supported set (C % 4 == 0, C <= "
                         f"{ATTN_MAX_CHANNELS}, C % heads == 0, (C / heads) % 4 == 0)")
    if a.dtype != torch.float32 or tuple(a.shape) != (2, C) or not a.is_contiguous():
        raise ValueError(f"{what}: a must be a contiguous (2, {C}) float32 tensor, got {tuple(a.shape)} {a.dtype}")
    for t in dense:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: float32 operands expected, got {t.dtype}")
        if tuple(t.shape) != (rows, C):
            raise ValueError(f"{what}: ({rows}, {C}) operands expected, got {tuple(t.shape)}")
        _ld(t)


def attn_elu_scores(x, a, heads: int, e):
    """e <- elu(x) (e: a (rows, C) view with contiguous rows, e.g. the first half of a concat buffer) and the (rows, 2 heads) scores
    of e under a, from one pass (sn_attn_elu_scores_f32).  Returns the scores."""
    _dev(x, a, e)
    rows, C = x.shape
    _attn_check("attn_elu_scores", rows, C, heads, a, x, e)
    s = torch.empty((rows, 2 * heads), dtype=torch.float32, device=x.device)
    _lib.call("sn_attn_elu_scores_f32", _p(x), _ld(x), _p(a), rows, C, int(heads), _p(e), _ld(e), _p(s), _stream())
    return s


def attn_propagate_fwd(rowptr, colind, M: int, K: int, e, s, heads: int, p):
    """p <- the attention-weighted sum of the rows of e over the pattern (rowptr, colind) (sn_attn_propagate_fwd_f32).  Returns
    (m, z), the (rows, heads) maxima and normalisers the backward pass reads."""
    _dev(rowptr, colind, e, s, p)
    if M != K:
        raise ValueError(f"attn_propagate_fwd: a square operator is required, got {(M, K)}")
    C = e.shape[1]
    if not attn_supported(C, heads):
        raise ValueError(f"attn_propagate_fwd: C = {C} channels in {heads} heads is outside the supported set")
    if tuple(e.shape) != (M, C) or tuple(p.shape) != (M, C) or tuple(s.shape) != (M, 2 * heads) or not s.is_contiguous():
        raise ValueError(f"attn_propagate_fwd: operands do not fit {M} rows of {C} channels in {heads} heads")
    m = torch.empty((M, heads), dtype=torch.float32, device=e.device)
    z = torch.empty((M, heads), dtype=torch.float32, device=e.device)
    _lib.call("sn_attn_propagate_fwd_f32", _p(rowptr), _p(colind), M, K, int(colind.numel()), _p(e), _ld(e), _p(s), C, int(heads),
              _p(p), _ld(p), _p(m), _p(z), _stream())
    return m, z


def attn_propagate_bwd(rowptr, colind, t_rowptr, t_colind, M: int, K: int, g, ge, e, p, s, m, z, a, heads: int):
    """(dx, da) of sn_attn_propagate_bwd_f32: g the gradient of p, ge the gradient of the e half (or None: dx is then the gradient
    of e itself, without the ELU's derivative); (t_rowptr, t_colind): the pattern of the transpose."""
    _dev(rowptr, colind, t_rowptr, t_colind, g, ge, e, p, s, m, z, a)
    if M != K:
        raise ValueError(f"attn_propagate_bwd: a square operator is required, got {(M, K)}")
    C = e.shape[1]
    _attn_check("attn_propagate_bwd", M, C, heads, a, g, ge, e, p)
    dx = torch.empty((M, C), dtype=torch.float32, device=e.device)
    da = torch.empty((2, C), dtype=torch.float32, device=e.device)
    ws, ws_bytes = _workspace("sn_attn_propagate_bwd_workspace_bytes", e.device, M, C, int(heads))
    _lib.call("sn_attn_propagate_bwd_f32", _p(rowptr), _p(colind), _p(t_rowptr), _p(t_colind), M, K, int(colind.numel()), _p(g), _ld(g),
              _p(ge), _ld(ge) if ge is not None else 0, _p(e), _ld(e), _p(p), _ld(p), _p(s), _p(m), _p(z), _p(a), C, int(heads),
              _p(dx), C, _p(da), _p(ws), ws_bytes, _stream())
    return dx, da
