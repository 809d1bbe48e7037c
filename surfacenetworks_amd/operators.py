"""Device-resident sparse operators of the Surface-Network path.

`SparseOperator`  one (usually batched block-diagonal) operator kept in HBM as CSR with int32 indices, plus —
                  built once and cached — the CSR of its transpose (for the backward) and the packed 4x4-block
                  BSR form used for the quaternionic Dirac operators.
`OperatorPool`    every mesh of a dataset converted ONCE (A and A^T, CSR and/or BSR4) and pooled in HBM; a batch
                  is assembled per step by one offset-concatenation launch instead of the reference's host-side
                  index shift + concat + coalesce() sort + H2D copy.

What this replaces in the reference (paths relative to the reference checkout):
    sp_sparse_to_pt_sparse      src/utils/utils_pt.py:56-69     (scipy -> torch COO, per sample per step)
    sparse_diag_cat             src/utils/utils_pt.py:41-53     (block-diagonal batching on the host, every step)
    sparse_cat                  src/utils/utils_pt.py:21-39     (3-D batched COO for SparseBMMFunc)
    transpose().coalesce()      src/utils/cuda/sparse_bmm_func.py:66-67  (re-done on every backward)
"""
from __future__ import annotations

import collections
import dataclasses
import os
import warnings
import weakref
from typing import Optional, Sequence

import numpy as np
import torch

from . import constants, kernels

__all__ = ["SparseOperator", "OperatorPool", "PackedSegments", "MaskedSegments", "as_operator", "dirac_operators_from_mesh",
           "laplacian_operator_from_mesh", "geodesic_matrix_from_mesh", "spgemm", "amplify_sequence_operators",
           "clean_mesh", "CleanMesh", "repair_mesh", "RepairedMesh", "vertex_descriptors", "MeshDescriptors", "vertex_normals", "face_areas", "vertex_mass",
           "gaussian_curvature", "delaunay_2d", "Delaunay2D", "arap_deform", "ArapDeformation", "laplacian_eigenpairs", "Eigenpairs",
           "wave_kernel_signature", "principal_curvatures", "PrincipalCurvatures", "curv4", "mesh_hierarchy", "MeshHierarchy"]

# A BSR4 copy is kept when zero-fill costs at most this much extra storage over CSR entries.
_BSR4_MAX_FILL = 1.6
# Form in which pools of Dirac operators assemble a batch: "q3" (quaternion-packed, default) or "bsr4"
# (functional.set_dirac_format switches both this and the kernel choice).
_POOL_FORMAT = "q3"
# SN_DEBUG_VALIDATE=1: every operator built from CSR arrays is checked on the device (SparseOperator.validate)
_DEBUG_VALIDATE = os.environ.get("SN_DEBUG_VALIDATE", "0") == "1"


class SparseOperator:
    """M x K fp32 sparse operator resident on one GPU (CSR, int32 indices).

    Quacks enough like the torch sparse tensors the reference models pass around: `.size()`, `.shape`,
    `.dim()`, `.is_cuda`, `.cuda()` (src/as_rigid_as_possible/models.py:133-136 inspects `Di.size()`).
    No gradient ever flows to an operator (src/utils/cuda/sparse_bmm_func.py:72).
    """

    layout = "sn_csr"
    requires_grad = False
    _format = None

    def __init__(self, rowptr, colind, vals, shape, *, batch: int = 1, transpose: "Optional[SparseOperator]" = None,
                 bsr4=None, q3=None):
        M, K = int(shape[0]), int(shape[1])
        self._shape = (M, K)
        if rowptr is None:
            if not isinstance(bsr4, tuple) and not isinstance(q3, tuple):
                raise ValueError("an operator needs CSR arrays, a BSR4 triple or a Q3 pair")
            self._csr = None                     # block-form-only operator (Dirac); CSR is expanded on demand
        else:
            if rowptr.dtype != torch.int32 or colind.dtype != torch.int32 or vals.dtype != torch.float32:
                raise TypeError("SparseOperator wants int32 rowptr/colind and float32 vals")
            if rowptr.numel() != M + 1 or colind.numel() != vals.numel():
                raise ValueError("inconsistent CSR arrays")
            self._csr = (rowptr, colind, vals)
            if _DEBUG_VALIDATE and rowptr.is_cuda:
                self.validate()
        self._nnz_cache = None
        self.batch = int(batch)                  # number of diagonal blocks (B of the reference's (B,R,K) operators)
        self.row_offsets = self.col_offsets = None   # packed (unpadded) batches: first row / column of every diagonal block
        # operator -> transpose is a strong reference, transpose -> operator a weak one: a strong pair would be a
        # reference cycle, and the per-step batch operators (hundreds of MB of HBM each) would then live until Python's
        # cyclic collector happens to run instead of being returned to the caching allocator when the step drops them
        self._t_strong = None
        self._t_weak = weakref.ref(transpose) if transpose is not None else None
        self._bsr4 = bsr4                        # (b_rowptr, b_colind, b_vals) | None | False (= not worthwhile)
        self._q3 = q3                            # (b_rowptr, q_blk) quaternion-packed form | None (unknown) | False (not a Dirac-type operator)
        self._rb4 = None                         # (b_ptr, b_col, b_val) 4x1 row-blocked form | None (not built) | False (not worthwhile)
        self._band = None                        # (max |column - row|, longest row, rows outside the ring window) | None (not measured)

    @property
    def format(self):
        """Storage form this operator's products take ("q3" | "bsr4" | "ring" | "rb4" | "csr"); None: the process default
        (functional.set_dirac_format / set_laplacian_format).  Shared with the attached transpose."""
        return self._format

    @format.setter
    def format(self, fmt):
        if fmt not in (None, "q3", "bsr4", "ring", "rb4", "csr"):
            raise ValueError(fmt)
        self._format = fmt
        t = self._t
        if t is not None:
            t._format = fmt

    @property
    def _t(self) -> "Optional[SparseOperator]":
        if self._t_strong is not None:
            return self._t_strong
        return self._t_weak() if self._t_weak is not None else None

    @_t.setter
    def _t(self, value):
        self._t_strong, self._t_weak = value, None

    # ---- tensor-like surface -------------------------------------------------------------------
    @property
    def shape(self):
        return torch.Size(self._shape)

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self._shape[dim]

    def dim(self) -> int:
        return 2

    # CSR arrays; for a BSR4-only operator they are expanded once (explicit zeros of the blocks dropped)
    def _ensure_csr(self):
        if self._csr is None:
            self._csr = _bsr4_to_csr(*self.bsr4(), self._shape[0])
        return self._csr

    @property
    def rowptr(self):
        return self._ensure_csr()[0]

    @property
    def colind(self):
        return self._ensure_csr()[1]

    @property
    def vals(self):
        return self._ensure_csr()[2]

    @property
    def nnz(self) -> int:
        if self._nnz_cache is None:
            if self._csr is not None:
                self._nnz_cache = int(self._csr[1].numel())
            elif isinstance(self._bsr4, tuple):
                self._nnz_cache = int(torch.count_nonzero(self._bsr4[2]).item())
            else:                                # Q3-only operator: every non-zero parameter appears four times in its block
                self._nnz_cache = 4 * int(torch.count_nonzero(self._q3[1][:, :3]).item())
        return self._nnz_cache

    def _nnz(self) -> int:
        return self.nnz

    @property
    def device(self):
        if self._csr is not None:
            return self._csr[0].device
        return (self._bsr4[0] if isinstance(self._bsr4, tuple) else self._q3[0]).device

    @property
    def is_cuda(self) -> bool:
        return self.device.type == "cuda"

    def cuda(self, *_, **__):
        return self.to("cuda")

    def _moved(self, device, transpose=None):
        """A copy of this operator's own arrays on `device` (the transpose is handled by to())."""
        mv = lambda t: t.to(device)
        b = tuple(mv(t) for t in self._bsr4) if isinstance(self._bsr4, tuple) else self._bsr4
        q = tuple(mv(t) for t in self._q3) if isinstance(self._q3, tuple) else self._q3
        csr = (None, None, None) if self._csr is None else tuple(mv(t) for t in self._csr)
        out = SparseOperator(*csr, self._shape, batch=self.batch, transpose=transpose, bsr4=b, q3=q)
        out._nnz_cache = self._nnz_cache
        out._band = self._band
        out.row_offsets, out.col_offsets = self.row_offsets, self.col_offsets
        return out

    def _cloned(self, transpose=None):
        cp = lambda t: t.clone()
        b = tuple(cp(t) for t in self._bsr4) if isinstance(self._bsr4, tuple) else self._bsr4
        q = tuple(cp(t) for t in self._q3) if isinstance(self._q3, tuple) else self._q3
        csr = (None, None, None) if self._csr is None else tuple(cp(t) for t in self._csr)
        out = SparseOperator(*csr, self._shape, batch=self.batch, transpose=transpose, bsr4=b, q3=q)
        out._rb4 = tuple(cp(t) for t in self._rb4) if isinstance(self._rb4, tuple) else self._rb4
        out._band = self._band
        out._nnz_cache = self._nnz_cache
        out.row_offsets, out.col_offsets = self.row_offsets, self.col_offsets
        return out

    def clone(self):
        """A deep copy (every materialised form, the attached transpose included): the static batch of a captured step is
        overwritten in place by every load, so it must not share arrays with a dataset's cached operators."""
        out = self._cloned()
        if self._t is not None:
            out._t = self._t._cloned(transpose=out)
        return out

    def to(self, device):
        device = torch.device(device)
        if device.type == self.device.type and (device.index is None or device.index == self.device.index):
            return self
        out = self._moved(device)
        t = self._t
        if t is not None:
            # the transpose's arrays are moved directly: t.to() would come back here through its own transpose link
            out._t = t._moved(device, transpose=out)
        return out

    def __repr__(self):
        return f"SparseOperator(shape={self._shape}, nnz={self.nnz}, batch={self.batch}, device={self.device})"

    def validate(self) -> None:
        """Debug check of the CSR arrays on the device (sn_validate_csr_i32): row pointers monotone from 0 to nnz, column
        indices inside [0, K) and strictly ascending per row, finite values.  Raises ValueError naming the defects.  Run on
        every operator built from CSR arrays when SN_DEBUG_VALIDATE=1 (the product kernels themselves do not bounds-check,
        like the reference's)."""
        rp, ci, va = self._ensure_csr()
        flags = kernels.validate_csr(rp, ci, va, self._shape[0], self._shape[1])
        if flags:
            names = {1: "rowptr[0] != 0", 2: "rowptr decreasing", 4: "rowptr[M] != nnz", 8: "column index out of range",
                     16: "row not sorted / duplicate columns", 32: "non-finite value"}
            raise ValueError("invalid CSR operator: " + ", ".join(v for k, v in names.items() if flags & k))

    # ---- derived forms --------------------------------------------------------------------------
    def t(self) -> "SparseOperator":
        """CSR of the transpose, built on first use by sn_csr_transpose_f32 and cached both ways."""
        t = self._t
        if t is None:
            M, K = self._shape
            tr, tc, tv = kernels.csr_transpose(self.rowptr, self.colind, self.vals, M, K)
            t = self._t = SparseOperator(tr, tc, tv, (K, M), batch=self.batch, transpose=self)
            t._format = self._format
        return t

    T = property(t)

    def matmul(self, other) -> "SparseOperator":
        """self · other between two SparseOperators (spgemm below); a dense right-hand side goes through functional.spmm."""
        if not isinstance(other, SparseOperator):
            raise TypeError("SparseOperator.matmul multiplies two SparseOperators; dense operands take functional.spmm")
        return spgemm(self, other)

    def __matmul__(self, other):
        return spgemm(self, other) if isinstance(other, SparseOperator) else NotImplemented

    @classmethod
    def from_bsr4(cls, fwd, bwd, shape, batch: int = 1) -> "SparseOperator":
        """Operator and its transpose given directly as BSR4 triples (kernels.dirac_from_mesh)."""
        M, K = int(shape[0]), int(shape[1])
        op = cls(None, None, None, (M, K), batch=batch, bsr4=tuple(fwd))
        opt = cls(None, None, None, (K, M), batch=batch, bsr4=tuple(bwd), transpose=op)
        op._t = opt
        return op

    def q3(self):
        """(b_rowptr, q_blk) — the quaternion-packed form (three floats + the block column per 4x4 block) — or None when the
        operator's blocks are not pure-quaternion matrices.  Built from the BSR4 form on first use; the check reads one
        flag back from the device (operators assembled by an OperatorPool arrive with the form already attached)."""
        if self._q3 is None:
            b = self.bsr4()
            if b is None:
                self._q3 = False
            else:
                q, flag = kernels.bsr4_to_q3(b[1], b[2])
                self._q3 = (b[0], q.view(-1, 4)) if int(flag.item()) == 0 else False
        return self._q3 or None

    @classmethod
    def from_q3(cls, fwd, bwd, shape, batch: int = 1) -> "SparseOperator":
        """Operator and its transpose given as quaternion-packed pairs (b_rowptr, q_blk) — what an OperatorPool of Dirac
        operators assembles per step."""
        M, K = int(shape[0]), int(shape[1])
        op = cls(None, None, None, (M, K), batch=batch, q3=tuple(fwd))
        opt = cls(None, None, None, (K, M), batch=batch, q3=tuple(bwd), transpose=op)
        op._t = opt
        return op

    def rb4(self):
        """(b_ptr, b_col, b_val): the 4x1 row-blocked form used by the Laplacian-type (group-1) products, built on the
        device on first use without a host synchronisation; None for operators with fewer than 2 entries per row on
        average (nothing to share between the rows of a group)."""
        if self._rb4 is None:
            M, K = self._shape
            if self._band is not None and self._band[1] == 0x7fffffff:
                self._rb4 = False                  # a row with non-ascending columns (band probe): the 4-way merge needs sorted rows
            elif self.nnz < 2 * M:
                self._rb4 = False
            else:
                self._rb4 = kernels.csr_to_rb4(self.rowptr, self.colind, self.vals, M, K)
        return self._rb4 or None

    def band(self):
        """(max |column - row|, longest row, rows with an entry outside the ring kernel's window) of the CSR arrays — what
        decides between the sliding-window kernel and the gather kernels for Laplacian-type products.  Measured on the device on
        first use (one host synchronisation per operator); operators assembled by an OperatorPool arrive with the values
        already attached (maxima / sums over their meshes)."""
        if self._band is None:
            M, K = self._shape
            self._band = kernels.csr_band(self.rowptr, self.colind, M, K)
        return self._band

    def ring_ok(self, N: int) -> bool:
        """True when the Laplacian-type product of this operator at N dense columns should take the sliding-window kernel:
        square, large enough to fill the chip with persistent strips, (nearly) every entry within the kernel's window of its
        row (the few rows that reach further — the wrap-around rows of closed meshes — gather from global memory in the kernel)."""
        M, K = self._shape
        if not kernels.spmm_ring_supported(N, 1, M, K):
            return False
        if self._band is None and self.is_cuda and torch.cuda.is_current_stream_capturing():
            return False                                   # measuring the band reads back to the host: never inside a capture
        band, longest, outside = self.band()
        return longest <= 32 and outside <= kernels.RING_MAX_OUTSIDE * M

    def bsr4(self):
        """(b_rowptr, b_colind, b_vals) or None when the 4x4-block form is not applicable / not worthwhile."""
        if self._bsr4 is None and self._csr is None and isinstance(self._q3, tuple):
            self._bsr4 = _q3_to_bsr4(*self._q3)          # export / fallback only
        if self._bsr4 is None:
            M, K = self._shape
            if M % 4 or K % 4 or self.nnz == 0:
                self._bsr4 = False
            else:
                b = kernels.csr_to_bsr4(self.rowptr, self.colind, self.vals, M, K)
                self._bsr4 = b if 16 * b[1].numel() <= _BSR4_MAX_FILL * self.nnz else False
        return self._bsr4 or None

    # ---- constructors ----------------------------------------------------------------------------
    @classmethod
    def from_scipy(cls, A, device="cuda", batch: int = 1) -> "SparseOperator":
        A = A.tocsr()
        A.sort_indices()
        return cls(torch.from_numpy(A.indptr.astype(np.int32)).to(device),
                   torch.from_numpy(A.indices.astype(np.int32)).to(device),
                   torch.from_numpy(A.data.astype(np.float32)).to(device), A.shape, batch=batch)

    @classmethod
    def from_torch_coo(cls, A: torch.Tensor) -> "SparseOperator":
        """From a coalesced torch sparse COO tensor on the GPU: 2-D (block-diagonal, the output of
        sparse_diag_cat) or 3-D (B,R,K) (the output of sparse_cat).  Conversion runs on the device."""
        if A.layout != torch.sparse_coo:
            raise TypeError("expected a torch sparse COO tensor")
        if not A.is_coalesced():
            A = A.coalesce()          # the reference coalesces before use (utils_pt.py:39,53)
        idx, vals = A._indices(), A._values()
        if vals.dtype != torch.float32:
            vals = vals.float()
        if A.dim() == 2:
            M, K = A.shape
            rowptr, colind = kernels.coo_to_csr(None, idx[0], idx[1], 1, M, K)
            return cls(rowptr, colind, vals.contiguous(), (M, K), batch=1)
        if A.dim() == 3:
            B, R, Kb = A.shape
            rowptr, colind = kernels.coo_to_csr(idx[0], idx[1], idx[2], B, R, Kb)
            return cls(rowptr, colind, vals.contiguous(), (B * R, B * Kb), batch=B)
        raise ValueError("operator must be 2-D or 3-D")

    # ---- export (tests / debugging) --------------------------------------------------------------
    def to_scipy(self):
        import scipy.sparse as sp

        return sp.csr_matrix((self.vals.cpu().numpy(), self.colind.cpu().numpy(), self.rowptr.cpu().numpy()),
                             shape=self._shape)


def _q3_to_bsr4(b_rowptr, q_blk):
    """Expand quaternion-packed records to BSR4 (torch arithmetic; export / generic-kernel fallback only)."""
    p1, p2, p3 = q_blk[:, 0], q_blk[:, 1], q_blk[:, 2]
    col = q_blk[:, 3].contiguous().view(torch.int32)
    z = torch.zeros_like(p1)
    rows = [torch.stack([z, p1, p2, p3], 1), torch.stack([-p1, z, p3, -p2], 1), torch.stack([-p2, -p3, z, p1], 1),
            torch.stack([-p3, p2, -p1, z], 1)]
    return b_rowptr, col.clone(), torch.stack(rows, 1).reshape(-1).contiguous()


def _bsr4_to_csr(b_rowptr, b_colind, b_vals, M: int):
    """Expand BSR4 to CSR with torch index arithmetic (not on the hot path: export / generic-kernel fallback only).
    Explicit zeros of the blocks are dropped so that the result equals the coalesced operator."""
    dev = b_rowptr.device
    Mb = M // 4
    nblk = int(b_colind.numel())
    cnt = (b_rowptr[1:] - b_rowptr[:-1]).long()                                   # blocks per block row
    brow = torch.repeat_interleave(torch.arange(Mb, device=dev), cnt)             # block row of each block
    q = torch.arange(4, device=dev)
    rows = (4 * brow[:, None, None] + q[None, :, None]).expand(nblk, 4, 4)
    cols = (4 * b_colind.long()[:, None, None] + q[None, None, :]).expand(nblk, 4, 4)
    v = b_vals.view(nblk, 4, 4)
    keep = v != 0
    rows, cols, v = rows[keep], cols[keep], v[keep]
    order = torch.argsort(rows * (4 * (int(b_colind.max().item()) + 1 if nblk else 1)) + cols)
    rows, cols, v = rows[order], cols[order], v[order]
    rowptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=M), 0)
    return rowptr.int(), cols.int(), v.contiguous()


def dirac_operators_from_mesh(V: torch.Tensor, F: torch.Tensor):
    """(Di, DiA) SparseOperators (with transposes attached) built on the device from vertex positions V and faces F —
    the on-the-fly replacement of the per-frame operators the reference precomputes with mesh.dirac
    (src/as_rigid_as_possible/add_laplacian.py:50-65).

    V: (nV,3) and F: (nF,3) for one mesh, or V: (B,nV,3) and F: (nF,3) shared / (B,nF,3) per-mesh faces for a batch
    of equally sized meshes, which yields the block-diagonal batched operators directly."""
    Vg, Fg, B, nV, nF = _offset_batch("dirac_operators_from_mesh", V, F, guard=False)
    di, diat, dia, dit = kernels.dirac_from_mesh(Vg, Fg)
    Di = SparseOperator.from_bsr4(di, dit, (4 * B * nF, 4 * B * nV), batch=B)
    DiA = SparseOperator.from_bsr4(dia, diat, (4 * B * nV, 4 * B * nF), batch=B)
    for o in (Di, Di._t, DiA, DiA._t):           # quaternion blocks by construction: pack without reading the check flag
        o._q3 = (o._bsr4[0], kernels.bsr4_to_q3(o._bsr4[1], o._bsr4[2])[0].view(-1, 4))
    return Di, DiA


def _mesh_offsets(B: int, nV: int, device) -> torch.Tensor:
    """(B,) int32: the first vertex of every mesh of a batch laid out as one disjoint mesh."""
    return torch.arange(B, device=device, dtype=torch.int32) * nV


def _offset_batch(who: str, V: torch.Tensor, F: torch.Tensor, guard: bool = True):
    """(Vg, Fg, B, nV, nF): a batch (B, nV, 3) with shared (nF, 3) or per-mesh (B, nF, 3) faces laid out as one disjoint mesh.
    guard: an index outside its own mesh becomes -1, so that it stays outside the batch and cannot land in a neighbour's block.
    That is for entry points that validate their faces and leave a bad one out.  sn_dirac_bsr4_from_mesh and
    sn_laplacian_csr_from_mesh do not: they would read V at -1, so their callers pass guard=False and get the plain F + b nV
    (arap_deform too: the layout it has always handed to its kernels)."""
    if V.dim() == 3:
        if V.shape[2] != 3 or F.dim() not in (2, 3) or F.shape[-1] != 3 or (F.dim() == 3 and F.shape[0] != V.shape[0]):
            raise ValueError(f"{who} wants V (B, nV, 3) with F (nF, 3) or (B, nF, 3), got {tuple(V.shape)} and {tuple(F.shape)}")
        B, nV = V.shape[0], V.shape[1]
        Fb = F if F.dim() == 3 else F.unsqueeze(0).expand(B, -1, -1)
        Fi = Fb.to(torch.int32)
        Fg = Fi + _mesh_offsets(B, nV, V.device).view(B, 1, 1)
        if guard:
            Fg = torch.where((Fi >= 0) & (Fi < nV), Fg, torch.full_like(Fi, -1))
        return V.reshape(B * nV, 3).float(), Fg.reshape(-1, 3), B, nV, Fb.shape[1]
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"{who} wants V (nV, 3) and F (nF, 3), got {tuple(V.shape)} and {tuple(F.shape)}")
    return V.float(), F.to(torch.int32), 1, V.shape[0], F.shape[0]


@dataclasses.dataclass
class MeshDescriptors:
    """What operators.vertex_descriptors returns: fp32 device tensors, None for an output that was not asked for.  Face outputs
    are (nF,) / (nF, 3), vertex outputs (nV,) / (nV, 3), with a leading batch axis for a batch; status is a 1-element int32
    device tensor of kernels.DESC_* bits (of the whole batch)."""
    face_area: Optional[torch.Tensor] = None
    face_normal: Optional[torch.Tensor] = None
    n_area: Optional[torch.Tensor] = None
    n_uniform: Optional[torch.Tensor] = None
    n_angle: Optional[torch.Tensor] = None
    mass_bary: Optional[torch.Tensor] = None
    mass_voronoi: Optional[torch.Tensor] = None
    gauss: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None
    status: Optional[torch.Tensor] = None


def vertex_descriptors(V: torch.Tensor, F: torch.Tensor, want=None) -> MeshDescriptors:
    """Normals, mass and curvature of a triangle mesh on the device (kernels.mesh_descriptors; include/sn_spmm.h, "Mesh
    descriptors", has the definition and mesh_ops.vertex_descriptors the host statement) — what the reference's
    src/utils/geom_utils.py takes from pyigl: compute_normals, area, laplacian_and_mass, gaussian_curvature.
    V: (nV, 3), F: (nF, 3), or a batch V: (B, nV, 3) with F shared or (B, nF, 3): one launch sequence over the offset faces,
    bit-identical to the per-mesh calls.  want: names of the MeshDescriptors fields to compute (None: all of them).
    Bad faces (an index outside the mesh, a repeated index) and flat faces contribute nothing and are reported in `status`
    together with vertices that have no normal.  Does not synchronise."""
    kernels._dev(V, F)
    Vg, Fg, B, nV, nF = _offset_batch("vertex_descriptors", V, F)
    out = kernels.mesh_descriptors(Vg, Fg, want)
    if V.dim() == 3:
        for name, (per_face, width) in kernels.DESCRIPTOR_FIELDS.items():
            if out[name] is not None:
                out[name] = out[name].view((B, nF if per_face else nV) + ((width,) if width > 1 else ()))
    return MeshDescriptors(**out)


def vertex_normals(V: torch.Tensor, F: torch.Tensor, weighting: str = "area") -> torch.Tensor:
    """(nV, 3) unit vertex normals, "area"-, "uniform"- or "angle"-weighted (igl.per_vertex_normals' three weightings; a vertex
    without a normal gets zeros) — geom_utils.compute_normals and the OBJ normals of sampler.py:23."""
    if weighting not in ("area", "uniform", "angle"):
        raise ValueError(f'vertex_normals: weighting must be "area", "uniform" or "angle", got {weighting!r}')
    return getattr(vertex_descriptors(V, F, want=["n_" + weighting]), "n_" + weighting)


def face_areas(V: torch.Tensor, F: torch.Tensor) -> torch.Tensor:
    """(nF,) face areas, 0 for a bad or flat face — geom_utils.area."""
    return vertex_descriptors(V, F, want=["face_area"]).face_area


def vertex_mass(V: torch.Tensor, F: torch.Tensor, kind: str = "voronoi") -> torch.Tensor:
    """(nV,) diagonal of the mass matrix: "voronoi" (Meyer's mixed cells) or "barycentric" — igl.massmatrix."""
    if kind not in ("voronoi", "barycentric"):
        raise ValueError(f'vertex_mass: kind must be "voronoi" or "barycentric", got {kind!r}')
    name = "mass_voronoi" if kind == "voronoi" else "mass_bary"
    return getattr(vertex_descriptors(V, F, want=[name]), name)


def gaussian_curvature(V: torch.Tensor, F: torch.Tensor, area_avg: bool = False) -> torch.Tensor:
    """(nV,) angle defect 2 pi - sum of the incident angles (igl.gaussian_curvature); area_avg: divided by the Voronoi mass, as
    geom_utils.gaussian_curvature does."""
    d = vertex_descriptors(V, F, want=["gauss", "mass_voronoi"] if area_avg else ["gauss"])
    return d.gauss / d.mass_voronoi if area_avg else d.gauss


@dataclasses.dataclass
class PrincipalCurvatures:
    """What operators.principal_curvatures returns: device tensors, None for an output that was not asked for.  k1 >= k2 are
    (nV,) fp32, d1 / d2 (nV, 3) fp32 unit directions, ring_size (nV,) int32 (the final patch size; kernels.CURV_MAX_RING + 1 where
    the search overflowed), with a leading batch axis for a batch; status is a 1-element int32 device tensor of
    kernels.DESC_BAD_FACE and kernels.CURV_* bits (of the whole batch).  A vertex that failed holds NaN."""
    k1: Optional[torch.Tensor] = None
    k2: Optional[torch.Tensor] = None
    d1: Optional[torch.Tensor] = None
    d2: Optional[torch.Tensor] = None
    ring_size: Optional[torch.Tensor] = None
    status: Optional[torch.Tensor] = None


def _mesh_tensors(who: str, V, F, device="cuda", checked: bool = False):
    """V as an fp32 and F as an int32 tensor: a tensor is cast where it is, anything else goes through numpy, is cast on the host
    and moved to `device` (F to where V is); device=None leaves it on the host, for checks that need no device.
    checked: V (nV, 3) floating point and F (nF, 3) int32 or int64 are required, ValueError for a shape and TypeError for a
    type; without it the layout checks of the caller follow."""
    v_given, f_given = torch.is_tensor(V), torch.is_tensor(F)
    if not v_given:
        V = torch.from_numpy(np.array(V, dtype=np.float32))
    if not f_given:
        F = torch.from_numpy(np.array(F))
    if checked:
        if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
            raise ValueError(f"{who} wants V (nV, 3) and F (nF, 3), got {tuple(V.shape)} and {tuple(F.shape)}")
        if F.dtype not in (torch.int32, torch.int64) or not V.is_floating_point():
            raise TypeError(f"{who} wants floating-point V and int32 or int64 F")
    V, F = V.float(), F.to(torch.int32)
    if device is not None:
        V = V if v_given else V.to(device)
        F = F if f_given else F.to(V.device)
    return V, F


def principal_curvatures(V, F, radius: int = 5, want=None) -> PrincipalCurvatures:
    """Principal curvatures and directions of a triangle mesh on the device, from a quadric fitted over the `radius`-ring patch of
    every vertex (kernels.mesh_principal_curvature; include/sn_spmm.h, "Principal curvatures", has the definition and
    mesh_ops.principal_curvatures the host statement, which the device equals bit for bit) — igl.principal_curvature of
    geom_utils.compute_curv4 in this project's own definition.  V: (nV, 3), F: (nF, 3), tensors or numpy arrays, or a batch
    V: (B, nV, 3) with F shared or (B, nF, 3): one launch sequence over the offset faces, bit-identical to the per-mesh calls.
    want: names of the PrincipalCurvatures fields to compute (None: all of them).  A vertex whose patch cannot be fitted (fewer
    than six members, more than kernels.CURV_MAX_RING, no normal, a degenerate patch) holds NaN and is reported in `status`.
    Does not synchronise."""
    V, F = _mesh_tensors("principal_curvatures", V, F)
    kernels._dev(V, F)
    Vg, Fg, B, nV, nF = _offset_batch("principal_curvatures", V, F)
    out = kernels.mesh_principal_curvature(Vg, Fg, radius, want)
    if V.dim() == 3:
        for name, (_, width) in kernels.CURVATURE_FIELDS.items():
            if out[name] is not None:
                out[name] = out[name].view((B, nV) + ((width,) if width > 1 else ()))
    return PrincipalCurvatures(**out)


def curv4(V, F, radius: int = 5):
    """geom_utils.compute_curv4 on the device: (nV, 4) fp32 columns [k1, k2, H, K] with H = (k1 + k2) / 2 and K = k1 k2 formed in
    fp32 from principal_curvatures, clipped to +-100, each column divided (in fp32) by its largest magnitude — per mesh for a
    batch, (B, nV, 4).  Where any entry is NaN it returns None after a warnings.warn naming the status bits, the reference's
    `return None`.  Synchronises (it reads whether a NaN occurred)."""
    pc = principal_curvatures(V, F, radius, want=["k1", "k2"])
    C = torch.stack([pc.k1, pc.k2, (pc.k1 + pc.k2) / 2, pc.k1 * pc.k2], dim=-1).clamp(-100.0, 100.0)
    if bool(torch.isnan(C).any()):
        status = int(pc.status.item())
        why = "; ".join(constants.status_sentences("curvature", status & ~kernels.DESC_BAD_FACE)) or "non-finite input"
        warnings.warn(f"curv4: {int(torch.isnan(pc.k1).sum())} vertices have no curvature (status {status}: {why}); no columns")
        return None
    return C / C.abs().amax(dim=-2, keepdim=True)


def laplacian_operator_from_mesh(V: torch.Tensor, F: torch.Tensor, intrinsic: bool = False, max_rounds: int = 1024,
                                 convention: str = "reference", mass: str = "barycentric", hack=None) -> SparseOperator:
    """convention="libigl": L = M^-1 C, igl.cotmatrix scaled by the inverse mass matrix (kernels.cot_laplacian_from_mesh;
    geom_utils.hacky_compute_laplacian), mass "barycentric" | "voronoi", hack: None or the value that replaces entries that are
    not finite or exceed 1e10 in magnitude; explicit zeros kept; intrinsic=True is refused with it.  `status` (DESC_* bits, a
    Python int) is set on the returned operator.  convention="reference" (default), everything below:
    L = A^-1 (D - W) built on the device (sn_laplacian_csr_from_mesh) — replaces the host pipeline
    mesh.cotangent_weights + graph.laplacian (src/mesh_mnist/add_laplacian.py:43-48).  V: (nV,3) or (B,nV,3) for a batch
    of equally sized meshes (block-diagonal result); F: (nF,3) shared or (B,nF,3).
    intrinsic=True: the same operator on the intrinsic Delaunay triangulation of the mesh (edge flips on the device,
    kernels.intrinsic_laplacian_from_mesh; include/sn_spmm.h has the definition) — what the reference calls
    mesh.intrinsic_laplacian, although NOT a reproduction of its unpublished matrix, whose scaling and sign are unknown.
    Every interior edge then has a non-negative weight.  A batch is one launch sequence over the offset faces.  Limits: the
    mesh must be manifold and consistently oriented (ValueError names what it is not), at most max_rounds parallel flip
    rounds (RuntimeError), explicit zeros are kept, no vertex-degree limit."""
    if convention not in ("reference", "libigl"):
        raise ValueError(f'laplacian_operator_from_mesh: convention must be "reference" or "libigl", got {convention!r}')
    if convention == "libigl":
        if intrinsic:
            raise ValueError('laplacian_operator_from_mesh: intrinsic=True has no convention="libigl" form')
        kernels._dev(V, F)
        Vg, Fg, B, nV, _ = _offset_batch("laplacian_operator_from_mesh", V, F)
        rowptr, colind, vals, st = kernels.cot_laplacian_from_mesh(Vg, Fg, mass, hack)
        L = SparseOperator(rowptr, colind, vals, (B * nV, B * nV), batch=B)
        L.status = st
        return L
    if mass != "barycentric" or hack is not None:
        raise ValueError('laplacian_operator_from_mesh: mass and hack belong to convention="libigl"')
    Vg, Fg, B, nV, _ = _offset_batch("laplacian_operator_from_mesh", V, F, guard=False)
    if intrinsic:
        rowptr, colind, vals = kernels.intrinsic_laplacian_from_mesh(Vg, Fg, max_rounds)
    else:
        rowptr, colind, vals = kernels.laplacian_from_mesh(Vg, Fg)
    return SparseOperator(rowptr, colind, vals, (B * nV, B * nV), batch=B)


def spgemm(A: SparseOperator, B: SparseOperator, keep_zeros: bool = False) -> SparseOperator:
    """C = A · B of two device operators in CSR (kernels.csr_spgemm; include/sn_spmm.h has the definition): every entry a
    sequential fp32 sum over A's row in ascending column order, columns ascending, bit-reproducible, exact-zero sums dropped as
    scipy's product drops them (keep_zeros=True keeps the structural pattern).  Two block-diagonal batches of the same count
    multiply block by block: the result carries `batch`.  Raises ValueError for mismatched shapes or a column out of range and
    RuntimeError for a result row wider than kernels.spgemm_max_window() columns — there is no host path."""
    if not isinstance(A, SparseOperator) or not isinstance(B, SparseOperator):
        raise TypeError("spgemm multiplies two SparseOperators")
    (M, K), (K2, N) = A._shape, B._shape
    if K != K2:
        raise ValueError(f"spgemm: shapes {A._shape} and {B._shape} do not chain")
    rp, ci, v = kernels.csr_spgemm((A.rowptr, A.colind, A.vals), (B.rowptr, B.colind, B.vals), (M, K, N), keep_zeros=keep_zeros)
    return SparseOperator(rp, ci, v, (M, N), batch=A.batch if A.batch == B.batch else 1)


def amplify_sequence_operators(L: SparseOperator):
    """[L0, L1, L2]: the operator sequence of the 'amp' tower (src/dense_correspondence/main.py:72-83) from a device Laplacian,
    in the reference's step order:  L0 = S(L);  L1 = S(L0)^2;  L2 = S(L1)^2,  S(X) = D^-1/2 X D^-1/2 (kernels.csr_scale_sym) and
    D = entries per row of L - 1, taken ONCE from L's own row lengths (explicit zeros count, as they do on the host).  L0 and L1
    are dense_correspondence.amplify_sequence's matrices bit for bit; L2 is the ascending-order sum where scipy sums its own
    unsorted rows (LABNOTES.md#spgemm).  A block-diagonal batch gives the block-diagonal of the single meshes; `batch` is
    carried over.  ValueError for a row holding only its diagonal."""
    if not isinstance(L, SparseOperator):
        raise TypeError("amplify_sequence_operators wants a SparseOperator")
    M, K = L._shape
    if M != K:
        raise ValueError(f"amplify_sequence_operators wants a square operator, got {L._shape}")
    d = kernels.csr_inv_sqrt_degree(L.rowptr)
    cur = kernels.csr_scale_sym((L.rowptr, L.colind, L.vals), d, M)
    out = [SparseOperator(*cur, (M, M), batch=L.batch)]
    for _ in range(2):
        cur = kernels.csr_scale_sym(cur, d, M)
        cur = kernels.csr_spgemm(cur, cur, (M, M, M))
        out.append(SparseOperator(*cur, (M, M), batch=L.batch))
    return out


def geodesic_matrix_from_mesh(V: torch.Tensor, F: torch.Tensor, symmetric: bool = True, require_connected: bool = True,
                              method: str = "edges") -> torch.Tensor:
    """(nV, nV) float32 matrix of shortest-path distances along the mesh edges, built on the device — the `dist_mat` the
    reference reads from its FAUST frames (src/dense_correspondence/main.py:65-104) and computes nowhere.
    The graph is the pattern of the device Laplacian (sn_laplacian_csr_from_mesh: the vertex adjacency plus the diagonal; an
    edge whose cotangent weight is exactly zero is not stored there and is not walked here) with Euclidean edge lengths;
    path lengths accumulate in fp32 from the source outward (definition and kernels: include/sn_spmm.h, sn_graph_apsp_f32).
    symmetric: min(D, D^T) — D itself differs from its transpose by ulps.  A disconnected mesh raises ValueError when
    require_connected, else keeps +inf between its components.  Synchronises (the pattern's size, the `unreached` flag).
    Raises for more than kernels.graph_apsp_max_vertices() vertices: there is no other path.
    method: "edges" (default) as above; "triangles" lets a path cross the faces — first-order Eikonal sweeps over the mesh's
    corner table (sn_mesh_corners_f32, sn_mesh_geodesics_f32; every face counts, whatever its cotangent weights), entrywise
    <= the "edges" matrix and a few fp32 ulps from bit-reproducible.  A face with a repeated or out-of-range index raises
    there; a run that has not converged after nV sweeps raises RuntimeError."""
    if method not in ("edges", "triangles"):
        raise ValueError(f'geodesic_matrix_from_mesh: method must be "edges" or "triangles", got {method!r}')
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"geodesic_matrix_from_mesh wants V (nV, 3) and F (nF, 3), got {tuple(V.shape)} and {tuple(F.shape)}")
    kernels._dev(V, F)
    nV = V.shape[0]
    if nV > kernels.graph_apsp_max_vertices():
        raise ValueError(f"geodesic_matrix_from_mesh: {nV} vertices, at most {kernels.graph_apsp_max_vertices()} are supported")
    Vf = V.float().contiguous()
    if method == "triangles":
        G, unreached = kernels.mesh_geodesics(kernels.mesh_corners(Vf, F.to(torch.int32)), nV)
    else:
        rowptr, colind, _ = kernels.laplacian_from_mesh(Vf, F.to(torch.int32))
        w = kernels.edge_lengths_csr(Vf, rowptr, colind)
        G, unreached = kernels.graph_apsp(rowptr, colind, w, nV)
    if symmetric:
        kernels.symmetrize_min_(G)
    flags = int(unreached.item())
    if flags & 2:
        raise RuntimeError(f"geodesic_matrix_from_mesh: the Eikonal sweeps had not converged after {nV} sweeps")
    if require_connected and flags & 1:
        raise ValueError("geodesic_matrix_from_mesh: the mesh is disconnected (some vertex pairs have no edge path); pass "
                         "require_connected=False to keep +inf between components")
    return G


CleanMesh = collections.namedtuple("CleanMesh", "V F vertex_map vertex_index face_map components faces_dropped vertices_dropped "
                                                 "bad_faces")


def clean_mesh(V, F, component="largest", connectivity: str = "edge") -> CleanMesh:
    """A raw scan made into a mesh the builders here accept, on the device: the faces of one connected component (or of all),
    without the faces that carry an index outside the mesh or a repeated index, and with the vertices nothing uses any more
    removed and the rest renumbered in ascending order.  Replaces the reference's off-line libigl script
    src/dense_correspondence/largest_component.py (igl.facet_components, scipy.stats.mode, igl.slice,
    igl.remove_unreferenced); kernels.mesh_components / mesh_label_mask / mesh_compact do the work, include/sn_spmm.h ("Mesh
    clean-up") has the definition and mesh_ops.largest_component the host statement.
    V: (nV, 3), F: (nF, 3), device tensors or numpy (then moved to the current device).  connectivity: "edge" (the reference's:
    faces are joined across shared edges) or "vertex".  component: "largest" — the most faces, on a tie the smallest label (in
    edge mode the component holding the lowest face index, as stats.mode picks it); "all" — every good face stays; or an integer
    label of kernels.mesh_components (the smallest face id of the component in edge mode, vertex id in vertex mode).
    Returns CleanMesh: V (nV', 3) fp32 and F (nF', 3) int32 on the device, rows of V copied bit for bit; vertex_map (nV',) new
    -> old vertex id, ascending; vertex_index (nV,) old -> new, -1 for a dropped vertex; face_map (nF',) the original index of
    every kept face, ascending; and as Python ints: components (how many were found), faces_dropped, vertices_dropped,
    bad_faces.  Synchronises once.  ValueError when the mesh has no good face or the label names no component."""
    if connectivity not in ("edge", "vertex"):
        raise ValueError(f'clean_mesh: connectivity must be "edge" or "vertex", got {connectivity!r}')
    if isinstance(component, str):
        if component not in ("largest", "all"):
            raise ValueError(f'clean_mesh: component must be "largest", "all" or an integer label, got {component!r}')
    elif isinstance(component, bool) or not isinstance(component, (int, np.integer)):
        raise TypeError(f'clean_mesh: component must be "largest", "all" or an integer label, got {component!r}')
    V, F = _mesh_tensors("clean_mesh", V, F, checked=True)
    kernels._dev(V, F)
    Vf, Fi = V.contiguous(), F.contiguous()
    nV, nF = Vf.shape[0], Fi.shape[0]
    cc = kernels.mesh_components(Fi, nV, connectivity)
    if isinstance(component, str) and component == "all":
        keep = torch.ones(nF, dtype=torch.int32, device=Fi.device)
        picked = cc.summary[2:3]
    elif isinstance(component, str):
        keep = kernels.mesh_label_mask(cc.flabel, cc.summary[1:2])       # the winner's label never leaves the device
        picked = cc.summary[2:3]
    else:
        lab = int(component)
        if not 0 <= lab < cc.count.shape[0]:
            raise ValueError(f"clean_mesh: label {lab} names no component")
        keep = kernels.mesh_label_mask(cc.flabel, torch.full((1,), lab, dtype=torch.int32, device=Fi.device))
        picked = cc.count[lab:lab + 1]
    out = kernels.mesh_compact(Fi, keep, nV, Vf)
    bad = (cc.flabel < 0).sum(dtype=torch.int32).view(1)
    nVk, nFk, ncomp, _, _, st, nbad, npicked = torch.cat([out.sizes, cc.summary, cc.status, bad, picked]).tolist()   # the one read
    kernels.raise_for_status("clean_mesh", "components", st, ((kernels.CC_INTERNAL, RuntimeError),))
    if ncomp == 0:
        raise ValueError("clean_mesh: the mesh has no face with three distinct vertices of the mesh")
    if npicked == 0:
        raise ValueError(f"clean_mesh: label {component!r} names no component")
    return CleanMesh(out.Vnew[:nVk], out.Fnew[:nFk], out.J[:nVk], out.I, out.Fsrc[:nFk], ncomp, nF - nFk, nV - nVk, nbad)


RepairedMesh = collections.namedtuple("RepairedMesh", "V F vertex_map vertex_index face_map flipped welded_vertices bad_faces "
                                                      "duplicate_faces degenerate_faces nonmanifold_edges nonorientable_classes "
                                                      "classes")


def repair_mesh(V, F, tol: float = 0.0, weld: bool = True, unique: bool = True, orient: bool = True) -> RepairedMesh:
    """A triangle soup or an inconsistently wound scan made into a mesh the builders here accept, on the device: duplicate
    vertices welded, bad and duplicate faces dropped, every component wound consistently, unused vertices removed.  The first
    step of the pipeline, before clean_mesh; replaces the reference's host-side pyigl calls (igl.remove_duplicate_vertices,
    igl.bfs_orient, the face filter of src/normal_predict/fix_degenerate.py).  kernels.mesh_weld / mesh_unique_faces /
    mesh_orient / mesh_compact do the work, include/sn_spmm.h ("Mesh repair") has the definition and mesh_ops.repair_mesh the
    host statement, which this equals bit for bit.
    V: (nV, 3), F: (nF, 3), device tensors or numpy (then moved to the current device).  tol == 0 welds vertices with equal
    coordinates (-0.0 == +0.0); tol > 0 welds the vertices in one cell of the grid rint(x / tol) — a grid, not a ball: points on
    either side of a cell border stay apart.  weld / unique / orient switch the steps off one at a time: without weld only the
    vertices with a non-finite coordinate are marked, without unique every good face stays, without orient every winding stays
    and the three orientation counts are -1.
    Returns RepairedMesh: V (nV', 3) fp32 and F (nF', 3) int32 on the device, rows of V copied bit for bit; vertex_map (nV',)
    new -> the smallest old vertex id of its class, ascending; vertex_index (nV,) old -> new, a welded vertex mapping to its
    class, -1 only for a dropped one; face_map (nF',) the original index of every kept face, ascending; flipped (nF',) int32, 1
    where the face was turned from (a, b, c) to (a, c, b); and as Python ints: welded_vertices, bad_faces (an index outside the
    mesh, a non-finite vertex or, after welding, a repeated index), duplicate_faces, degenerate_faces (kept faces of zero area on
    three distinct vertices: counted, never repaired), nonmanifold_edges (three and more faces: they link nothing),
    nonorientable_classes (left as they came) and classes.  Synchronises once."""
    tol = float(tol)
    if not 0.0 <= tol < float("inf"):
        raise ValueError(f"repair_mesh: tol must be finite and >= 0, got {tol!r}")
    V, F = _mesh_tensors("repair_mesh", V, F, checked=True)
    kernels._dev(V, F)
    Vf, Fi = V.contiguous(), F.contiguous()
    nV = Vf.shape[0]
    w = kernels.mesh_weld(Vf, Fi, tol, weld)
    u = kernels.mesh_unique_faces(w.F, nV, Vf, unique)
    words = [w.counts, u.counts, w.status, u.status]
    if orient:
        o = kernels.mesh_orient(w.F, u.keep, nV)
        Fo, flip = o.F, o.flip
        words += [o.counts, o.status]
    else:
        Fo, flip = w.F, torch.zeros(Fi.shape[0], dtype=torch.int32, device=Fi.device)
    out = kernels.mesh_compact(Fo, u.keep, nV, Vf)
    got = torch.cat([out.sizes] + words).tolist()                                         # the one read
    nVk, nFk, welded, bad, dup, flat, st_w, st_u = got[:8]
    nonman, twisted, classes, st_o = got[8:] if orient else (-1, -1, -1, 0)
    kernels.raise_for_status("repair_mesh", "repair", st_w | st_u | st_o, ((kernels.REPAIR_INTERNAL, RuntimeError),))
    face_map = out.Fsrc[:nFk]
    return RepairedMesh(out.Vnew[:nVk], out.Fnew[:nFk], out.J[:nVk], out.I[w.rep.long()], face_map, flip[face_map.long()], welded, bad,
                        dup, flat, nonman, twisted, classes)


@dataclasses.dataclass
class Delaunay2D:
    """What operators.delaunay_2d returns, int32 device tensors; one set: F (2 n, 3) and 0-d fields, a batch: F (B, 2 Nmax, 3)
    and (B,) fields.  F is canonical with -1 in the rows past nF; status holds kernels.DT_* bits (0: triangulated)."""
    F: torch.Tensor
    nF: torch.Tensor
    status: torch.Tensor
    flips: torch.Tensor
    cocircular: torch.Tensor
    rounds: torch.Tensor
    boundary: torch.Tensor

    def faces(self, b: Optional[int] = None) -> torch.Tensor:
        """The (nF, 3) faces of the set (of set b of a batch).  Reads nF: synchronises."""
        F, nF = (self.F, self.nF) if b is None else (self.F[b], self.nF[b])
        return F[: int(nF)]


def delaunay_2d(P, count=None, quantum=None, max_rounds: int = kernels.DT_MAX_ROUNDS, device="cuda") -> Delaunay2D:
    """Delaunay triangulation of 2-D point sets on the device, exact on an integer lattice (kernels.delaunay_2d; the definition
    is in include/sn_spmm.h, "Lattice Delaunay and the Mesh-MNIST maker", the host statement is mesh_ops.delaunay_2d) — the
    batched replacement of scipy.spatial.Delaunay in src/mesh_mnist/create_data.py:81.
    P: tensor or numpy, (n, 2) one set or (B, Nmax, 2) a padded batch with count (B,) (None: every set has Nmax points).  Integer
    P are lattice coordinates, |x|, |y| < 2^24.  quantum: the input (any dtype) is snapped first, rint(P / quantum) in float64;
    floating-point P needs it.  At most kernels.delaunay_max_points() points per set.  Each set gets its own status
    (kernels.DT_*): a refused set has nF = 0 and leaves its neighbours alone.  Nothing synchronises unless the caller reads."""
    Pt = P if torch.is_tensor(P) else torch.from_numpy(np.ascontiguousarray(P))
    Pt = Pt.to(device) if not Pt.is_cuda else Pt
    if Pt.dim() not in (2, 3) or Pt.shape[-1] != 2:
        raise ValueError(f"delaunay_2d wants P (n, 2) or (B, Nmax, 2), got {tuple(Pt.shape)}")
    if quantum is not None:
        q = float(quantum)
        if not (q > 0.0 and q < float("inf")):
            raise ValueError(f"delaunay_2d: quantum must be finite and > 0, got {quantum!r}")
        Pt = torch.round(Pt.to(torch.float64) / q)
        Pt = torch.where(torch.isfinite(Pt), Pt, torch.full_like(Pt, float(1 << 24)))
    elif Pt.is_floating_point():
        raise TypeError("delaunay_2d: floating-point P needs quantum= (the lattice spacing); integer P are lattice coordinates")
    lim = 1 << 24                                  # a coordinate at +-2^24 is out of range: the kernel reports DT_RANGE
    Pi = Pt.clamp(-lim, lim).to(torch.int32)
    single = Pi.dim() == 2
    if single:
        Pi = Pi.unsqueeze(0)
        count = None if count is None else torch.as_tensor([int(count)])
    if count is not None:
        count = (count if torch.is_tensor(count) else torch.from_numpy(np.asarray(count))).to(Pi.device).to(torch.int32).reshape(-1)
        if count.shape[0] != Pi.shape[0]:
            raise ValueError(f"delaunay_2d: count has {count.shape[0]} entries for {Pi.shape[0]} sets")
    r = kernels.delaunay_2d(Pi, count, max_rounds)
    f = (lambda t: t[0]) if single else (lambda t: t)
    return Delaunay2D(f(r.F), f(r.nF), f(r.status), f(r.counts[:, 0]), f(r.counts[:, 1]), f(r.counts[:, 2]), f(r.counts[:, 3]))


class PackedSegments:
    """Per-mesh row ranges of a PACKED batch (the concatenation of the meshes' node rows, no padding) — what takes the place
    of the reference's (B, Vmax, 1) `mask` tensor when a model runs on a packed batch: pass it as the `mask` argument of
    AvgResNet2 / global_average / the task models.  Holds the host lengths and, on the device, the tile table of
    sn_segment_colsum_ragged_f32 (tiles of <= 256 rows, a mesh's tiles consecutive) and 1 / vertex count per mesh."""

    TILE = 256

    def __init__(self, lengths, device="cuda"):
        self.lengths = np.asarray(lengths, dtype=np.int64)
        if self.lengths.ndim != 1 or (self.lengths < 1).any():
            raise ValueError("PackedSegments: one positive row count per mesh")
        self.nseg = int(len(self.lengths))
        self.offsets = np.zeros(self.nseg + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=self.offsets[1:])
        self.rows = int(self.offsets[-1])
        per = (self.lengths + self.TILE - 1) // self.TILE
        seg_tile_ptr = np.zeros(self.nseg + 1, dtype=np.int64)
        np.cumsum(per, out=seg_tile_ptr[1:])
        seg = np.repeat(np.arange(self.nseg), per)
        k = np.arange(int(seg_tile_ptr[-1])) - seg_tile_ptr[seg]                   # tile index inside its mesh
        first = self.offsets[seg] + k * self.TILE
        cnt = np.minimum(self.TILE, self.offsets[seg + 1] - first)
        self.device = torch.device(device)
        self.tiles = h2d_async(np.stack([seg, first, cnt], axis=1), self.device)
        self.seg_tile_ptr = h2d_async(seg_tile_ptr, self.device)
        self.inv_count = h2d_async((1.0 / self.lengths).astype(np.float32), self.device)
        self.off_dev = h2d_async(self.offsets, self.device)                        # (nseg + 1,) int64: first row of every mesh
        # row slabs of the weight-gradient pass (sn_wgrad_slabs_f32): about 256 in all, none crossing a mesh boundary
        target = max(256, -(-self.rows // 256))
        nsl = np.maximum(1, -(-self.lengths // target))
        slab_ptr = np.zeros(self.nseg + 1, dtype=np.int64)
        np.cumsum(nsl, out=slab_ptr[1:])
        sseg = np.repeat(np.arange(self.nseg), nsl)
        sk = np.arange(int(slab_ptr[-1])) - slab_ptr[sseg]
        per = -(-self.lengths // nsl)
        per = (per + 15) // 16 * 16
        s0 = np.minimum(self.offsets[sseg] + sk * per[sseg], self.offsets[sseg + 1])
        self.nslab = int(slab_ptr[-1])
        self.slab_off = h2d_async(np.concatenate([s0, self.offsets[-1:]]), self.device)
        self.seg_slab_ptr = h2d_async(slab_ptr, self.device)
        self.len_f64 = h2d_async(self.lengths.astype(np.float64), self.device)
        self.min_len = int(self.lengths.min())

    _recent = {}

    @classmethod
    def cached(cls, lengths, device="cuda") -> "PackedSegments":
        """The segments of `lengths`, re-used when the same sizes come back (a sampler that draws the same meshes every step
        would otherwise upload the eight small tables again per step); holds the last 16 distinct size lists."""
        key = (tuple(int(v) for v in lengths), str(torch.device(device)))
        hit = cls._recent.get(key)
        if hit is None:
            if len(cls._recent) >= 16:
                cls._recent.pop(next(iter(cls._recent)))
            hit = cls._recent[key] = cls(lengths, device)
        return hit

    @classmethod
    def of_operator(cls, op: "SparseOperator", group: int = 1, side: str = "cols") -> "PackedSegments":
        """Row ranges of the dense operand of a packed operator: its column blocks (`side="cols"`, the input side) or its
        row blocks, divided by `group` (4 for the quaternion view of the Dirac operators)."""
        off = op.col_offsets if side == "cols" else op.row_offsets
        if off is None:
            raise ValueError("not a packed operator (OperatorPool.assemble(sel) without sizes)")
        return cls(np.diff(off) // group, op.device)

    def mean(self, x2d: torch.Tensor) -> torch.Tensor:
        """(nseg, C): per-mesh column means of the (rows, C) operand."""
        if x2d.shape[0] != self.rows:
            raise ValueError(f"PackedSegments: {self.rows} rows expected, got {x2d.shape[0]}")
        return kernels.segment_colsum_ragged(x2d, self.tiles, self.seg_tile_ptr, self.nseg, self.inv_count)

    # ---- the global-average stage on this layout (functional.avg_stage_forward / avg_stage_backward; MaskedSegments has the same) ----
    stats_from_partials = True    # stage_stats starts from the statistics partials alone: the stage GEMMs always leave them

    def stage_supported(self, C: int, J: int) -> bool:
        return kernels.avg_stage_ragged_supported(C, J, self)

    def stage_stats(self, e, e_tiles=None, part=None):
        """(m, stats): per-mesh means of e and the BatchNorm statistics of [e | mean broadcast] (mesh i contributes len_i·m_i and
        len_i·m_i²).  e_tiles: the (tile sums, partials) the GEMM that wrote e left — no pass over e at all; part: its statistics
        partials alone — the means take one pass, the statistics none; neither: one more pass over e, handed on as one block."""
        if e_tiles is not None:
            return kernels.avg_stats_from_tiles_ragged(e_tiles[0], e_tiles[1], e, self)
        m = self.mean(e).contiguous()
        C = e.shape[1]
        if part is not None and C == 128:
            return m, kernels.avg_stats_ragged(m, self, part, kernels.linear_fwd_stats_blocks(e.shape[0]))
        return m, kernels.avg_stats_ragged(m, self, kernels.colstats(e).reshape(1, 2, C), 1)

    def linear_fwd_segbias(self, e, W, segb, *epilogue):
        return kernels.linear_fwd_segbias_ragged(e, W, segb, self, *epilogue)

    def wgrad(self, dy, e, center, bounds):
        return kernels.wgrad_slabs(dy, e, center, self, bounds=bounds)

    def avg_bn_bwd(self, G1, sdy, Sg, m, *layer):
        return kernels.avg_bn_bwd(G1, sdy, Sg, m.contiguous(), *layer, self.inv_count, segoff=self.off_dev)

    def bwd_segvec(self, *terms):
        return kernels.avg_bwd_segvec_ragged(*terms, self)

    def dgrad_eluseg(self, dy, W, e, center, B, Cc, segvec, gadd):
        return kernels.linear_dgrad_eluseg_ragged(dy, W, e, center, B, Cc, segvec, self, gadd)

    def bcast(self, src, dst) -> None:
        """dst[r, :] = src[mesh(r), :]."""
        kernels.bcast_rows_ragged(src, self.tiles, dst)

    def elu_bwd_mean(self, g_e, g_m, e, g_x) -> None:
        """g_x = (g_e + the gradient the mesh's mean receives from g_m, the gradient of its broadcast, per row) * elu'(e)."""
        gb = torch.empty_like(g_x)
        self.bcast(self.mean(g_m), gb)                            # (sum over the mesh's rows of d/d(mean)) / count
        kernels.elu_bwd(g_e, e, g_x, False, gb)

    def plan_view(self):
        """(device tables, layout key): what a launch plan takes as operands / what tells two layouts apart in a plan's key."""
        return (self.tiles, self.seg_tile_ptr, self.inv_count, self.off_dev, self.slab_off, self.seg_slab_ptr, self.len_f64), \
            ("packed", self.nseg, self.rows, self.nslab, self.min_len, int(self.tiles.shape[0]))


class MaskedSegments:
    """The meshes of a PADDED batch — B meshes of V rows each, real rows marked by the reference's (B, V, 1) `mask` — with the
    same global-average stage methods as PackedSegments: the flattened mask, 1 / vertex count per mesh and the row period."""

    stats_from_partials = False   # stage_stats needs the producer's tile sums too: without them the GEMM is not asked for partials

    def __init__(self, mask: torch.Tensor, B: int, V: int):
        self.nseg, self.rows_per_seg, self.rows = B, V, B * V
        self.mask_rows = mask.reshape(self.rows).contiguous()
        self.inv_count = 1.0 / mask.reshape(B, V).sum(1, keepdim=True)

    def mean(self, x2d: torch.Tensor) -> torch.Tensor:
        """(nseg, C): per-mesh masked column means of the (rows, C) operand."""
        return kernels.segment_colsum(x2d, self.mask_rows, self.rows_per_seg, self.nseg) * self.inv_count

    def stage_supported(self, C: int, J: int) -> bool:
        return kernels.avg_stage_supported(C, J, self.rows_per_seg)

    def stage_stats(self, e, e_tiles=None, part=None):
        """(m, stats) as PackedSegments.stage_stats (padding rows count in the statistics, as in the reference): from the producer's
        tile sums and partials, else one pass over e."""
        if e_tiles is not None:
            return kernels.avg_stats_from_tiles(e_tiles[0], e_tiles[1], e, self.mask_rows, self.inv_count, self.rows_per_seg, self.nseg)
        return kernels.avg_stats(e, self.mask_rows, self.inv_count, self.rows_per_seg, self.nseg)

    def linear_fwd_segbias(self, e, W, segb, *epilogue):
        return kernels.linear_fwd_segbias(e, W, segb, self.rows_per_seg, *epilogue)

    def wgrad(self, dy, e, center, bounds):
        return kernels.wgrad_seg(dy, e, center, self.rows_per_seg, bounds=bounds)

    def avg_bn_bwd(self, *terms):
        return kernels.avg_bn_bwd(*terms, self.inv_count, rows_per_seg=self.rows_per_seg)

    def bwd_segvec(self, *terms):
        return kernels.avg_bwd_segvec(*terms, self.inv_count, self.rows_per_seg)

    def dgrad_eluseg(self, dy, W, e, center, B, Cc, segvec, gadd):
        return kernels.linear_dgrad_eluseg(dy, W, e, center, B, Cc, segvec, self.rows_per_seg, self.mask_rows, gadd)

    def bcast(self, src, dst) -> None:
        kernels.bcast_rows(src, dst, self.rows_per_seg)

    def elu_bwd_mean(self, g_e, g_m, e, g_x) -> None:
        gm = kernels.segment_colsum(g_m, None, self.rows_per_seg, self.nseg) * self.inv_count      # d/d(mean) / count
        kernels.elu_bwd_bcast(g_e, e, gm.contiguous(), self.mask_rows, g_x, self.rows_per_seg)

    def plan_view(self):
        return (self.mask_rows, self.inv_count), ("masked", self.nseg, self.rows_per_seg, self.mask_rows.dtype)


def as_operator(A) -> SparseOperator:
    """Normalise whatever the reference drivers pass as L / Di / DiA (SparseOperator, torch sparse COO 2-D or
    3-D) to a SparseOperator.  The converted form is cached on the tensor object, so one operator that feeds
    several residual blocks in a step (and their backward passes) is converted once."""
    if isinstance(A, SparseOperator):
        return A
    if isinstance(A, torch.Tensor) and A.layout == torch.sparse_coo:
        cached = getattr(A, "_sn_operator", None)
        if cached is None:
            cached = SparseOperator.from_torch_coo(A)
            A._sn_operator = cached
        return cached
    raise TypeError(f"cannot interpret {type(A)} as a sparse operator")


def h2d_async(arr, device) -> torch.Tensor:
    """Small host array -> device tensor WITHOUT stalling the host on the stream: staged through pinned memory (torch's
    caching host allocator keeps the staging block alive until the copy has run), so the per-step index / descriptor
    uploads of the samplers do not wait for the previous step's kernels — a pageable-source copy does."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    dev = torch.device(device)
    if dev.type != "cuda":
        return t.to(dev, non_blocking=True)
    stage = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    stage.copy_(t)
    return stage.to(dev, non_blocking=True)


class OperatorPool:
    """All per-mesh operators of one kind (e.g. every Di of a dataset) resident in HBM, A and A^T.

    `assemble(sel, size0, size1)` returns the batched block-diagonal SparseOperator of the selected meshes —
    identical (after to_dense) to the reference's `sparse_diag_cat([op[i] for i in sel], size0, size1)` — with its
    transpose attached, so neither forward nor backward ever sorts, transposes or touches the host.
    """

    def __init__(self, mats: Sequence, device="cuda", want_bsr4: bool = False, lean: bool = False):
        """lean=True: keep only the arrays batches are assembled from — for pools of Dirac operators that turn out to be
        quaternion-packed, the pooled CSR and BSR4 device arrays are dropped (the CSR entry counts stay on the host)."""
        self.device = torch.device(device)
        self.n = len(mats)
        self.want_bsr4 = bool(want_bsr4)
        self.lean = bool(lean)
        fwd = [m.tocsr() for m in mats]
        for m in fwd:
            m.sort_indices()
        self.rows = np.array([m.shape[0] for m in fwd], dtype=np.int64)
        self.cols = np.array([m.shape[1] for m in fwd], dtype=np.int64)
        self._fwd = self._upload(fwd)
        self._bwd = self._upload([m.T.tocsr() for m in fwd])   # one-time host transpose at load, like the dataset prep
        # per mesh: (max |column - row|, longest row, rows outside the ring window) of the operator and of its transpose — a
        # batch whose blocks sit on the diagonal (equal row and column offsets) inherits them without a device pass
        self._band_fwd = np.array([self._mesh_band(m) for m in fwd], dtype=np.int64).reshape(-1, 3)
        self._band_bwd = np.array([self._mesh_band(m.T.tocsr()) for m in fwd], dtype=np.int64).reshape(-1, 3)
        self._fwd_b = self._bwd_b = None
        self._fwd_q = self._bwd_q = None
        if self.want_bsr4:
            self._fwd_b = self._pool_bsr4(self._fwd, self.rows, self.cols)
            self._bwd_b = self._pool_bsr4(self._bwd, self.cols, self.rows)
            # quaternion-packed pools when every block of every mesh is a pure-quaternion matrix (Dirac operators are)
            fq, ff = kernels.bsr4_to_q3(self._fwd_b["colind"], self._fwd_b["vals"])
            bq, bf = kernels.bsr4_to_q3(self._bwd_b["colind"], self._bwd_b["vals"])
            if int(ff.item()) == 0 and int(bf.item()) == 0:
                self._fwd_q = dict(self._fwd_b, vals=fq.reshape(-1), colind=None)
                self._bwd_q = dict(self._bwd_b, vals=bq.reshape(-1), colind=None)
            if self.lean and self._fwd_q is not None:
                self._fwd_b = self._bwd_b = None
                for pool in (self._fwd, self._bwd):
                    pool["rowptr"] = pool["colind"] = pool["vals"] = None

    # ---- growing pools (utils_pt's resident cache appends the operators a driver shows it for the first time) -----------
    @staticmethod
    def _arena_append(buf, used: int, new):
        """`new` copied behind the first `used` elements of `buf`; the buffer doubles when it is full (offsets into it stay
        valid: the assembly kernels address pooled arrays by element offsets, never by their length)."""
        need = used + int(new.numel())
        if buf is None or need > buf.numel():
            cap = max(need, 2 * (int(buf.numel()) if buf is not None else 0), 1 << 16)
            grown = torch.empty(cap, dtype=new.dtype, device=new.device)
            if used:
                grown[:used].copy_(buf[:used])
            buf = grown
        buf[used:need].copy_(new.reshape(-1))
        return buf

    @classmethod
    def _merge(cls, dst, src, vpe: int):
        if src is None or dst is None:
            return None
        used_rp, used_e = int(dst["rp_off"][-1]), int(dst["e_off"][-1])
        for key, used, n_src in (("rowptr", used_rp, int(src["rp_off"][-1])), ("colind", used_e, int(src["e_off"][-1])),
                                 ("vals", used_e * vpe, int(src["e_off"][-1]) * vpe)):
            if dst[key] is not None and src[key] is not None:
                dst[key] = cls._arena_append(dst[key], used, src[key][:n_src])
        dst["rp_off"] = np.concatenate([dst["rp_off"], used_rp + src["rp_off"][1:]])
        dst["e_off"] = np.concatenate([dst["e_off"], used_e + src["e_off"][1:]])
        dst["cnt"] = np.diff(dst["e_off"])
        return dst

    def append(self, mats: Sequence) -> np.ndarray:
        """Add operators to the pool (converted like the constructor's: one-time host transpose, device BSR4 / quaternion
        packing); returns their indices for assemble().  A pool that was quaternion-packed stays so only while every added
        operator is — the caller (utils_pt's resident cache) keeps such operators in a pool of their own."""
        if not len(mats):
            return np.zeros(0, dtype=np.int64)
        return self.absorb(OperatorPool(mats, self.device, self.want_bsr4, self.lean))

    def absorb(self, chunk: "OperatorPool") -> np.ndarray:
        """Merge another pool of the same kind into this one (its arrays are copied behind this pool's); returns the indices
        its operators now have here."""
        if chunk.want_bsr4 != self.want_bsr4 or chunk.device != self.device:
            raise ValueError("OperatorPool.absorb: pools of different kinds")
        if (chunk._fwd_q is None) != (self._fwd_q is None) or (chunk._fwd_b is None) != (self._fwd_b is None):
            raise ValueError("OperatorPool.append: the new operators do not pack the way this pool's do")
        first = self.n
        self._fwd = self._merge(self._fwd, chunk._fwd, 1)
        self._bwd = self._merge(self._bwd, chunk._bwd, 1)
        fwd_rowptr_shared = self._fwd_q is not None and self._fwd_b is not None
        self._fwd_b = self._merge(self._fwd_b, chunk._fwd_b, 16)
        self._bwd_b = self._merge(self._bwd_b, chunk._bwd_b, 16)
        if fwd_rowptr_shared:                                 # (the quaternion dicts share block-row pointers and offsets)
            for q, b, cq in ((self._fwd_q, self._fwd_b, chunk._fwd_q), (self._bwd_q, self._bwd_b, chunk._bwd_q)):
                used = int(q["e_off"][-1])
                q["vals"] = self._arena_append(q["vals"], used * 4, cq["vals"][: int(cq["e_off"][-1]) * 4])
                q["rowptr"], q["rp_off"], q["e_off"], q["cnt"] = b["rowptr"], b["rp_off"], b["e_off"], b["cnt"]
        else:
            self._fwd_q = self._merge(self._fwd_q, chunk._fwd_q, 4)
            self._bwd_q = self._merge(self._bwd_q, chunk._bwd_q, 4)
        self.rows = np.concatenate([self.rows, chunk.rows])
        self.cols = np.concatenate([self.cols, chunk.cols])
        self._band_fwd = np.concatenate([self._band_fwd, chunk._band_fwd])
        self._band_bwd = np.concatenate([self._band_bwd, chunk._band_bwd])
        self.n += chunk.n
        return np.arange(first, self.n, dtype=np.int64)

    def device_bytes(self) -> int:
        tot = 0
        seen = set()
        for pool in (self._fwd, self._bwd, self._fwd_b, self._bwd_b, self._fwd_q, self._bwd_q):
            for key in ("rowptr", "colind", "vals"):
                t = pool[key] if pool is not None else None
                if t is not None and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    tot += t.numel() * t.element_size()
        return tot

    @staticmethod
    def _mesh_band(m):
        m = m.tocsr()
        if m.nnz == 0:
            return (0, 0, 0)
        counts = np.diff(m.indptr)
        rows = np.repeat(np.arange(m.shape[0]), counts)
        far = np.abs(m.indices.astype(np.int64) - rows)
        outside = np.unique(rows[far > kernels.ring_half_window()]).size if far.max() > 0 else 0
        return (int(far.max()), int(counts.max()), int(outside))

    def _attach_band(self, op, sel, diagonal: bool):
        if diagonal and len(sel):
            f, b = self._band_fwd[sel], self._band_bwd[sel]
            op._band = (int(f[:, 0].max()), int(f[:, 1].max()), int(f[:, 2].sum()))
            if op._t is not None:
                op._t._band = (int(b[:, 0].max()), int(b[:, 1].max()), int(b[:, 2].sum()))

    # pooled CSR: dict(rowptr, colind, vals device tensors; rp_off, e_off, cnt host int64 arrays)
    def _upload(self, mats):
        for m in mats:
            m.sort_indices()
        rp_off = np.zeros(len(mats) + 1, dtype=np.int64)
        e_off = np.zeros(len(mats) + 1, dtype=np.int64)
        for i, m in enumerate(mats):
            rp_off[i + 1] = rp_off[i] + m.shape[0] + 1
            e_off[i + 1] = e_off[i] + m.nnz
        cat = lambda parts, dt: torch.from_numpy(np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)).to(self.device)
        return {
            "rowptr": cat([m.indptr for m in mats], np.int32),
            "colind": cat([m.indices for m in mats], np.int32),
            "vals": cat([m.data for m in mats], np.float32),
            "rp_off": rp_off, "e_off": e_off, "cnt": np.diff(e_off),
        }

    def _pool_bsr4(self, pool, rows, cols):
        """Convert each pooled mesh to BSR4 on the device, then re-pool (runs once per dataset)."""
        parts = []
        for i in range(self.n):
            rp = pool["rowptr"][pool["rp_off"][i]: pool["rp_off"][i + 1]]
            sl = slice(int(pool["e_off"][i]), int(pool["e_off"][i + 1]))
            parts.append(kernels.csr_to_bsr4(rp, pool["colind"][sl], pool["vals"][sl], int(rows[i]), int(cols[i])))
        rp_off = np.zeros(self.n + 1, dtype=np.int64)
        e_off = np.zeros(self.n + 1, dtype=np.int64)
        for i, (brp, bci, _) in enumerate(parts):
            rp_off[i + 1] = rp_off[i] + brp.numel()
            e_off[i + 1] = e_off[i] + bci.numel()
        return {
            "rowptr": torch.cat([p[0] for p in parts]), "colind": torch.cat([p[1] for p in parts]),
            "vals": torch.cat([p[2] for p in parts]), "rp_off": rp_off, "e_off": e_off, "cnt": np.diff(e_off),
        }

    def _concat(self, pool, sel, nrows, size0, size1, vpe):
        cnt = pool["cnt"][sel]
        out_off = np.zeros(len(sel) + 1, dtype=np.int64)
        np.cumsum(cnt, out=out_off[1:])
        desc = np.stack([pool["rp_off"][sel], pool["e_off"][sel], nrows, out_off[:-1]], axis=1)
        desc_d = h2d_async(desc, self.device)
        return kernels.blockdiag_concat(pool["rowptr"], pool["colind"], pool["vals"], desc_d, size0, size1,
                                        int(out_off[-1]), vpe)

    def _concat_ragged(self, pool, sel, nrows, row_off, col_off, vpe):
        cnt = pool["cnt"][sel]
        out_off = np.zeros(len(sel) + 1, dtype=np.int64)
        np.cumsum(cnt, out=out_off[1:])
        desc = np.stack([pool["rp_off"][sel], pool["e_off"][sel], nrows, out_off[:-1], row_off[:-1], col_off[:-1]], axis=1)
        desc_d = h2d_async(desc, self.device)
        return kernels.blockdiag_concat_ragged(pool["rowptr"], pool["colind"], pool["vals"], desc_d, int(row_off[-1]),
                                               int(col_off[-1]), int(out_off[-1]), vpe)

    def assemble_packed(self, sel) -> SparseOperator:
        """The batch WITHOUT padding: mesh i owns rows [row_offsets[i], row_offsets[i+1]) and columns
        [col_offsets[i], col_offsets[i+1]) (prefix sums of the meshes' own sizes), so the dense operands are the plain
        concatenation of the meshes' node rows — (sum V_i, C) instead of the reference's (B, Vmax, C)
        (src/as_rigid_as_possible/main.py:172-185 pads to the batch maxima).  The product then neither scans padding rows
        nor writes zeros into them.  The offsets (host int64 arrays, length B+1) ride on the operator."""
        sel = np.asarray(sel, dtype=np.int64)
        B = len(sel)
        rows, cols = self.rows[sel], self.cols[sel]
        ro = np.zeros(B + 1, dtype=np.int64)
        co = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(rows, out=ro[1:])
        np.cumsum(cols, out=co[1:])
        shape = (int(ro[-1]), int(co[-1]))
        if self.want_bsr4:
            if (rows % 4).any() or (cols % 4).any():
                raise ValueError("BSR4 pools need every mesh's sizes to be multiples of 4")
            if self._fwd_q is not None and (_POOL_FORMAT == "q3" or self._fwd_b is None):
                fr, _, fq = self._concat_ragged(self._fwd_q, sel, rows // 4, ro // 4, co // 4, 4)
                br_, _, bq = self._concat_ragged(self._bwd_q, sel, cols // 4, co // 4, ro // 4, 4)
                op = SparseOperator.from_q3((fr, fq.view(-1, 4)), (br_, bq.view(-1, 4)), shape, batch=B)
            else:
                fb = self._concat_ragged(self._fwd_b, sel, rows // 4, ro // 4, co // 4, 16)
                bb = self._concat_ragged(self._bwd_b, sel, cols // 4, co // 4, ro // 4, 16)
                op = SparseOperator.from_bsr4(fb, bb, shape, batch=B)
            op._nnz_cache = op._t._nnz_cache = int(self._fwd["cnt"][sel].sum())
        else:
            f = self._concat_ragged(self._fwd, sel, rows, ro, co, 1)
            b = self._concat_ragged(self._bwd, sel, cols, co, ro, 1)
            op = SparseOperator(*f, shape, batch=B)
            opt = SparseOperator(*b, (shape[1], shape[0]), batch=B, transpose=op)
            op._t = opt
            op._bsr4 = opt._bsr4 = False
            self._attach_band(op, sel, bool((rows == cols).all()))
        op.row_offsets, op.col_offsets = ro, co
        op._t.row_offsets, op._t.col_offsets = co, ro
        return op

    def assemble(self, sel, size0: Optional[int] = None, size1: Optional[int] = None) -> SparseOperator:
        """size0/size1 = the padded block size of the reference's sparse_diag_cat; both None: packed (assemble_packed)."""
        if size0 is None and size1 is None:
            return self.assemble_packed(sel)
        if size0 is None or size1 is None:
            raise ValueError("assemble: give both block sizes (padded batch) or neither (packed batch)")
        sel = np.asarray(sel, dtype=np.int64)
        B = len(sel)
        rows, cols = self.rows[sel], self.cols[sel]
        if (rows > size0).any() or (cols > size1).any():
            raise ValueError("size0/size1 smaller than a selected mesh")
        if self.want_bsr4:
            # Dirac pools: only the packed blocks are assembled per step (the products use them exclusively); the CSR
            # view of the batch is expanded from the blocks on demand (export / generic-kernel fallback).
            if size0 % 4 or size1 % 4:
                raise ValueError("BSR4 pools need size0 and size1 to be multiples of 4")
            if self._fwd_q is not None and (_POOL_FORMAT == "q3" or self._fwd_b is None):
                fr, _, fq = self._concat(self._fwd_q, sel, rows // 4, size0 // 4, size1 // 4, 4)
                br_, _, bq = self._concat(self._bwd_q, sel, cols // 4, size1 // 4, size0 // 4, 4)
                op = SparseOperator.from_q3((fr, fq.view(-1, 4)), (br_, bq.view(-1, 4)), (B * size0, B * size1), batch=B)
            else:
                fb = self._concat(self._fwd_b, sel, rows // 4, size0 // 4, size1 // 4, 16)
                bb = self._concat(self._bwd_b, sel, cols // 4, size1 // 4, size0 // 4, 16)
                op = SparseOperator.from_bsr4(fb, bb, (B * size0, B * size1), batch=B)
            op._nnz_cache = op._t._nnz_cache = int(self._fwd["cnt"][sel].sum())      # entries of the pooled CSR: no sync
            return op
        f = self._concat(self._fwd, sel, rows, size0, size1, 1)
        b = self._concat(self._bwd, sel, cols, size1, size0, 1)
        op = SparseOperator(*f, (B * size0, B * size1), batch=B)
        opt = SparseOperator(*b, (B * size1, B * size0), batch=B, transpose=op)
        op._t = opt
        op._bsr4 = opt._bsr4 = False
        self._attach_band(op, sel, size0 == size1)
        return op


ArapDeformation = collections.namedtuple("ArapDeformation", "frames cg_iters energy status")


def arap_deform(V0, F, handles, H, iters: int = 2, tol: float = 1e-10, max_cg: int = 4096) -> ArapDeformation:
    """As-rigid-as-possible deformation sequences on the device: spokes-only ARAP (Sorkine & Alexa 2007), local and global steps
    alternating `iters` times per frame, the global step by Jacobi-preconditioned CG, fp64 inside, frames rounded once to fp32.
    include/sn_spmm.h ("ARAP deformation") has the definition, mesh_ops.arap_deform the host statement, which this equals bit
    for bit; kernels.arap_weights / arap_frames do the work.  The textbook algorithm with this project's weights — not a
    reproduction of the reference's downloaded sequences, whose generator is not in its tree.
    V0 (nV, 3) rest mesh, F (nF, 3), handles (nH,) distinct vertex ids, H (T, nH, 3) their positions in every frame; or a batch
    of equally sized meshes (B, nV, 3), (B, nF, 3), (B, nH), (B, T, nH, 3).  Device tensors or numpy (then moved to the current
    device).  Frame t starts from frame t - 1, frame 0 from V0.
    Returns ArapDeformation of device tensors: frames (T, nV, 3) fp32, cg_iters (T, iters) int32, energy (T,) fp64 after the last
    step of every frame, status () int32 — each with a leading B for a batch.  ValueError for a handle out of range or repeated,
    and for a mesh in which a connected component (a vertex no face uses is one) has no handle; a warning with the reason when a
    status bit comes back.  Synchronises (the checks and the status are read).  A CPU tensor is refused as
    everywhere in this package; a numpy array is checked on the host and then uploaded."""
    def tensor(a, dtype):      # numpy stays on the host until the checks that need no device have passed
        return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.array(a)).to(dtype)

    given = (V0, F, handles, H)
    (V0, F), handles, H = _mesh_tensors("arap_deform", V0, F, device=None), tensor(handles, torch.int32), tensor(H, torch.float32)
    single = V0.dim() == 2
    if single:
        V0, F, handles, H = V0[None], F[None], handles[None], H[None]
    if (V0.dim() != 3 or V0.shape[2] != 3 or F.dim() != 3 or F.shape[2] != 3 or handles.dim() != 2 or H.dim() != 4 or H.shape[3] != 3
            or not V0.shape[0] == F.shape[0] == handles.shape[0] == H.shape[0] or H.shape[2] != handles.shape[1]):
        raise ValueError(f"arap_deform wants V0 (nV, 3), F (nF, 3), handles (nH,), H (T, nH, 3), or all four with a leading batch "
                         f"dimension; got {tuple(V0.shape)}, {tuple(F.shape)}, {tuple(handles.shape)}, {tuple(H.shape)}")
    B, nV, nH, T = V0.shape[0], V0.shape[1], handles.shape[1], H.shape[1]
    if nH < 1:
        raise ValueError("arap_deform: at least one handle is required")
    if nV > kernels.arap_max_vertices():
        raise ValueError(f"arap_deform: {nV} vertices, at most {kernels.arap_max_vertices()} are supported")
    hs = handles.sort(dim=1).values
    ok_range, ok_distinct = torch.stack([((handles >= 0) & (handles < nV)).all(), (hs[:, 1:] != hs[:, :-1]).all()]).tolist()
    if not ok_range:
        raise ValueError(f"arap_deform: a handle lies outside 0..{nV - 1}")
    if not ok_distinct:
        raise ValueError("arap_deform: a handle is repeated")
    V0, F, handles, H = (t if torch.is_tensor(g) else t.to("cuda") for t, g in zip((V0, F, handles, H), given))
    kernels._dev(V0, F, handles, H)
    dev = V0.device
    Vu, Fu = _offset_batch("arap_deform", V0, F, guard=False)[:2]
    voff, hoff = _mesh_offsets(B + 1, nV, dev), _mesh_offsets(B + 1, nH, dev)
    hu = (handles + voff[:B, None]).reshape(-1).contiguous()
    cc = kernels.mesh_components(Fu, B * nV, "vertex")
    has = torch.zeros(B * nV, dtype=torch.bool, device=dev)
    has[cc.vlabel[hu.long()].long()] = True
    if not bool(has[cc.vlabel.long()].all()):
        raise ValueError("arap_deform: a connected component of the mesh has no handle (its positions are not determined)")
    weights = kernels.arap_weights(Vu, Fu)
    Hu = H.permute(1, 0, 2, 3).reshape(T, B * nH, 3).contiguous()
    out = kernels.arap_frames(Vu, weights, voff, hoff, hu, Hu, nV, iters, tol, max_cg)
    status = out.status | weights.status          # the builder's word covers the union
    bits = 0
    for word in status.tolist():
        bits |= word
    for reason in constants.status_sentences("arap", bits):
        warnings.warn(f"arap_deform: {reason}", RuntimeWarning, stacklevel=2)
    frames = out.frames.reshape(T, B, nV, 3).permute(1, 0, 2, 3).contiguous()
    if single:
        return ArapDeformation(frames[0], out.cg_iters[0], out.energy[0], status[0])
    return ArapDeformation(frames, out.cg_iters, out.energy, status)


@dataclasses.dataclass
class Eigenpairs:
    """What operators.laplacian_eigenpairs returns: fp64 device tensors over the B meshes of the call.  values (B, k) ascending;
    vectors (n, k) with phi^T diag(mass) phi = I inside every mesh, n the rows of the whole batch; residuals (B, k) of the
    standard form A = D S D; bound (B,) its Gershgorin bound b; outer_iterations (B,) int64; mass (n,) = Am, the clipped and
    normalised Voronoi mass; voff (B + 1,) int32, the first row of every mesh; status a Python int of kernels.DESC_* and
    kernels.EIG_* bits (of the whole batch)."""
    values: torch.Tensor
    vectors: torch.Tensor
    residuals: torch.Tensor
    bound: torch.Tensor
    outer_iterations: torch.Tensor
    mass: torch.Tensor
    voff: torch.Tensor
    status: int


# The m x m eigh of the Rayleigh-Ritz step: torch.linalg.eigh in fp64 on the device (LABNOTES.md#spectral says what was measured);
# True moves that one factorisation, at most about 1 MB per outer iteration, to the host.
_EIGH_ON_HOST = False


def _sym_eigh(H: torch.Tensor):
    if _EIGH_ON_HOST:
        w, Q = np.linalg.eigh(H.cpu().numpy())
        return torch.from_numpy(w).to(H.device), torch.from_numpy(Q).to(H.device)
    return torch.linalg.eigh(H)


def _spectral_layout(who: str, V, F, sizes):
    """(Vg, Fg, B, voff as a list): a single mesh, a batch through _offset_batch, or a ragged batch given as one disjoint mesh
    with the vertex counts of its parts."""
    if not torch.is_tensor(V) or not torch.is_tensor(F) or not V.is_cuda or not F.is_cuda:
        raise ValueError(f"{who} wants V and F as device tensors (there is no host path in this package; mesh_ops has the statement)")
    if sizes is None:
        Vg, Fg, B, nV, _ = _offset_batch(who, V, F)
        return Vg, Fg, B, [b * nV for b in range(B + 1)]
    sizes = [int(x) for x in sizes]
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3 or not sizes or min(sizes) < 0 or sum(sizes) != V.shape[0]:
        raise ValueError(f"{who}: with sizes, V (n, 3) and F (nF, 3) hold the meshes as one disjoint mesh and the sizes add up to n; "
                         f"got {tuple(V.shape)}, {tuple(F.shape)} and {sizes}")
    return V.float(), F.to(torch.int32), len(sizes), [0] + [int(x) for x in np.cumsum(sizes)]


def laplacian_eigenpairs(V, F, k: int = 300, guard: Optional[int] = None, deg: int = 24, tol: float = 1e-10, max_outer: int = 40,
                         seed: int = 0, sizes: Optional[Sequence[int]] = None) -> Eigenpairs:
    """The k lowest eigenpairs S phi = lambda diag(Am) phi of the cotangent pencil of every mesh, on the device: what
    geom_utils.compute_wks takes from scipy's shift-invert eigsh(-L, M=Am, sigma=-1e-5, k=300), and the basis of any spectral
    descriptor.  Chebyshev-filtered subspace iteration (Zhou & Saad's scaled filter) on the standard form A = D S D,
    D = Am^-1/2: include/sn_spmm.h ("Spectral") has the steps, mesh_ops.laplacian_eigenpairs the numpy statement with the same
    steps and parameters.  The pencil (kernels.cot_pencil_from_mesh), the start block and every product with A
    (kernels.cheb_filter_step: deg launches per filter, per-mesh scalars read on the device) are this package's kernels; QR,
    X^T A X, eigh and the rotations are torch's fp64 linear algebra, mesh by mesh.
    V (nV, 3) and F (nF, 3); a batch V (B, nV, 3) with F shared or (B, nF, 3); or, with sizes, a ragged batch laid out as one
    disjoint mesh whose parts have these vertex counts.  Am = max(M_voronoi, 1e-8) normalised to sum 1 per mesh.
    m = min(smallest mesh, k + guard) columns, guard = max(16, k // 8) by default.  Converged when every residual
    |A x_i - theta_i x_i| <= tol b, i < k, b the Gershgorin bound; a warning and EIG_NOT_CONVERGED after max_outer iterations.
    ValueError for k < 1, k above the vertices of the smallest mesh, a non-tensor or host tensor, a vertex with more incident
    faces than SN_LAP_MAX_DEGREE.  Synchronises once per outer iteration (the convergence test)."""
    who = "laplacian_eigenpairs"
    Vg, Fg, B, voff_h = _spectral_layout(who, V, F, sizes)
    n = voff_h[-1]
    smallest = min(voff_h[b + 1] - voff_h[b] for b in range(B))
    k = int(k)
    if k < 1 or k > smallest:
        raise ValueError(f"{who}: k must lie in 1..{smallest} (the vertices of the smallest mesh), got {k}")
    if deg < 1 or max_outer < 1:
        raise ValueError(f"{who}: deg >= 1 and max_outer >= 1 are required, got {deg} and {max_outer}")
    from . import mesh_ops

    dev = Vg.device
    rowptr, colind, S, mass, status = kernels.cot_pencil_from_mesh(Vg, Fg)
    if status & kernels.DESC_DEGREE:
        raise ValueError(f"{who}: a vertex has more incident faces than SN_LAP_MAX_DEGREE (status SN_DESC_DEGREE)")
    parts = [slice(voff_h[b], voff_h[b + 1]) for b in range(B)]
    voff = torch.tensor(voff_h, dtype=torch.int32, device=dev)
    Am = mass.clamp_min(mesh_ops.EIG_MASS_FLOOR)
    clipped = (~(mass >= mesh_ops.EIG_MASS_FLOOR)).any()
    for p in parts:
        Am[p] /= Am[p].sum()
    d = 1 / torch.sqrt(Am)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
    A = (d[rows] * S) * d[colind.long()]
    one = torch.ones(B, dtype=torch.float64, device=dev)
    zero = torch.zeros(B, dtype=torch.float64, device=dev)
    ones = torch.ones(n, 1, dtype=torch.float64, device=dev)
    absrow = kernels.cheb_filter_step(rowptr, colind, A.abs(), voff, one, zero, zero, ones, ones)      # row sums in stored order
    bound = torch.stack([absrow[p].max() for p in parts])
    bound_h, clipped = bound.tolist(), bool(clipped)
    if clipped:
        status |= kernels.EIG_CLIPPED_MASS
    m = min(smallest, k + (mesh_ops.eig_guard(k) if guard is None else int(guard)))
    X = kernels.spectral_start(seed, voff, n, m)
    for p in parts:
        X[p] = torch.linalg.qr(X[p])[0]
    AX, T = torch.empty_like(X), torch.empty_like(X)
    theta = torch.zeros(B, m, dtype=torch.float64, device=dev)
    res = torch.zeros(B, k, dtype=torch.float64, device=dev)
    active, outer = [True] * B, [0] * B
    for it in range(1, max_outer + 1):
        kernels.cheb_filter_step(rowptr, colind, A, voff, one, zero, zero, X, X, out=AX)
        for b, p in enumerate(parts):
            if active[b]:
                H = X[p].T @ AX[p]
                theta[b], Q = _sym_eigh((H + H.T) / 2)
                X[p], AX[p] = X[p] @ Q, AX[p] @ Q
                res[b] = (AX[p] - X[p] * theta[b]).square().sum(dim=0).sqrt()[:k]
        theta_h, res_h = theta.tolist(), res.tolist()
        for b in range(B):
            if active[b]:
                outer[b] = it
                active[b] = not all(r <= tol * bound_h[b] for r in res_h[b])
        if not any(active):
            break
        if it == max_outer:
            status |= kernels.EIG_NOT_CONVERGED
            warnings.warn(f"{who}: a mesh did not reach tol = {tol:g} within max_outer = {max_outer} outer iterations", RuntimeWarning,
                          stacklevel=2)
            break
        # a converged mesh is handed through: Z = 0 (...) + X
        sc = [mesh_ops.cheb_filter_scalars(theta_h[b][0], theta_h[b][m - 1], bound_h[b], deg) if active[b]
              else (np.zeros(deg), np.full(deg, -1.0), np.zeros(deg)) for b in range(B)]
        alpha, beta, shift = (torch.from_numpy(np.stack([s[j] for s in sc], axis=1)).to(dev) for j in range(3))      # (deg, B) each
        old, cur = X, X                       # two buffers: Z takes the place of the older block
        for j in range(deg):
            kernels.cheb_filter_step(rowptr, colind, A, voff, alpha[j], beta[j], shift[j], old, cur, out=T if j == 0 else old)
            old, cur = (cur, T) if j == 0 else (cur, old)
        if cur is not X:
            X, T = T, X
        for b, p in enumerate(parts):
            if active[b]:
                X[p] = torch.linalg.qr(X[p])[0]
    return Eigenpairs(theta[:, :k].contiguous(), (d[:, None] * X[:, :k]).contiguous(), res, bound,
                      torch.tensor(outer, device=dev), Am, voff, status)


def wave_kernel_signature(V, F, N: int = 100, k: int = 300, eigenpairs: Optional[Eigenpairs] = None, dtype=torch.float32,
                          sizes: Optional[Sequence[int]] = None) -> torch.Tensor:
    """(nV, N) wave kernel signature on the device, geom_utils.compute_wks line for line (the 'wks': 100 input channels of the
    reference's normal prediction): E = sorted |values|, logE = log(max(E, 1e-6)), ee = linspace(logE[1], max(logE) / 1.02, N),
    sigma = 6 (ee[1] - ee[0]), W_ki = exp(-(ee_i - logE_k)^2 / (2 sigma^2)), WKS[v, i] = (sum_k phi_vk^2 W_ki) / sum_k W_ki.
    The eigenpairs are laplacian_eigenpairs(V, F, k, sizes=sizes) unless given; W and C (a few kilobytes) are torch
    expressions, the nV x k x N contraction is kernels.wks_contract.  Host statement: mesh_ops.wave_kernel_signature.
    dtype: torch.float32 (default) or torch.float64.  A batch (B, nV, 3) keeps its leading axis: (B, nV, N).  N >= 2, k >= 2."""
    who = "wave_kernel_signature"
    if N < 2 or (eigenpairs is None and k < 2) or (eigenpairs is not None and eigenpairs.values.shape[1] < 2):
        raise ValueError(f"{who}: N >= 2 and k >= 2 are required")
    ep = eigenpairs if eigenpairs is not None else laplacian_eigenpairs(V, F, k, sizes=sizes)
    B, kk = ep.values.shape
    E, order = ep.values.abs().sort(dim=1, stable=True)
    logE = torch.log(E.clamp_min(1e-6))
    start, stop = logE[:, 1], logE.max(dim=1).values / 1.02
    step = (stop - start) / (N - 1)                                                                       # numpy's linspace
    ee = torch.arange(N, dtype=torch.float64, device=E.device)[None, :] * step[:, None] + start[:, None]
    ee[:, -1] = stop
    sigma = (ee[:, 1] - ee[:, 0]) * 6
    W = torch.exp((-(ee[:, None, :] - logE[:, :, None]) ** 2) / (2 * sigma ** 2)[:, None, None])
    C = W.sum(dim=1)
    counts = (ep.voff[1:] - ep.voff[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(B, device=E.device), counts)
    phi = ep.vectors.gather(1, order[seg])
    out = kernels.wks_contract(phi, ep.voff, W, C, dtype)
    return out.view(V.shape[0], V.shape[1], N) if torch.is_tensor(V) and V.dim() == 3 else out


# ---- mesh hierarchy (include/sn_spmm.h "Mesh hierarchy"; the numpy statement is mesh_ops.mesh_hierarchy) ------------------------------
MeshHierarchy = collections.namedtuple("MeshHierarchy", "L real order position sizes singletons rounds status positions")


def _csr_rows(rowptr, n: int):
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device, dtype=torch.int64), torch.diff(rowptr.long()))


def _csr_from_sorted(rows, cols, vals, shape):
    """SparseOperator from COO triples in any order with distinct (row, column) pairs: sorted by row, then column."""
    M, K = shape
    order = torch.argsort(rows * K + cols)
    rowptr = torch.zeros(M + 1, dtype=torch.int64, device=rows.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=M), 0)
    return SparseOperator(rowptr.int(), cols[order].int(), vals[order].contiguous(), (M, K))


def mesh_hierarchy(L: SparseOperator, levels: int = 4, mass=None, pad_coarsest_to: int = 1, max_rounds: int = 1024,
                   blocks=None) -> MeshHierarchy:
    """Hierarchy of a square fp32 CSR operator with ascending columns on the device, level 0 the coarsest as the `Laps` of
    cascade.LapCascade are indexed; equal to mesh_ops.mesh_hierarchy bit for bit (integers as integers, fp32 by bit pattern).

    levels - 1 times: the handshake matching on the Graclus scores and the restriction weights in one launch
    (kernels.mesh_match), clusters numbered by the rank of their smallest member, the coarse operator R (L P) by two spgemm
    products.  Positions: pos_0(c) = c; pos_k(child) = 2 pos_{k-1}(parent) + slot, slot 0 for the child with the smaller number;
    a singleton's slot 1 is a fake node with an empty row and column.  mass: (n,) fp32 restriction weights, None = ones
    (vertex_mass fits).  pad_coarsest_to rounds the coarsest count up with fake clusters.  blocks: the row counts of the meshes of
    a block-diagonal batch (None: one mesh): every mesh gets the coarsest size of the largest and owns positions
    b n_0 2^k .. (b + 1) n_0 2^k of level k.  Per level the host reads the cluster count (it sizes the next level) together with
    the rounds and the status word.  RuntimeError past max_rounds, ValueError for a column outside the operator.

    Returns MeshHierarchy: L[k] SparseOperators in position order, (B n_0 2^k) square; real[k] bool masks; order: position -> id or
    -1; position: id -> position; sizes, singletons, rounds per level (lists of int); status; positions[k]: level-k number ->
    position.  levels = 1 returns L unchanged with the identity order."""
    if not isinstance(L, SparseOperator):
        raise TypeError("mesh_hierarchy wants a SparseOperator")
    kernels._dev(L.rowptr, mass if torch.is_tensor(mass) else None)
    n, K = L._shape
    if n != K or levels < 1 or pad_coarsest_to < 1:
        raise ValueError("mesh_hierarchy: a square operator, levels >= 1 and pad_coarsest_to >= 1 are required")
    blocks = [n] if blocks is None else [int(b) for b in blocks]
    if sum(blocks) != n:
        raise ValueError(f"mesh_hierarchy: blocks sum to {sum(blocks)}, the operator has {n} rows")
    dev = L.rowptr.device
    i64 = dict(dtype=torch.int64, device=dev)
    m = None if mass is None else torch.as_tensor(mass, dtype=torch.float32, device=dev).reshape(n).contiguous()
    ops, mates, parents, rounds, singles = [L], [None], [None], [0], [0]
    owners = [torch.repeat_interleave(torch.arange(len(blocks), **i64), torch.tensor(blocks, **i64))]
    status = 0
    for _ in range(levels - 1):
        cur = ops[0]
        nk = cur._shape[0]
        mate, r, msum, out = kernels.mesh_match(cur.rowptr, cur.colind, cur.vals, nk, m, max_rounds)
        idx = torch.arange(nk, **i64)
        mate = mate.long()
        rep = torch.where((mate >= 0) & (mate < idx), mate, idx)
        is_rep = rep == idx
        parent = (torch.cumsum(is_rep.long(), 0) - 1)[rep]
        nc, nsingle, nrounds, st = (int(v) for v in torch.stack([is_rep.sum(), (mate < 0).sum(), out[0].long(), out[1].long()]).tolist())
        status |= st
        kernels.raise_for_status("mesh_hierarchy", "hierarchy", st, ((constants.HIER_BAD_COLUMN, ValueError),
                                                                     (constants.HIER_NOT_FINISHED, RuntimeError)))
        P = SparseOperator(torch.arange(nk + 1, dtype=torch.int32, device=dev), parent.int(), torch.ones(nk, device=dev), (nk, nc))
        R = _csr_from_sorted(parent, idx, r, (nc, nk))
        Lc = spgemm(R, spgemm(cur, P))
        m = msum[is_rep].contiguous()
        own = owners[0][is_rep]
        mates[0], parents[0], rounds[0], singles[0] = mate, parent, nrounds, nsingle
        ops.insert(0, Lc); mates.insert(0, None); parents.insert(0, None); rounds.insert(0, 0); singles.insert(0, 0)
        owners.insert(0, own)
    if levels == 1:
        eye = torch.arange(n, **i64)
        return MeshHierarchy([L], [torch.ones(n, dtype=torch.bool, device=dev)], eye, eye, [n], [0], [0], 0, [eye])
    B = len(blocks)
    counts0 = torch.bincount(owners[0], minlength=B)
    n0 = -(-max(int(counts0.max()), 1) // pad_coarsest_to) * pad_coarsest_to
    first0 = torch.cumsum(counts0, 0) - counts0
    pos = owners[0] * n0 + (torch.arange(ops[0]._shape[0], **i64) - first0[owners[0]])
    out_L, real, sizes, positions = [], [], [], []
    for k in range(levels):
        if k > 0:
            mate = mates[k]
            pos = 2 * pos[parents[k]] + ((mate >= 0) & (mate < torch.arange(mate.numel(), **i64))).long()
        size = (B * n0) << k
        op = ops[k]
        nk = op._shape[0]
        rows = _csr_rows(op.rowptr, nk)
        out_L.append(_csr_from_sorted(pos[rows], pos[op.colind.long()], op.vals, (size, size)))
        mask = torch.zeros(size, dtype=torch.bool, device=dev)
        mask[pos] = True
        real.append(mask)
        sizes.append(nk)
        positions.append(pos)
    order = torch.full((real[-1].numel(),), -1, **i64)
    order[pos] = torch.arange(n, **i64)
    return MeshHierarchy(out_L, real, order, pos, sizes, singles, rounds, status, positions)
