"""The status bits and limits of the C interface (include/sn_spmm.h), once.  Standard library only: mesh_ops (numpy / scipy, the
host statements) and kernels (torch, the launchers) both take their copies from here and keep exposing them under the same names.

Every upper-case number of this module mirrors the macro SN_<NAME>, except the names of _OTHER_MACRO; MACROS has the pairs and
tests/test_constants.py holds them to the header, both ways.  A status word is shared by the entry points of one family (the
curvature and eigenpair bits sit next to the descriptor bits in one word), and different families reuse the low bits
(ARAP_BAD_FACE == DESC_CLAMPED == 8): what a bit means is asked of status_names / status_sentences with the family.
"""
from __future__ import annotations

# Mass-normalised Laplacians, corner tables
LAP_MAX_DEGREE = 24                  # the device row kernels keep a vertex's neighbours in registers
MESH_CORNER_BYTES = 40               # int32 a, b; float l_a, l_b; double c, s_b, h

# Intrinsic Delaunay Laplacian
IDT_BAD_FACE, IDT_NOT_CONVERGED, IDT_DEGENERATE, IDT_NON_MANIFOLD, IDT_ORIENTATION = 1, 2, 4, 8, 16
IDT_THRESHOLD = -1e-12               # a glued side is non-Delaunay iff cot_f + cot_g < IDT_THRESHOLD (part of the definition)

# Mesh clean-up: the two modes, then the status bits
CC_EDGE, CC_VERTEX = 0, 1
CC_BAD_FACE, CC_INTERNAL = 1, 2

# Mesh repair
REPAIR_BAD_FACE, REPAIR_NONFINITE, REPAIR_NONORIENTABLE, REPAIR_NONMANIFOLD, REPAIR_INTERNAL = 1, 2, 4, 8, 16

# Lattice Delaunay and the Mesh-MNIST maker
DELAUNAY_MAX_POINTS = 1024
MESHDIGITS_MAX_ATTEMPTS = 8
MESHDIGITS_MIN_DET = 85899345        # floor(0.02 * 2^32): area <= 1e-2 pixel^2  <=>  det <= this
DT_DEGENERATE, DT_DUPLICATE, DT_RANGE, DT_TOO_LARGE, DT_NOT_CONVERGED, DT_REJECTED, DT_INTERNAL = 1, 2, 4, 8, 16, 32, 64

# Mesh descriptors; the curvature and eigenpair bits share their word
DESC_BAD_FACE, DESC_FLAT_FACE, DESC_NO_NORMAL, DESC_CLAMPED, DESC_DEGREE = 1, 2, 4, 8, 16
DESC_MASS_BARYCENTRIC, DESC_MASS_VORONOI = 0, 1
CURV_FEW_POINTS, CURV_NO_NORMAL, CURV_OVERFLOW, CURV_DEGENERATE = 32, 64, 128, 1024
CURV_MAX_RING = 1024                 # the largest patch
CURV_MIN_POINTS = 6                  # the smallest patch a quadric is fitted to
CURV_PIVOT_FLOOR = 1e-12             # a Cholesky pivot must exceed this times its diagonal entry of G
EIG_NOT_CONVERGED, EIG_CLIPPED_MASS = 256, 512

# ARAP deformation
ARAP_NOT_CONVERGED, ARAP_BREAKDOWN, ARAP_DEGENERATE, ARAP_BAD_FACE, ARAP_DEGREE, ARAP_TOO_LARGE = 1, 2, 4, 8, 16, 32
ARAP_REDUCE_WIDTH = 1024             # SN_ARAP_THREADS: the width of the workgroup's reduction tree
ARAP_JACOBI_SWEEPS = 6
ARAP_RANK_EPS = 1e-20
ARAP_MAX_CG = 65536

# Mesh hierarchy
HIER_NOT_FINISHED, HIER_BAD_COLUMN = 1, 2
HIER_THREADS = 1024                  # the one workgroup that walks an operator

# Graph attention
ATTN_MAX_CHANNELS = 256              # C / 4 lanes of one wave hold a row
ATTN_SLOPE = 0.2                     # the negative slope of the logits' leaky ReLU (part of the definition)

# Sparse x sparse products
SPGEMM_MAX_WINDOW = 131072
SPGEMM_BAD_COLUMN, SPGEMM_TOO_WIDE, SPGEMM_TOO_LARGE, CSR_NO_OFFDIAGONAL = 1, 2, 4, 8

_OTHER_MACRO = {"ARAP_REDUCE_WIDTH": "SN_ARAP_THREADS"}
MACROS = {name: _OTHER_MACRO.get(name, "SN_" + name) for name, value in list(globals().items())
          if name.isupper() and not name.startswith("_") and isinstance(value, (int, float))}
__all__ = list(MACROS)               # what `from .constants import *` hands to mesh_ops and kernels: the mirrored numbers

BAD_FACE_SENTENCE = "a face has an index outside the mesh or a repeated index"

# What every status bit says, by constant name; the short name of a bit is its constant without the family prefix
_SENTENCES = {
    "SPGEMM_BAD_COLUMN": "a column index is outside the operand's column range",
    "SPGEMM_TOO_WIDE": f"a result row spans more than spgemm_max_window() = {SPGEMM_MAX_WINDOW} columns; there is no other path",
    "SPGEMM_TOO_LARGE": "the result's structural entries do not fit int32 row pointers",
    "CSR_NO_OFFDIAGONAL": "a row holds fewer than two entries (no off-diagonal entry: D^-1/2 divides by zero)",
    "IDT_BAD_FACE": BAD_FACE_SENTENCE,
    "IDT_NOT_CONVERGED": "the last of the max_rounds flip rounds still found a non-Delaunay side",
    "IDT_DEGENERATE": "a tested face has a Heron radicand <= 0: its sides are never flipped",
    "IDT_NON_MANIFOLD": "an edge has more than two faces (the mesh is not manifold)",
    "IDT_ORIENTATION": "an edge is traversed in the same direction by its two faces (the mesh is not consistently oriented)",
    "CC_BAD_FACE": BAD_FACE_SENTENCE,
    "CC_INTERNAL": "the component kernels hit a loop bound (status SN_CC_INTERNAL)",
    "REPAIR_BAD_FACE": BAD_FACE_SENTENCE,
    "REPAIR_NONFINITE": "a vertex has a coordinate that is not finite",
    "REPAIR_NONORIENTABLE": "an orientation class has no consistent winding and was left as it came",
    "REPAIR_NONMANIFOLD": "an edge has three or more faces and links none of them",
    "REPAIR_INTERNAL": "the repair kernels hit a loop bound (status SN_REPAIR_INTERNAL)",
    "DT_DEGENERATE": "fewer than three points, or all of them on one line",
    "DT_DUPLICATE": "two points coincide",
    "DT_RANGE": "a coordinate lies outside the lattice",
    "DT_TOO_LARGE": f"more than {DELAUNAY_MAX_POINTS} points",
    "DT_NOT_CONVERGED": "the flip rounds ran out before the triangulation was Delaunay",
    "DT_REJECTED": f"every one of the sampling attempts was refused (at most {MESHDIGITS_MAX_ATTEMPTS})",
    "DT_INTERNAL": "the triangulation kernels hit a loop bound",
    "DESC_BAD_FACE": BAD_FACE_SENTENCE,
    "DESC_FLAT_FACE": "a face is flat and contributes nothing",
    "DESC_NO_NORMAL": "a vertex has no normal",
    "DESC_CLAMPED": "an entry that was not finite or exceeded 1e10 in magnitude was replaced",
    "DESC_DEGREE": "a vertex has more incident faces than SN_LAP_MAX_DEGREE (status SN_DESC_DEGREE)",
    "CURV_FEW_POINTS": "a patch has fewer than six members",
    "CURV_NO_NORMAL": "a vertex has no normal",
    "CURV_OVERFLOW": f"a patch has more than {CURV_MAX_RING} members",
    "CURV_DEGENERATE": "a patch is degenerate",
    "EIG_NOT_CONVERGED": "an eigenpair did not reach tol",
    "EIG_CLIPPED_MASS": "a Voronoi mass below the floor was clipped",
    "ARAP_NOT_CONVERGED": "a conjugate-gradient solve stopped at max_cg iterations before reaching tol",
    "ARAP_BREAKDOWN": "a solve broke down (p.Ap <= 0 or a free row without a positive diagonal): the frame keeps its start values",
    "ARAP_DEGENERATE": "a vertex has spokes of rank below 2: its rotation is the identity",
    "ARAP_BAD_FACE": BAD_FACE_SENTENCE,
    "ARAP_DEGREE": "a vertex has more incident faces than SN_LAP_MAX_DEGREE and got no weights",
    "ARAP_TOO_LARGE": "a mesh was too large for the launch and was left at rest",
    "HIER_NOT_FINISHED": "the matching is not finished after max_rounds rounds",
    "HIER_BAD_COLUMN": "a column index is outside the operator",
}


def _family(*prefixes):
    rows = [(globals()[name], name.split("_", 1)[1], text) for name, text in _SENTENCES.items()
            if name.startswith(prefixes)]
    return tuple(sorted(rows))


# family -> ((bit, short name, sentence), ...) in ascending bit order: one table per status word ("curvature" is the part of the
# descriptor word that sn_mesh_principal_curvature_f32 raises)
STATUS_FAMILIES = {
    "spgemm": _family("SPGEMM_", "CSR_"),
    "idt": _family("IDT_"),
    "components": _family("CC_"),
    "repair": _family("REPAIR_"),
    "delaunay": _family("DT_"),
    "descriptors": _family("DESC_", "CURV_", "EIG_"),
    "curvature": _family("DESC_BAD_FACE", "CURV_"),
    "arap": _family("ARAP_"),
    "hierarchy": _family("HIER_NOT_FINISHED", "HIER_BAD_COLUMN"),
}


def status_sentences(family: str, status: int) -> list:
    """What the bits set in `status` say, one sentence per bit of the family, ascending."""
    return [text for bit, _, text in STATUS_FAMILIES[family] if status & bit]


def status_names(family: str, status: int) -> list:
    """The short names of the bits set in `status`, ascending."""
    return [name for bit, name, _ in STATUS_FAMILIES[family] if status & bit]
