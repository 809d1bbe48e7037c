"""The byte counts of the *_workspace_bytes queries of the mesh builders, the sparse product, the scan and the transpose (no GPU:
they are host functions of the library).  Callers allocate by these numbers and the refusal tests pass one byte less, so a layout
that is described differently must still add up to the same total: the table below was recorded from the library as it was
before the layouts moved onto one carver (commit 55d8aba), and is compared literally."""
import pytest

from surfacenetworks_amd import _lib

NV = (0, 1, 2047, 2048, 4096, 6890)          # 2047 / 2048: nV + 1 at and past one scan tile of 2048 items; 6890: FAUST
NF = (0, 1, 13776)

# (nV, nF) -> bytes, rows over NV, columns over NF
BY_VERTICES_AND_FACES = {
    "sn_dirac_workspace_bytes": ((48, 80, 275568), (64, 96, 275584), (32784, 32816, 308304), (32816, 32848, 308336), (65584, 65616, 341104), (110288, 110320, 385808)),
    "sn_laplacian_workspace_bytes": ((48, 80, 275568), (64, 96, 275584), (32784, 32816, 308304), (32816, 32848, 308336), (65584, 65616, 341104), (110288, 110320, 385808)),
    "sn_mesh_glue_workspace_bytes": ((48, 64, 165360), (48, 64, 165360), (16400, 16416, 181712), (16432, 16448, 181744), (32816, 32832, 198128), (55168, 55184, 220480)),
    "sn_mesh_idt_laplacian_workspace_bytes": ((32, 272, 3306592), (80, 320, 3306640), (57360, 57600, 3363920), (57376, 57616, 3363936), (114720, 114960, 3421280), (192960, 193200, 3499520)),
    "sn_mesh_compact_workspace_bytes": ((48, 48, 55168), (48, 48, 55168), (8224, 8224, 63344), (8240, 8240, 63360), (16432, 16432, 71552), (27616, 27616, 82720)),
    "sn_mesh_orient_workspace_bytes": ((48, 80, 220464), (48, 80, 220464), (16400, 16432, 236816), (16432, 16464, 236848), (32816, 32848, 253232), (55168, 55200, 275584)),
    "sn_mesh_descriptors_workspace_bytes": ((48, 64, 165360), (48, 64, 165360), (16400, 16416, 181712), (16432, 16448, 181744), (32816, 32832, 198128), (55168, 55184, 220480)),
    "sn_mesh_cot_laplacian_workspace_bytes": ((48, 64, 165360), (48, 64, 165360), (16400, 16416, 181712), (16432, 16448, 181744), (32816, 32832, 198128), (55168, 55184, 220480)),
}
# sn_mesh_components_workspace_bytes(nV, nF, mode) by mode (SN_CC_EDGE = 0, SN_CC_VERTEX = 1)
COMPONENTS = {
    0: ((64, 80, 165376), (64, 80, 165376), (16416, 16432, 181728), (16448, 16464, 181760), (32832, 32848, 198144), (55184, 55200, 220496)),
    1: ((16, 16, 16), (16, 16, 16), (16, 16, 16), (16, 16, 16), (16, 16, 16), (16, 16, 16)),
}
# sn_csr_transpose_workspace_bytes(M = nF, K = nV, nnz = 3 nF)
TRANSPOSE = ((8, 8, 8), (24, 24, 24), (8200, 8200, 8200), (8204, 8204, 8204), (16400, 16400, 16400), (27588, 27588, 27588))
# one argument, over NV
BY_VERTICES = {
    "sn_mesh_corners_workspace_bytes": (32, 32, 8208, 8224, 16416, 27600),
    "sn_mesh_weld_workspace_bytes": (16, 16, 16384, 16384, 32768, 65536),
    "sn_csr_spgemm_workspace_bytes": (32, 32, 8208, 8224, 16416, 27600),
    "sn_scan_workspace_bytes": (4, 8, 8, 8, 12, 20),
}
# one argument, over NF
BY_FACES = {
    "sn_mesh_idt_workspace_bytes": (0, 16, 110208),
    "sn_mesh_unique_faces_workspace_bytes": (16, 16, 131072),
}


def _table(fn):
    return tuple(tuple(int(fn(v, f)) for f in NF) for v in NV)


@pytest.mark.parametrize("name", sorted(BY_VERTICES_AND_FACES))
def test_two_argument_queries(name):
    assert _table(getattr(_lib.load(), name)) == BY_VERTICES_AND_FACES[name]


@pytest.mark.parametrize("mode", sorted(COMPONENTS))
def test_components_query(mode):
    lib = _lib.load()
    assert _table(lambda v, f: lib.sn_mesh_components_workspace_bytes(v, f, mode)) == COMPONENTS[mode]


def test_transpose_query():
    lib = _lib.load()
    assert _table(lambda v, f: lib.sn_csr_transpose_workspace_bytes(f, v, 3 * f)) == TRANSPOSE


@pytest.mark.parametrize("name", sorted(BY_VERTICES) + sorted(BY_FACES))
def test_one_argument_queries(name):
    fn = getattr(_lib.load(), name)
    if name in BY_VERTICES:
        assert tuple(int(fn(v)) for v in NV) == BY_VERTICES[name]
    else:
        assert tuple(int(fn(f)) for f in NF) == BY_FACES[name]


def test_every_mesh_builder_query_is_in_the_table():
    """A *_workspace_bytes of sn_meshops.hip that is added later has to be added here too."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "surfacenetworks_amd", "csrc", "sn_meshops.hip")).read()
    declared = set(re.findall(r"^size_t (sn_\w+_workspace_bytes)\(", src, re.M))
    covered = set(BY_VERTICES_AND_FACES) | set(BY_VERTICES) | set(BY_FACES) | {"sn_mesh_components_workspace_bytes"}
    assert declared and declared <= covered, sorted(declared - covered)
