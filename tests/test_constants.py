"""The one home of the interface constants (surfacenetworks_amd/constants.py), host side (no GPU): every status bit and limit of
include/sn_spmm.h is mirrored exactly once and mesh_ops / kernels expose that same value; the reason tables cover every bit of
their family; the batch-to-disjoint-mesh layout of operators._offset_batch, guarded and unguarded."""
import os
import re

import pytest
import torch

from surfacenetworks_amd import constants, kernels, mesh_ops, operators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_macros():
    """name -> value of every `#define SN_<NAME> <number>` of the header past the error codes."""
    text = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    text = text[text.index("#define SN_E_UNSUPPORTED"):].split("\n", 1)[1]
    found = re.findall(r"^#define (SN_[A-Z0-9_]+)[ \t]+\(?(-?[0-9][0-9A-Za-z.+-]*)\)?[ \t]*(?:/\*.*)?$", text, flags=re.M)
    out = {}
    for name, value in found:
        assert name not in out, f"{name} is defined twice"
        out[name] = float(value) if re.search(r"[.eE]", value) else int(value, 0)
    return out


def test_every_macro_of_the_header_is_mirrored_exactly_once():
    macros = _header_macros()
    assert len(macros) >= 58 and macros["SN_ARAP_BAD_FACE"] == 8 and macros["SN_IDT_THRESHOLD"] == -1e-12      # the parser works
    assert len(re.findall(r"^#define SN_[A-Z0-9_]+[ \t]+\(?-?[0-9]", open(os.path.join(ROOT, "include", "sn_spmm.h")).read(),
                          flags=re.M)) == len(macros) + 9      # + SN_ABI_VERSION, SN_OK and the seven error codes: none was missed
    mirrored = {}
    for name, macro in constants.MACROS.items():
        assert macro in macros, f"constants.{name} claims to mirror {macro}, which the header does not define"
        assert macro not in mirrored, f"{macro} is mirrored by {mirrored[macro]} and by {name}"
        mirrored[macro] = name
        value = getattr(constants, name)
        assert value == macros[macro] and type(value) is type(macros[macro]), (name, value, macros[macro])
    assert sorted(set(macros) - set(mirrored)) == []      # a status bit or limit without a Python home
    assert constants.MACROS["ARAP_REDUCE_WIDTH"] == "SN_ARAP_THREADS"


def test_mesh_ops_and_kernels_expose_the_same_values():
    seen = 0
    for name in constants.MACROS:
        for module in (mesh_ops, kernels):
            if hasattr(module, name):
                seen += 1
                assert getattr(module, name) == getattr(constants, name), (module.__name__, name)
    assert seen >= 80
    for name in mesh_ops.__all__:      # every constant mesh_ops exports that the header defines comes from the one home
        if name.isupper() and "SN_" + name in _header_macros():
            assert name in constants.MACROS and getattr(mesh_ops, name) == getattr(constants, name), name


@pytest.mark.parametrize("family", sorted(constants.STATUS_FAMILIES))
def test_reason_tables_cover_every_bit_of_their_family(family):
    rows = constants.STATUS_FAMILIES[family]
    bits = [bit for bit, _, _ in rows]
    assert all(bit > 0 and bit & (bit - 1) == 0 for bit in bits) and len(set(bits)) == len(bits)      # one row per bit
    assert all(name and text for _, name, text in rows)
    word = 0
    for bit in bits:
        word |= bit
    assert len(constants.status_sentences(family, word)) == len(rows) == len(constants.status_names(family, word))
    assert constants.status_sentences(family, 0) == [] and constants.status_names(family, 0) == []
    for bit, name, text in rows:
        assert constants.status_sentences(family, bit) == [text] and constants.status_names(family, bit) == [name]


def test_every_status_bit_belongs_to_a_family():
    prefixes = ("SPGEMM_", "CSR_", "IDT_", "CC_", "REPAIR_", "DT_", "DESC_", "CURV_", "EIG_", "ARAP_")
    not_bits = {"SPGEMM_MAX_WINDOW", "IDT_THRESHOLD", "CC_EDGE", "CC_VERTEX", "DESC_MASS_BARYCENTRIC", "DESC_MASS_VORONOI",
                "CURV_MAX_RING", "CURV_MIN_POINTS", "CURV_PIVOT_FLOOR", "ARAP_REDUCE_WIDTH", "ARAP_JACOBI_SWEEPS", "ARAP_RANK_EPS",
                "ARAP_MAX_CG"}
    bits = {n for n in constants.MACROS if n.startswith(prefixes) and n not in not_bits}
    told = {(bit, name) for rows in constants.STATUS_FAMILIES.values() for bit, name, _ in rows}
    for n in bits:
        assert (getattr(constants, n), n.split("_", 1)[1]) in told, n


def test_curvature_status_names_are_what_they_were():
    assert mesh_ops.curvature_status_names(0) == "no status bit"
    assert mesh_ops.curvature_status_names(33) == "BAD_FACE | FEW_POINTS"
    assert mesh_ops.curvature_status_names(1024) == "DEGENERATE"


def test_batch_layout_guarded_and_unguarded():
    B, nV = 2, 3
    V = torch.arange(B * nV * 3, dtype=torch.float32).view(B, nV, 3)
    F = torch.tensor([[0, 2, 3], [-1, 0, 2], [2, 0, 0]], dtype=torch.int32)
    Fb = F.unsqueeze(0).expand(B, -1, -1).contiguous()
    off = (torch.arange(B, dtype=torch.int32) * nV).view(B, 1, 1)
    inside = (Fb >= 0) & (Fb < nV)

    Vg, Fg, b, nv, nf = operators._offset_batch("test", V, Fb)                     # the default is the guarded layout
    assert (b, nv, nf) == (B, nV, 3) and Fg.dtype == torch.int32 and Fg.shape == (B * 3, 3)
    assert torch.equal(Vg, V.reshape(B * nV, 3))
    assert torch.equal(Fg.view(B, 3, 3), torch.where(inside, Fb + off, torch.full_like(Fb, -1)))
    for m in range(B):      # 3 (= nV) and -1 leave the batch in both meshes, 0 and 2 land in their own block
        assert Fg.view(B, 3, 3)[m].tolist() == [[m * nV, m * nV + 2, -1], [-1, m * nV, m * nV + 2], [m * nV + 2, m * nV, m * nV]]

    Vu, Fu, b, nv, nf = operators._offset_batch("test", V, Fb, guard=False)
    assert (b, nv, nf) == (B, nV, 3) and torch.equal(Vu, Vg) and Fu.dtype == torch.int32
    assert torch.equal(Fu.view(B, 3, 3), Fb + off)                                  # exactly F + b nV, bad indices included

    for guard in (True, False):
        shared = operators._offset_batch("test", V, F, guard=guard)                # a shared (nF, 3) F is every mesh's F
        per_mesh = operators._offset_batch("test", V, Fb, guard=guard)
        assert torch.equal(shared[1], per_mesh[1]) and shared[2:] == per_mesh[2:]
        V1, F1, b, nv, nf = operators._offset_batch("test", V[0], F, guard=guard)  # a single mesh passes through untouched
        assert (b, nv, nf) == (1, nV, 3) and torch.equal(V1, V[0]) and torch.equal(F1, F)
    with pytest.raises(ValueError, match="wants V"):
        operators._offset_batch("test", V, Fb[:1])
