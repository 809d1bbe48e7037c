"""Mesh clean-up on the device against its host statement (mesh_ops.components / compact / largest_component), bit for bit:
kernels.mesh_components, mesh_label_mask, mesh_compact, operators.clean_mesh and faust_frame_from_mesh(component="largest").
Every comparison is an exact integer or bitwise one; no tolerance anywhere."""
import numpy as np
import pytest
import torch

import abi_cases
import components_cases as cases
from surfacenetworks_amd import datasets, kernels, mesh_ops, operators

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")              # (a copy: the cases are read-only)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _device_components(name, mode):
    c = cases.case(name)
    return kernels.mesh_components(_dev(c.F), c.V.shape[0], mode)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_components_equal_the_host_twin(name, mode):
    want = cases.host_components(name, mode)
    got = _device_components(name, mode)
    assert (got.vlabel is None) == (want.vlabel is None) == (mode == "edge")
    if mode == "vertex":
        assert got.vlabel.dtype == torch.int32 and np.array_equal(_np(got.vlabel), want.vlabel)
    for field in ("flabel", "count", "summary"):
        g = getattr(got, field)
        assert g.dtype == torch.int32 and np.array_equal(_np(g), getattr(want, field)), field
    assert _np(got.status).tolist() == [want.status]


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_compact_equals_the_host_twin(name, mode):
    c = cases.case(name)
    nV = c.V.shape[0]
    keep = cases.winner_mask(name, mode)
    want = mesh_ops.compact(c.V, c.F, keep)
    got = kernels.mesh_compact(_dev(c.F), _dev(keep), nV, _dev(c.V))
    nVk, nFk = _np(got.sizes).tolist()
    assert [nVk, nFk] == want.sizes.tolist()
    assert np.array_equal(_np(got.I), want.I)
    assert np.array_equal(_np(got.J)[:nVk], want.J) and np.array_equal(_np(got.Fsrc)[:nFk], want.Fsrc)
    assert np.array_equal(_np(got.Fnew)[:nFk], want.Fnew)
    assert _np(got.Vnew)[:nVk].tobytes() == want.Vnew.tobytes()
    nov = kernels.mesh_compact(_dev(c.F), _dev(keep), nV)              # without coordinates: the same maps, no Vnew
    assert nov.Vnew is None and torch.equal(nov.I, got.I) and torch.equal(nov.sizes, got.sizes)
    assert torch.equal(nov.J[:nVk], got.J[:nVk]) and torch.equal(nov.Fnew[:nFk], got.Fnew[:nFk])


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", ["two_grids", "tie", "junk", "all_bad"])
def test_label_mask_is_the_winner_on_the_device(name, mode):
    cc = _device_components(name, mode)
    keep = kernels.mesh_label_mask(cc.flabel, cc.summary[1:2])
    assert keep.dtype == torch.int32 and np.array_equal(_np(keep), cases.winner_mask(name, mode))


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", ["strip_permuted", "soup"])
def test_two_runs_are_bit_identical(name, mode):
    a, b = _device_components(name, mode), _device_components(name, mode)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


def test_clean_mesh_on_junk_returns_the_large_grid():
    c = cases.case("junk")
    Vw, Fw, Jw, Fsrcw = cases.expected_part("junk", 0)
    assert len(Jw) == 144 and len(Fsrcw) == 242                        # the grid_cloth(12, 12)
    for V, F in ((_dev(c.V), _dev(c.F)), (c.V, c.F.astype(np.int64))):           # device tensors, and numpy
        cm = operators.clean_mesh(V, F)
        assert cm.V.dtype == torch.float32 and _np(cm.V).tobytes() == Vw.tobytes()
        assert cm.F.dtype == torch.int32 and np.array_equal(_np(cm.F), Fw)
        assert np.array_equal(_np(cm.vertex_map), Jw) and np.array_equal(_np(cm.face_map), Fsrcw)
        index = np.full(c.V.shape[0], -1, np.int32)
        index[Jw] = np.arange(len(Jw))
        assert np.array_equal(_np(cm.vertex_index), index)
        assert (cm.components, cm.bad_faces) == (3, 4)
        assert (cm.faces_dropped, cm.vertices_dropped) == (c.F.shape[0] - 242, c.V.shape[0] - 144)
    # "all": only the bad faces and the unused vertices go;  an integer label: that component (the stray triangle's face id)
    every = operators.clean_mesh(_dev(c.V), _dev(c.F), component="all")
    assert (every.components, every.bad_faces, every.faces_dropped, every.vertices_dropped) == (3, 4, 4, int((c.vert_block < 0).sum()))
    assert np.array_equal(_np(every.face_map), np.nonzero(c.face_block >= 0)[0])
    stray = int(np.nonzero(c.face_block == 2)[0][0])
    one = operators.clean_mesh(_dev(c.V), _dev(c.F), component=stray)
    assert np.array_equal(_np(one.face_map), [stray]) and np.array_equal(_np(one.F), [[0, 1, 2]]) and one.V.shape == (3, 3)
    with pytest.raises(ValueError, match="names no component"):
        operators.clean_mesh(_dev(c.V), _dev(c.F), component=stray + 1)             # a face id that is no class minimum
    with pytest.raises(ValueError, match="names no component"):
        operators.clean_mesh(_dev(c.V), _dev(c.F), component=c.F.shape[0])
    vert = operators.clean_mesh(_dev(c.V), _dev(c.F), connectivity="vertex")
    assert torch.equal(vert.V, cm.V) and torch.equal(vert.F, cm.F)


def test_frame_from_a_disconnected_mesh_end_to_end():
    c = cases.case("two_grids")
    V, F = _dev(c.V), _dev(c.F)
    with pytest.raises(ValueError, match="disconnected"):               # the gap: what every builder said before the clean-up
        operators.geodesic_matrix_from_mesh(V, F)
    frame = datasets.faust_frame_from_mesh(V, F, component="largest")
    Vw, Fw, Jw, _ = cases.expected_part("two_grids", 0)
    assert frame["V"].shape == (144, 3) and bool(torch.isfinite(frame["G"]).all())
    own = operators.geodesic_matrix_from_mesh(_dev(Vw), _dev(Fw))       # the 12 x 12 part on its own, same relative order
    assert torch.equal(frame["G"], own)
    assert frame["vertex_map"].dtype == torch.int64 and np.array_equal(_np(frame["vertex_map"]), Jw)
    assert np.array_equal(_np(frame["label"]), np.arange(144)) and _np(frame["V"]).tobytes() == Vw.tobytes()


def test_component_none_leaves_the_frame_as_it_was():
    V, F = mesh_ops.grid_cloth(9, 7, np.random.default_rng(21))
    label = np.random.default_rng(22).permutation(V.shape[0])
    a = datasets.faust_frame_from_mesh(V, F, label=label)
    b = datasets.faust_frame_from_mesh(V, F, label=label, component=None)
    assert list(a) == list(b) and "vertex_map" not in b
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k].shape == b[k].shape and all(np.array_equal(getattr(a[k], x), getattr(b[k], x)) for x in ("indptr", "indices", "data")), k


def test_refusals():
    for name in cases.NO_FACE:
        c = cases.case(name)
        with pytest.raises(ValueError, match="no face"):
            operators.clean_mesh(_dev(c.V), _dev(c.F))
    c = cases.case("two_grids")
    V, F = _dev(c.V), _dev(c.F)
    with pytest.raises(ValueError, match="label must be None"):
        datasets.faust_frame_from_mesh(V, F, label=np.arange(c.V.shape[0]), component="largest")
    with pytest.raises(ValueError, match="component"):
        datasets.faust_frame_from_mesh(V, F, component="all")
    keep = torch.ones(F.shape[0], dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        kernels.mesh_components(F.long(), c.V.shape[0])
    with pytest.raises(TypeError):
        kernels.mesh_compact(F.long(), keep, c.V.shape[0])
    with pytest.raises(TypeError):
        kernels.mesh_compact(F, keep.long(), c.V.shape[0])
    with pytest.raises(TypeError):
        kernels.mesh_compact(F, keep, c.V.shape[0], V.double())
    with pytest.raises(TypeError):
        kernels.mesh_label_mask(keep.long(), keep[:1])
    with pytest.raises(TypeError):
        operators.clean_mesh(V, F.float())
    with pytest.raises(ValueError, match="mode"):
        kernels.mesh_components(F, c.V.shape[0], "corner")
    with pytest.raises(ValueError, match="connectivity"):
        operators.clean_mesh(V, F, connectivity="corner")


def test_c_level_refusals():
    """The statuses of the two entry points for arguments that must be refused before anything is launched (the
    tests/abi_cases.py pattern, device backend)."""
    be = abi_cases.Backend("device")
    lib = be.lib
    nV, nF = 40, 30
    Fp, _ = be.buf(np.zeros((nF, 3), np.int32))
    outp, _ = be.buf(np.zeros(4 * max(nV, nF), np.int32))
    fl, _ = be.buf(np.zeros(3 * max(nV, nF), np.float32))
    wsp, _ = be.buf(np.zeros(1 << 16, np.uint8))
    comp, cpt = lib.sn_mesh_components_i32, lib.sn_mesh_compact_i32
    calls = []
    for mode in (0, 1):
        need = int(lib.sn_mesh_components_workspace_bytes(nV, nF, mode))
        assert 16 <= need <= 1 << 16
        calls += [
            (f"components({mode}): short workspace", comp(Fp, nV, nF, mode, outp, outp, outp, outp, outp, wsp, need - 1, None), abi_cases.SN_E_WORKSPACE),
            (f"components({mode}): null workspace", comp(Fp, nV, nF, mode, outp, outp, outp, outp, outp, None, need, None), abi_cases.SN_E_WORKSPACE),
            (f"components({mode}): null summary", comp(Fp, nV, nF, mode, outp, outp, outp, None, outp, wsp, need, None), abi_cases.SN_E_NULL),
            (f"components({mode}): null F", comp(None, nV, nF, mode, outp, outp, outp, outp, outp, wsp, need, None), abi_cases.SN_E_NULL),
            (f"components({mode}): negative nF", comp(Fp, nV, -1, mode, outp, outp, outp, outp, outp, wsp, need, None), abi_cases.SN_E_SHAPE),
            (f"components({mode}): 3 nF past int32", comp(Fp, nV, 2**30, mode, outp, outp, outp, outp, outp, wsp, need, None), abi_cases.SN_E_RANGE),
        ]
    calls.append(("components: mode 2", comp(Fp, nV, nF, 2, outp, outp, outp, outp, outp, wsp, 1 << 16, None), abi_cases.SN_E_SHAPE))
    calls.append(("components: vertex mode without vlabel", comp(Fp, nV, nF, 1, None, outp, outp, outp, outp, wsp, 1 << 16, None), abi_cases.SN_E_NULL))
    need = int(lib.sn_mesh_compact_workspace_bytes(nV, nF))
    assert 16 <= need <= 1 << 16
    calls += [
        ("compact: short workspace", cpt(fl, Fp, outp, nV, nF, outp, outp, outp, outp, fl, outp, wsp, need - 1, None), abi_cases.SN_E_WORKSPACE),
        ("compact: null keep", cpt(fl, Fp, None, nV, nF, outp, outp, outp, outp, fl, outp, wsp, need, None), abi_cases.SN_E_NULL),
        ("compact: V without Vnew", cpt(fl, Fp, outp, nV, nF, outp, outp, outp, outp, None, outp, wsp, need, None), abi_cases.SN_E_NULL),
        ("compact: null sizes", cpt(fl, Fp, outp, nV, nF, outp, outp, outp, outp, fl, None, wsp, need, None), abi_cases.SN_E_NULL),
        ("compact: nV + 1 past int32", cpt(fl, Fp, outp, 2**31 - 1, nF, outp, outp, outp, outp, fl, outp, wsp, need, None), abi_cases.SN_E_RANGE),
        ("mask: null label", lib.sn_mesh_label_mask_i32(outp, nF, None, outp, None), abi_cases.SN_E_NULL),
    ]
    wrong = [(what, got, want) for what, got, want in calls if got != want]
    assert not wrong, wrong
