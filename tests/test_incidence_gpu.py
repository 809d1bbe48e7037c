"""The by-vertex incidence the mesh builders share (sn_internal_incidence) raises the bad-face bit of its CALLER in the caller's own
status word: SN_ARAP_BAD_FACE for sn_arap_weights_f64, SN_DESC_BAD_FACE for sn_mesh_principal_curvature_f32.  On the smallest mesh
where that can go wrong, a jittered octahedron with three bad faces appended: the two status words exactly, every output of the
two entry points byte for byte against the host statements, no bit leaking from one caller to the other, and the empty shapes."""
import numpy as np
import pytest
import torch

from surfacenetworks_amd import kernels, mesh_ops

pytestmark = pytest.mark.gpu

_AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
V = (_AXES + 0.05 * np.random.default_rng(0).standard_normal((6, 3))).astype(np.float32)
GOOD = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
BAD = np.concatenate([GOOD, np.array([[0, 0, 1], [0, 1, 6], [-1, 2, 3]], dtype=np.int32)])      # repeated, past nV, negative


@pytest.fixture(scope="module")
def host():
    """The host statements, computed once: (ARAP weights, curvatures at radius 2) without and with the bad faces."""
    out = {name: (mesh_ops.arap_weights(V, F), mesh_ops.principal_curvatures(V, F, radius=2)) for name, F in (("good", GOOD), ("bad", BAD))}
    assert out["good"][0].status == 0 and out["good"][1].status == 0
    w, pc = out["bad"]
    assert w.status == kernels.ARAP_BAD_FACE == 8 and int(w.rowptr[-1]) == 24
    assert pc.status == kernels.DESC_BAD_FACE == 1 and not np.isnan(pc.k1).any() and (pc.ring_size == 6).all()
    assert mesh_ops.principal_curvatures(V, BAD, radius=1).status == (kernels.DESC_BAD_FACE | kernels.CURV_FEW_POINTS) == 33
    return out


def _dev(F):
    return torch.tensor(V).cuda(), torch.tensor(F).cuda()


def _same_bytes(got, want):
    got = got.cpu().numpy()
    want = np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _check_weights(got, want, status):
    assert int(got.status.item()) == status == want.status
    nnz = int(want.rowptr[-1])
    assert nnz == 24 and _same_bytes(got.rowptr, want.rowptr) and _same_bytes(got.d, want.d)
    assert _same_bytes(got.colind[:nnz], want.colind[:nnz]) and _same_bytes(got.w[:nnz], want.w[:nnz])


def _check_curvature(got, want, status):
    assert int(got["status"].item()) == status == want.status
    for name in ("k1", "k2", "d1", "d2", "ring_size"):
        assert _same_bytes(got[name], getattr(want, name)), name


def test_each_caller_raises_its_own_bit_in_its_own_word(host):
    Vd, Fd = _dev(BAD)
    _check_weights(kernels.arap_weights(Vd, Fd), host["bad"][0], 8)
    _check_curvature(kernels.mesh_principal_curvature(Vd, Fd, radius=2), host["bad"][1], 1)
    assert int(kernels.mesh_principal_curvature(Vd, Fd, radius=1)["status"].item()) == 33


def test_good_faces_raise_nothing(host):
    Vd, Fd = _dev(GOOD)
    _check_weights(kernels.arap_weights(Vd, Fd), host["good"][0], 0)
    _check_curvature(kernels.mesh_principal_curvature(Vd, Fd, radius=2), host["good"][1], 0)


def test_no_bit_leaks_between_the_two_callers_on_one_stream():
    Vd, Fd = _dev(BAD)
    words = []
    for arap_first in (True, False):
        a = kernels.arap_weights(Vd, Fd).status if arap_first else None
        c = kernels.mesh_principal_curvature(Vd, Fd, radius=2)["status"]
        a = a if arap_first else kernels.arap_weights(Vd, Fd).status
        words.append((int(a.item()), int(c.item())))
    assert words == [(8, 1), (8, 1)]      # a leaked bit would show as 8 in the curvature word or 1 in the ARAP word


@pytest.mark.parametrize("nV,nF", [(6, 0), (0, 0)], ids=["no_faces", "no_vertices"])
def test_empty_shapes_return_without_a_bad_face(nV, nF):
    """The fill and launch guards of the incidence are on these paths.  Both ARAP words are 0 and the curvature word of nV = 0 is
    0; six vertices without a face have no normal by the definition, so their curvature word is the host statement's
    CURV_NO_NORMAL (64, on every commit) — no bad-face bit of either caller in it."""
    Vd = torch.tensor(V[:nV]).cuda()
    Fd = torch.zeros(nF, 3, dtype=torch.int32, device="cuda")
    w = kernels.arap_weights(Vd, Fd)
    assert int(w.status.item()) == 0 and w.rowptr.tolist() == [0] * (nV + 1)
    pc = kernels.mesh_principal_curvature(Vd, Fd, radius=2)
    want = mesh_ops.principal_curvatures(V[:nV], np.zeros((nF, 3), np.int32), radius=2)
    assert int(pc["status"].item()) == want.status == (kernels.CURV_NO_NORMAL if nV else 0)
    assert _same_bytes(pc["ring_size"], want.ring_size)
