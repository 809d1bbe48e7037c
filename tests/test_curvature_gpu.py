"""Principal curvatures on the device (sn_mesh_principal_curvature_f32) against the numpy statement of the header section
"Principal curvatures": k1, k2, d1, d2 bit for bit (NaN patterns included), ring_size and the status word as integers, no
tolerance anywhere.  Then the layers above: operators.principal_curvatures on batches, operators.curv4 and the input columns of
datasets.normal_frame_from_mesh.  The cases and their host statements are shared (tests/curvature_cases.py)."""
import numpy as np
import pytest
import torch

import curvature_cases as cases
from surfacenetworks_amd import datasets, kernels, mesh_ops, operators

pytestmark = pytest.mark.gpu

FIELDS = ("k1", "k2", "d1", "d2", "ring_size")


def _dev(c):
    return torch.tensor(c.V).cuda(), torch.tensor(c.F).cuda()      # a copy: the cases are read-only arrays


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


def _assert_equal(got, want, who, fields=FIELDS):
    for name in fields:
        g, w = _bits(getattr(got, name)), _bits(getattr(want, name))
        assert g.shape == w.shape, (who, name)
        rows = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert rows.size == 0, f"{who}: {name} differs at {rows.size} vertices, first {rows[:8]}"
    assert int(got.status.item()) == want.status, (who, int(got.status.item()), want.status)


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_equals_the_host_statement_bit_for_bit(name):
    V, F = _dev(cases.case(name))
    for radius in cases.radii(name):
        _assert_equal(operators.principal_curvatures(V, F, radius), cases.host(name, radius), f"{name} radius {radius}")


def test_the_sums_follow_the_ids_not_the_search():
    """disc with its vertices renumbered at random: the device equals the host statement of the renumbered mesh, whose patches
    are those of disc under the renumbering."""
    V, F = _dev(cases.case("disc_permuted"))
    for radius in (2, 5):
        got = operators.principal_curvatures(V, F, radius)
        _assert_equal(got, cases.host("disc_permuted", radius), f"disc_permuted radius {radius}")
        base = cases.host("disc", radius)
        perm = cases.permutation()
        assert np.array_equal(got.ring_size.cpu().numpy(), base.ring_size[perm])


@pytest.mark.parametrize("name,radius", [("disc", 5), ("big", cases.BIG_RADIUS)])
def test_two_runs_are_bit_identical(name, radius):
    V, F = _dev(cases.case(name))
    a, b = operators.principal_curvatures(V, F, radius), operators.principal_curvatures(V, F, radius)
    for f in FIELDS:
        assert torch.equal(_as_int(getattr(a, f)), _as_int(getattr(b, f))), f
    assert torch.equal(a.status, b.status)


def _as_int(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_one_output_alone_equals_it_among_all():
    V, F = _dev(cases.case("junk"))
    everything = operators.principal_curvatures(V, F, 2)
    for f in FIELDS:
        alone = operators.principal_curvatures(V, F, 2, want=[f])
        assert torch.equal(_as_int(getattr(alone, f)), _as_int(getattr(everything, f))), f
        assert all(getattr(alone, g) is None for g in FIELDS if g != f)
        assert torch.equal(alone.status, everything.status)
    none = operators.principal_curvatures(V, F, 2, want=[])
    assert all(getattr(none, g) is None for g in FIELDS) and torch.equal(none.status, everything.status)
    with pytest.raises(ValueError):
        operators.principal_curvatures(V, F, 2, want=["k3"])
    with pytest.raises(ValueError):
        operators.principal_curvatures(V, F, 0)


def test_numpy_input_and_kernel_entry():
    c = cases.case("torus_jitter")
    _assert_equal(operators.principal_curvatures(c.V, c.F, 2), cases.host("torus_jitter", 2), "numpy input")
    V, F = _dev(c)
    out = kernels.mesh_principal_curvature(V, F, 2, want=["k1"])
    assert out["k2"] is None and out["status"].is_cuda and _bits(out["k1"]).tobytes() == _bits(cases.host("torus_jitter", 2).k1).tobytes()


def test_batch_equals_single_calls():
    c = cases.case("batch")
    V, F = _dev(c)
    for radius in (2, 5):
        got = operators.principal_curvatures(V, F, radius)
        want = cases.host("batch", radius)
        per_mesh = torch.stack([torch.tensor(c.F)] * 3).cuda()
        again = operators.principal_curvatures(V, per_mesh, radius)
        for b in range(3):
            single = operators.principal_curvatures(V[b], F, radius)
            for f in FIELDS:
                assert _bits(getattr(got, f)[b]).tobytes() == _bits(getattr(want[b], f)).tobytes(), (radius, b, f)
                assert torch.equal(_as_int(getattr(got, f)[b]), _as_int(getattr(single, f))), (radius, b, f)
                assert torch.equal(_as_int(getattr(got, f)[b]), _as_int(getattr(again, f)[b])), (radius, b, f)
        assert int(got.status.item()) == want[0].status | want[1].status | want[2].status


def test_a_bad_index_stays_out_of_the_neighbouring_mesh():
    """junk stacked with a copy of itself scaled by 3: the face with an index past nV must not reach into the second mesh, whose
    curvatures are the first's divided by 3 up to rounding and equal its own host statement exactly."""
    c = cases.case("junk_pair")
    V, F = _dev(c)
    got = operators.principal_curvatures(V, F, 2)
    for b in range(2):
        want = mesh_ops.principal_curvatures(c.V[b], c.F, 2)
        for f in FIELDS:
            assert _bits(getattr(got, f)[b]).tobytes() == _bits(getattr(want, f)).tobytes(), (b, f)
        assert int(got.status.item()) == want.status == mesh_ops.DESC_BAD_FACE | mesh_ops.CURV_NO_NORMAL
    assert torch.equal(got.ring_size[0], got.ring_size[1])


def test_curv4_equals_the_host_columns():
    """Both sides form H and K in fp32 from the fp32 curvatures, clip, and divide every column by its largest magnitude in fp32
    (one correctly rounded fp32 division per entry): equal bit for bit."""
    for name, radius in (("torus_jitter", 2), ("disc", 5)):
        c = cases.case(name)
        V, F = _dev(c)
        got = operators.curv4(V, F, radius)
        want = mesh_ops.curv4(c.V, c.F, radius)
        assert got.dtype == torch.float32 and got.shape == (c.V.shape[0], 4)
        assert _bits(got).tobytes() == _bits(want).tobytes(), name
    c = cases.case("batch")
    got = operators.curv4(*_dev(c), 2)
    for b in range(3):                                                   # the scaling is per mesh
        assert _bits(got[b]).tobytes() == _bits(mesh_ops.curv4(c.V[b], c.F, 2)).tobytes()
    with pytest.warns(UserWarning, match="fewer than six"):
        assert operators.curv4(*_dev(cases.case("tetra")), 2) is None


def test_normal_frame_inputs():
    c = cases.case("torus_jitter")
    frame = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "curv4", "N", "G"), curv_radius=2)
    Vd, Fd = frame["V"], frame["F"]
    assert frame["input"].shape == (c.V.shape[0], 11) and frame["input"].dtype == torch.float32
    blocks = (Vd, operators.curv4(Vd, Fd, 2), operators.vertex_normals(Vd, Fd), operators.gaussian_curvature(Vd, Fd).unsqueeze(1))
    assert torch.equal(frame["input"], torch.cat(blocks, dim=1))
    assert torch.equal(frame["input"][:, 7:10], frame["target_dist"])
    default = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "curv4"))               # curv_radius=5
    assert torch.equal(default["input"][:, 3:], operators.curv4(Vd, Fd, 5))
    base = datasets.normal_frame_from_mesh(c.V, c.F)
    assert base["input"] is base["V"] and torch.equal(base["V"], Vd)
    assert torch.equal(datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V",))["input"], base["input"])
    with pytest.raises(ValueError):
        datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "curv3"))


def test_normal_frame_with_wks_is_unchanged():
    c = cases.case("torus_jitter")
    frame = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "wks"), wks_k=12)
    wks = operators.wave_kernel_signature(frame["V"], frame["F"], N=100, eigenpairs=frame["eigenpairs"])
    assert frame["input"].shape == (c.V.shape[0], 103) and torch.equal(frame["input"], torch.cat([frame["V"], wks], dim=1))
    both = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("G", "V", "wks"), wks_k=12)
    assert torch.equal(both["input"][:, 1:4], frame["V"]) and both["input"].shape == (c.V.shape[0], 104)
    assert torch.equal(both["input"][:, 0], operators.gaussian_curvature(frame["V"], frame["F"]))


def test_normal_frame_gives_up_where_curv4_does():
    c = cases.case("tetra")
    with pytest.warns(UserWarning, match="no principal curvatures"):
        assert datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "curv4")) is None
    frame = datasets.normal_frame_from_mesh(c.V, c.F, inputs=("V", "N"))
    assert frame is not None and torch.equal(frame["input"][:, 3:], frame["target_dist"])
