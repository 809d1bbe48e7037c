"""Host statements of the integer Poisson-disc sampler, the intensity and the Mesh-MNIST maker (mesh_ops.poisson_disc,
lattice_intensity, mesh_digits; include/sn_spmm.h, "Lattice Delaunay and the Mesh-MNIST maker").  No GPU."""
import numpy as np
import pytest

import delaunay_cases as cases
from surfacenetworks_amd import mesh_ops as mo

Q = mo.MESHDIGITS_Q
PARAMS = [(1.5, 27, 27, 0), (1.0, 9, 9, 3), (1.25, 12, 7, 1)]


@pytest.fixture(scope="module")
def samples():
    return {p: mo.poisson_disc(7, 5, p[3], p[0], p[1], p[2]) for p in PARAMS}


@pytest.mark.parametrize("p", PARAMS)
def test_sampler_keeps_its_promises(samples, p):
    r, W, H, _ = p
    s = samples[p]
    R, cell, gw, gh = mo.poisson_grid(r, W, H)
    pts = [(int(x), int(y)) for x, y in s.P]
    assert s.count == len(pts) and s.P.dtype == np.int32
    assert all(0 < x < W * Q and 0 < y < H * Q for x, y in pts), "a sample is not strictly inside the domain"
    d2 = min((ax - bx) ** 2 + (ay - by) ** 2 for i, (ax, ay) in enumerate(pts) for bx, by in pts[:i])
    assert d2 >= R * R, "two samples are closer than R"
    assert len({(x // cell, y // cell) for x, y in pts}) == len(pts), "two samples share a cell"
    assert len(pts) <= gw * gh and 1 <= s.steps <= 2 * gw * gh and s.steps == 2 * len(pts) - 1
    assert 2 * cell * cell <= R * R < 2 * (cell + 1) ** 2 and cell * 2 > R


def test_full_size_sample_count(samples):
    assert 180 <= samples[PARAMS[0]].count <= 240                # about 200 points per 27 x 27 image


def test_seed_image_and_attempt_key_the_stream():
    a = mo.poisson_disc(7, 5, 3, 1.0, 9, 9)
    assert np.array_equal(a.P, mo.poisson_disc(7, 5, 3, 1.0, 9, 9).P)
    for other in (mo.poisson_disc(8, 5, 3, 1.0, 9, 9), mo.poisson_disc(7, 6, 3, 1.0, 9, 9), mo.poisson_disc(7, 5, 4, 1.0, 9, 9)):
        assert other.P.shape != a.P.shape or not np.array_equal(other.P, a.P)
    d = [mo.lattice_draw(1, 2, 3, 4, 5, 6, p) for p in range(5)]
    assert len(set(d)) == 5 and all(0 <= v < 2 ** 64 for v in d)


def test_parameters_outside_the_lattice_are_refused():
    with pytest.raises(ValueError, match="cells exceed"):
        mo.poisson_grid(1.5, 40, 40)
    with pytest.raises(ValueError, match="outside the lattice"):
        mo.poisson_grid(1.5, 256, 4)


def test_intensity_at_whole_pixels_is_the_pixel():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(28, 28)).astype(np.uint8)
    ij = [(i, j) for i in range(27) for j in range(27)]
    z = mo.lattice_intensity(img, [(i * Q, j * Q) for i, j in ij])
    want = np.array([np.float32(np.float64(int(img[27 - j, i])) / 255.0) for i, j in ij], np.float32)
    assert z.dtype == np.float32 and np.array_equal(z, want)
    # half way between two columns / two rows: the mean of the two pixels, exactly representable sums
    z = mo.lattice_intensity(img, [(3 * Q + Q // 2, 5 * Q), (3 * Q, 5 * Q + Q // 2)])
    assert z[0] == np.float32((int(img[22, 3]) + int(img[22, 4])) / 510.0)
    assert z[1] == np.float32((int(img[22, 3]) + int(img[21, 3])) / 510.0)


@pytest.fixture(scope="module")
def small_images():
    return cases.stroke_images(4, 10, 7)


def test_maker_meshes_pass_the_quality_test(small_images):
    r = mo.mesh_digits(small_images, seed=3, r=1.0, min_points=20)
    assert r.P.shape == (4, 169, 2) and r.V.shape == (4, 169, 3) and r.F.shape == (4, 338, 3)
    for b in range(4):
        assert r.status[b] == 0 and 0 <= r.attempts[b] < mo.MESHDIGITS_MAX_ATTEMPTS and r.count[b] >= 20
        P, F = r.P[b, : r.count[b]], r.F[b, : r.nF[b]]
        cases.check_triangulation(P, F)
        assert min(cases.orient(P[i], P[j], P[k]) for i, j, k in F.tolist()) > mo.MESHDIGITS_MIN_DET
        assert np.array_equal(r.V[b, : r.count[b], :2], (P / 65536.0).astype(np.float32))
        assert np.array_equal(r.V[b, : r.count[b], 2], mo.lattice_intensity(small_images[b], P))
        assert not r.P[b, r.count[b]:].any() and not r.V[b, r.count[b]:].any() and (r.F[b, r.nF[b]:] == -1).all()
        s = mo.poisson_disc(3, b, int(r.attempts[b]), 1.0, 9, 9)
        assert np.array_equal(s.P, P)
    assert (r.V[0, :, 2] == 0).all() and (r.V[1, : r.count[1], 2] == 1).all()        # the all-zero and the all-255 image


def test_a_tight_threshold_drives_retries_and_rejection(small_images):
    r = mo.mesh_digits(small_images[:3], seed=3, r=1.0, min_points=20, min_det=1 << 29)
    assert (r.status == 0).all() and r.attempts.max() > 0
    r = mo.mesh_digits(small_images[:2], seed=3, r=1.0, min_points=20, min_det=1 << 40)
    assert (r.status == mo.DT_REJECTED).all() and (r.attempts == mo.MESHDIGITS_MAX_ATTEMPTS).all()
    assert not r.count.any() and not r.nF.any() and (r.F == -1).all() and not r.V.any()
    r = mo.mesh_digits(small_images[:1], seed=3, r=1.0, min_points=170)                  # more points than cells
    assert r.status[0] == mo.DT_REJECTED


def test_full_size_image():
    imgs = cases.stroke_images(3)[2:]
    r = mo.mesh_digits(imgs, seed=0, image_base=2)
    assert r.status[0] == 0 and r.count[0] >= 101 and r.P.shape[1] == 676
    cases.check_triangulation(r.P[0, : r.count[0]], r.F[0, : r.nF[0]])
