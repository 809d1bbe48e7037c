"""sn_poisson_disc_i32 and sn_mesh_digits_u8 on the MI355X against the host statements, bit for bit, and the dataset built on
them end to end."""
import warnings

import numpy as np
import pytest
import torch

import delaunay_cases as cases
from surfacenetworks_amd import datasets, kernels, mesh_mnist, mesh_ops as mo

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("P", "count", "V", "F", "nF", "status", "attempts")


def _same(dev_out, want):
    for k in FIELDS:
        got, ref = getattr(dev_out, k).cpu().numpy(), getattr(want, k)
        assert got.dtype == ref.dtype and got.shape == ref.shape, k
        assert got.tobytes() == ref.tobytes(), f"{k} differs from the host statement"


@pytest.fixture(scope="module")
def full_images():
    return cases.stroke_images(6)


def test_full_size_images_equal_the_statement(full_images):
    out = kernels.mesh_digits(torch.from_numpy(full_images).to(DEV), seed=0)
    want = mo.mesh_digits(full_images, seed=0)
    _same(out, want)
    assert (want.status == 0).all() and (want.count >= 101).all()
    again = kernels.mesh_digits(torch.from_numpy(full_images).to(DEV), seed=0)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), "two runs differ"
    counts = out.counts.cpu().numpy()
    assert (counts[:, 1] == 0).all() and (counts[:, 3] == 2 * want.count - 2 - want.nF).all()


@pytest.mark.parametrize("seed,r,base", [(3, 1.0, 0), (4, 1.0, 1 << 33), (2 ** 64 - 1, 1.25, 5), (5, 0.8, 0)])
def test_small_images_equal_the_statement(seed, r, base):
    imgs = cases.stroke_images(4, 10, 7)
    R = int(round(r * 65536))
    out = kernels.mesh_digits(torch.from_numpy(imgs).to(DEV), seed=seed, R=R, min_points=20, image_base=base)
    _same(out, mo.mesh_digits(imgs, seed=seed, r=r, min_points=20, image_base=base))


def test_the_large_variant_equals_the_statement(full_images):
    """r = 1.2 on 28 x 28: 1024 cells and a packing bound above 512 samples, so the 1024-point kernel runs (r = 1.5 takes the
    512-point one)."""
    R = int(round(1.2 * 65536))
    assert kernels.poisson_disc_cells(27, 27, R) == 1024 and 4 * (27 * 65536 + R) ** 2 // (3 * R * R) > 512
    out = kernels.mesh_digits(torch.from_numpy(full_images[1:4]).to(DEV), seed=1, R=R, image_base=1)
    want = mo.mesh_digits(full_images[1:4], seed=1, r=1.2, image_base=1)
    _same(out, want)
    assert (want.status == 0).all() and want.count.min() > 250


def test_sampler_alone_equals_the_statement():
    for r, W, H, attempt in ((1.0, 9, 9, 0), (1.25, 12, 7, 2)):
        s = kernels.poisson_disc(3, seed=9, image_base=4, attempt=attempt, R=int(round(r * 65536)), width=W, height=H)
        P, count, steps = s.P.cpu().numpy(), s.count.cpu().numpy(), s.steps.cpu().numpy()
        for b in range(3):
            w = mo.poisson_disc(9, 4 + b, attempt, r, W, H)
            assert count[b] == w.count and steps[b] == w.steps
            assert np.array_equal(P[b, : w.count], w.P) and not P[b, w.count:].any()
    with pytest.raises(ValueError, match="refused"):
        kernels.poisson_disc(1, width=40, height=40)


def test_a_tight_threshold_drives_a_retry():
    imgs = cases.stroke_images(3, 10, 7)
    want = mo.mesh_digits(imgs, seed=3, r=1.0, min_points=20, min_det=1 << 29)
    assert want.attempts.max() > 0 and (want.status == 0).all()
    out = kernels.mesh_digits(torch.from_numpy(imgs).to(DEV), seed=3, R=65536, min_points=20, min_det=1 << 29)
    _same(out, want)
    assert int(out.attempts.max()) > 0


def test_a_threshold_nothing_meets_ends_rejected():
    imgs = cases.stroke_images(2, 10, 7)
    out = kernels.mesh_digits(torch.from_numpy(imgs).to(DEV), seed=3, R=65536, min_points=20, min_det=1 << 40)
    _same(out, mo.mesh_digits(imgs, seed=3, r=1.0, min_points=20, min_det=1 << 40))
    assert out.status.tolist() == [mo.DT_REJECTED] * 2 and out.attempts.tolist() == [mo.MESHDIGITS_MAX_ATTEMPTS] * 2
    assert not out.count.any() and not out.nF.any()


@pytest.fixture(scope="module")
def eight():
    imgs = np.concatenate([cases.stroke_images(6), cases.stroke_images(4, seed=9)[2:]])
    return imgs, np.arange(8) % 10


@pytest.mark.parametrize("model", ["dir", "lap"])
def test_dataset_from_images_trains_one_step(eight, model):
    imgs, labels = eight
    ds = mesh_mnist.MeshDigits.from_images(imgs, labels, seed=0, device=DEV, model=model)
    assert isinstance(ds, mesh_mnist.MeshDigits) and ds.n == 8 and ds.rejected.size == 0 and ds.labels.tolist() == labels.tolist()
    net = (mesh_mnist.DirModel() if model == "dir" else mesh_mnist.Model()).to(DEV)
    opt = mesh_mnist.make_optimizer(net)
    batch = ds.sample_batch(4, np.random.default_rng(0))
    loss = mesh_mnist.train_step(net, opt, batch)
    assert torch.isfinite(loss).item()
    want = mo.mesh_digits(imgs, seed=0)
    for i in (0, 5):
        o = ds.orders[i]
        V = want.V[i, : want.count[i]] / np.float32(27) - np.array([0.5, 0.5, 0.0], np.float32)
        Vs, Fs = o.mesh(V, want.F[i, : want.nF[i]].astype(np.int64))
        assert np.array_equal(ds.V[i], Vs) and np.array_equal(ds.F[i], Fs)


def test_dataset_operators_equal_the_host_builder(eight):
    imgs, labels = eight
    ds = datasets.mesh_mnist_from_images(imgs, labels, seed=0, device=DEV, model="dir")
    for i in (1, 6):
        D, DA = mo.dirac(ds.V[i].astype(np.float64), ds.F[i].astype(np.int64))
        nv, nf = int(ds.nv[i]), int(ds.nf[i])
        for pool, ref, shape in ((ds.pool_Di, D, (4 * nf, 4 * nv)), (ds.pool_DiA, DA, (4 * nv, 4 * nf))):
            r = ref.astype(np.float32).tocsr()
            r.sort_indices()
            r.eliminate_zeros()
            g = pool.assemble(np.array([i]), *shape).to_scipy()
            g.eliminate_zeros()
            assert np.array_equal(g.indptr, r.indptr) and np.array_equal(g.indices, r.indices) and np.array_equal(g.data, r.data)


def test_chunked_dataset_equals_the_dataset_made_at_once(eight, monkeypatch):
    """Three images per launch instead of all at once: image_base keeps every image on its own random stream."""
    imgs, labels = eight
    whole = datasets.mesh_mnist_from_images(imgs, labels, seed=0, device=DEV, model="dir")
    monkeypatch.setattr(datasets, "_DIGITS_CHUNK", 3)
    parts = datasets.mesh_mnist_from_images(imgs, labels, seed=0, device=DEV, model="dir")
    assert parts.n == whole.n == 8 and torch.equal(parts.xyz, whole.xyz) and torch.equal(parts.labels, whole.labels)
    assert all(np.array_equal(a, b) for a, b in zip(parts.F, whole.F)) and np.array_equal(parts.attempts, whole.attempts)
    ids = np.arange(8)
    nv, nf = int(whole.nv.max()), int(whole.nf.max())
    for a, b in ((parts.pool_Di.assemble(ids, 4 * nf, 4 * nv), whole.pool_Di.assemble(ids, 4 * nf, 4 * nv)),
                 (parts.pool_DiA.assemble(ids, 4 * nv, 4 * nf), whole.pool_DiA.assemble(ids, 4 * nv, 4 * nf))):
        assert all(torch.equal(x, y) for x, y in zip(a.bsr4(), b.bsr4()))
    with pytest.raises(ValueError, match="7 labels for 8 images"):
        datasets.mesh_mnist_from_images(imgs, labels[:7], device=DEV)


def test_samples_round_trip_through_the_reference_layout(eight, tmp_path):
    imgs, labels = eight
    samples = datasets.mesh_digit_samples(imgs[:3], labels[:3], seed=0, device=DEV)
    want = mo.mesh_digits(imgs[:3], seed=0)
    assert len(samples) == 3
    for b, s in enumerate(samples):
        assert s["V"].dtype == np.float32 and s["F"].dtype == np.int32 and s["label"] == labels[b]
        assert np.array_equal(s["V"], want.V[b, : want.count[b]]) and np.array_equal(s["F"], want.F[b, : want.nF[b]])
    path = str(tmp_path / "train_plus.np")
    datasets.write_mesh_mnist(path, [(s["V"].astype(np.float64) / 27 - np.array([0.5, 0.5, 0.0]), s["F"]) for s in samples],
                              [s["label"] for s in samples])
    ds = datasets.mnist_from_samples(datasets.load_mesh_mnist(path), device=DEV, model="dir")
    assert ds.n == 3 and ds.nv.tolist() == want.count.tolist() and ds.nf.tolist() == want.nF.tolist()
    batch = ds.sample_batch(2, np.random.default_rng(1))
    assert batch.inputs.shape[0] == 2 and batch.Di is not None


def test_rejected_images_are_left_out_and_named(eight, monkeypatch):
    imgs, labels = eight
    monkeypatch.setattr(kernels, "MESHDIGITS_MIN_DET", 1 << 40)          # nothing passes: every image ends rejected
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        samples = datasets.mesh_digit_samples(imgs[:2], labels[:2], seed=0, device=DEV)
    assert samples == [] and any("left out: [0, 1]" in str(x.message) for x in w)
    with pytest.raises(ValueError, match="no image gave a mesh"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        datasets.mesh_mnist_from_images(imgs[:2], labels[:2], device=DEV)
