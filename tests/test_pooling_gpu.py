"""Sibling-pair pooling on the device (functional.pool_max2, functional.unpool2_add; include/sn_spmm.h "Sibling-pair pooling")
against torch's own MaxPool1d(2, 2) and F.interpolate(scale_factor=2) + add on the same device and the same tensors: forward
and backward equal element for element — ties, infinities and a NaN in either slot included — for every kernel form (16-byte
items, single floats, more than one workgroup, a width that is no multiple of 4)."""
import pytest
import torch

from cascade_cases import torch_pool, torch_unpool_add      # torch's own forms, as the reference writes them

pytestmark = pytest.mark.gpu

DEV = "cuda"
#        one pair      C % 4 == 0   scalar form  the model's width   C = 130: scalar, ld not 4 | 16-byte   > 1 workgroup per pass
SHAPES = [(1, 2, 1), (2, 6, 4), (2, 6, 3), (3, 10, 128), (2, 4, 130), (1, 2 * 4099, 4)]


def _planted(shape, seed):
    """Random values with, where the tensor is large enough, planted pairs (first row, second row) in column 0: an exact tie,
    +-0, +-inf in each slot, and a NaN in the first slot, the second slot and both."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    inf, nan = float("inf"), float("nan")
    pairs = [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (inf, 1.0), (1.0, inf), (-inf, 1.0), (1.0, -inf), (inf, inf), (nan, 0.0), (0.0, nan),
             (nan, nan), (nan, inf), (-inf, nan)]
    flat = x.view(-1, shape[2])
    for k, (a, b) in enumerate(pairs):
        if 2 * k + 1 < flat.shape[0]:
            c = k % shape[2]
            flat[2 * k, c], flat[2 * k + 1, c] = a, b
    return x.to(DEV)


def _same(a, b):
    """torch.equal with NaN equal to NaN (and nowhere else)."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=0.0, posinf=float("inf"), neginf=-float("inf")),
                    torch.nan_to_num(b, nan=0.0, posinf=float("inf"), neginf=-float("inf")))


@pytest.mark.parametrize("shape", SHAPES)
def test_pool_max2_equals_maxpool1d(shape):
    from surfacenetworks_amd import functional as snF

    x = _planted(shape, 1)
    g = torch.randn(shape[0], shape[1] // 2, shape[2], generator=torch.Generator().manual_seed(2)).to(DEV)
    got, want = [], []
    for fn, out in ((snF.pool_max2, got), (torch_pool, want)):
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        y.backward(g)
        out += [y.detach(), xi.grad]
    assert got[0].shape == (shape[0], shape[1] // 2, shape[2]) and got[0].is_contiguous()
    assert _same(got[0], want[0]), shape
    assert _same(got[1], want[1]), shape
    # the signed zeros of a tie keep the first element's bits, as torch's
    assert torch.equal(torch.signbit(got[0]), torch.signbit(want[0]))
    # every element of the input gradient is written: exactly one of each pair carries g, the other an exact zero
    gx = got[1].view(shape[0], shape[1] // 2, 2, shape[2])
    assert bool(((gx[:, :, 0] == 0) | (gx[:, :, 1] == 0)).all()) and torch.equal(gx[:, :, 0] + gx[:, :, 1], g)


@pytest.mark.parametrize("shape", SHAPES)
def test_unpool2_add_equals_interpolate_plus_add(shape):
    from surfacenetworks_amd import functional as snF

    B, V, C = shape
    skip = _planted(shape, 3)
    x = _planted((B, V // 2, C), 4) if V >= 4 else torch.randn(B, V // 2, C, generator=torch.Generator().manual_seed(4)).to(DEV)
    g = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    got, want = [], []
    for fn, out in ((snF.unpool2_add, got), (torch_unpool_add, want)):
        xi, si = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
        y = fn(xi, si)
        y.backward(g)
        out += [y.detach(), xi.grad, si.grad]
    for a, b, name in zip(got, want, ("y", "gx", "gskip")):
        assert _same(a, b), (shape, name)
    assert torch.equal(got[2], g)


def test_only_the_wanted_gradients_are_computed():
    from surfacenetworks_amd import functional as snF

    x = torch.randn(2, 3, 8, device=DEV)
    skip = torch.randn(2, 6, 8, device=DEV, requires_grad=True)
    snF.unpool2_add(x, skip).sum().backward()
    assert x.grad is None and torch.equal(skip.grad, torch.ones_like(skip))


def test_views_with_a_row_pitch_and_other_strides_are_accepted():
    from surfacenetworks_amd import functional as snF

    big = torch.randn(2, 6, 12, device=DEV)
    for view in (big[:, :, :8], big[:, :, 4:12], big[:, :, 1:6], big.transpose(0, 1)[:2], big[:, ::2].expand(2, 3, 12)[:, :2]):
        assert not view.is_contiguous()
        assert torch.equal(snF.pool_max2(view), torch_pool(view)), view.stride()
        coarse = torch.randn(view.shape[0], view.shape[1] // 2, view.shape[2], device=DEV)
        assert torch.equal(snF.unpool2_add(coarse, view), torch_unpool_add(coarse, view)), view.stride()
    # a gradient that arrives as a non-contiguous view
    x = torch.randn(2, 6, 8, device=DEV, requires_grad=True)
    w = torch.randn(8, 2, 3, device=DEV)
    (snF.pool_max2(x) * w.permute(1, 2, 0)).sum().backward()
    xi = x.detach().clone().requires_grad_(True)
    (torch_pool(xi) * w.permute(1, 2, 0)).sum().backward()
    assert torch.equal(x.grad, xi.grad)


def test_refusals():
    from surfacenetworks_amd import functional as snF

    with pytest.raises(ValueError, match="even"):
        snF.pool_max2(torch.zeros(1, 3, 4, device=DEV))
    with pytest.raises(ValueError, match="even"):
        snF.unpool2_add(torch.zeros(1, 1, 4, device=DEV), torch.zeros(1, 3, 4, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        snF.pool_max2(torch.zeros(1, 4, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        snF.unpool2_add(torch.zeros(1, 2, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError):
        snF.pool_max2(torch.zeros(4, 4, device=DEV))
    with pytest.raises(ValueError):
        snF.unpool2_add(torch.zeros(1, 3, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU"):
        snF.pool_max2(torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU"):
        snF.unpool2_add(torch.zeros(1, 2, 4), torch.zeros(1, 4, 4))


def test_a_captured_graph_of_both_kernels_replays_to_the_eager_result():
    from surfacenetworks_amd import functional as snF

    def step(x, skip):
        xi, si = x.detach().requires_grad_(True), skip.detach().requires_grad_(True)
        y = snF.unpool2_add(snF.pool_max2(xi), si)
        y.square().sum().backward()
        return y.detach(), xi.grad, si.grad

    x, skip = torch.randn(2, 12, 128, device=DEV), torch.randn(2, 12, 128, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(x, skip)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x, skip)
    for seed in (7, 8):
        g = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(2, 12, 128, generator=g))
        skip.copy_(torch.randn(2, 12, 128, generator=g))
        graph.replay()
        want = step(x.clone(), skip.clone())
        for a, b in zip(held, want):
            assert torch.equal(a, b)
