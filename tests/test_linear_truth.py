"""The bound tests/test_linear_forms_gpu.py holds the Linear kernels to separates a right two-piece product from a subtly wrong
one — shown on the numpy model of the split (linear_truth.split_model), without a GPU: the faithful model stays within HALF the
bound, and a model that loses ONE of the two correction products (x high · W low, or x low · W high) exceeds FOUR times the
bound on the same operands."""
import numpy as np
import pytest

import linear_truth as lt

ROWS = 257


@pytest.mark.parametrize("flavour", ["plain", "magnitudes"])
@pytest.mark.parametrize("J", [128, 120, 64, 4])
@pytest.mark.parametrize("K", [128, 256])
def test_the_bound_separates_the_faithful_split_from_a_lost_correction_product(K, J, flavour):
    ops = lt.fwd_operands(ROWS, K, J, flavour, "cpu")
    x, W = ops["x"].numpy(), ops["W"].numpy()
    ref = x.astype(np.float64) @ W.astype(np.float64).T
    tol = lt.tol_of(np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T, K)      # no epilogue: scale = S
    assert (tol > 0).all()
    ratio = {}
    for name, drop in (("faithful", ()), ("hl", ("hl",)), ("lh", ("lh",))):
        got = lt.split_model(x, W, drop=drop).astype(np.float64)
        assert np.isfinite(got).all()
        ratio[name] = float((np.abs(got - ref) / tol).max())
    print(f"split model K={K} J={J} {flavour}: err / tol  faithful {ratio['faithful']:.3f}  without x_hi·W_lo {ratio['hl']:.1f}  "
          f"without x_lo·W_hi {ratio['lh']:.1f}")
    assert ratio["faithful"] <= 0.5, ratio
    assert ratio["hl"] > 4.0 and ratio["lh"] > 4.0, ratio


def test_forward_form_query_follows_the_row_threshold():
    """sn_linear_small_rows / sn_linear_fwd_form (host-only queries): SMALL up to the threshold, large above it, the eight-wave
    kernel only for K = 256 launches above it that write nothing but the activated copy — and 0 throughout on the A/B baseline."""
    from surfacenetworks_amd import kernels

    R = kernels.linear_small_rows()
    assert R >= 32
    split = kernels._split_gemm()
    want = (lambda f: f) if split else (lambda f: 0)
    for K in (128, 256):
        for J in (128, 120, 4):
            assert kernels.linear_fwd_form(33, K, J) == want(1) and kernels.linear_fwd_form(R, K, J, y_elu=True) == want(1)
            assert kernels.linear_fwd_form(R + 1, K, J, residual=True, y_elu=True) == want(2)
    copy = dict(want_y=False, y_elu=True)
    assert kernels.linear_fwd_form(R + 1, 256, 128, **copy) == want(3) and kernels.linear_fwd_form(R, 256, 128, **copy) == want(1)
    for other in (dict(K=128), dict(J=120), dict(residual=True), dict(tile_sums=True), dict(want_y=True), dict(y_elu=False)):
        args = dict(K=256, J=128, residual=False, tile_sums=False, **copy)
        args.update(other)
        assert kernels.linear_fwd_form(R + 1, **args) == want(2), other


def test_split_model_pieces_and_scales():
    """The model's own pieces: the scale brings a row's maximum into [2^13, 2^14), two pieces hold an fp32 value to 2^-22 of the
    row's maximum, and power-of-two row / column factors leave the arithmetic unchanged (what `magnitudes` relies on)."""
    m = np.array([1.0, 0.75, 3e-9, 6e4, 2.0 ** -30], np.float32)
    s = m * lt.pow2_up(m)
    assert ((s >= 2.0 ** 13) & (s < 2.0 ** 14)).all()
    ops = lt.fwd_operands(64, 128, 8, "plain", "cpu")
    x, W = ops["x"].numpy(), ops["W"].numpy()
    a = x * lt.pow2_up(np.abs(x).max(1))[:, None]
    H, L = lt._pieces(a)
    assert np.abs(a.astype(np.float64) - (H.astype(np.float64) + L.astype(np.float64) / 2048)).max() <= 2.0 ** 14 * 2.0 ** -22
    rf, cf = lt.row_factors(64, "cpu").numpy(), lt.col_factors(8, "cpu").numpy()
    y = lt.split_model(x, W)
    assert np.array_equal(lt.split_model(x * rf[:, None], W * cf[:, None]), y * rf[:, None] * cf[None, :])
