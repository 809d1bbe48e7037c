"""The written definition of the sparse x sparse product (include/sn_spmm.h, emulated in tests/amplify_cases.py) against the host
function dense_correspondence.amplify_sequence, i.e. scipy, on the stored Laplacians of tests/amplify_cases.py.

Why matrix 2 is held to a bound and not to bits: scipy's csr_matmat returns UNSORTED rows, and the second squaring then sums
over its left operand in that storage order, the definition in ascending column order.  Matrices 0 and 1 (three scalings and a
squaring whose operand has ascending columns) agree bit for bit, pattern included; the entries of matrix 2 stay within
2 gamma_n T (amplify_cases.product_bound), no entry exists on one side only, and both orders drop the same exact-zero sums."""
import numpy as np
import pytest

import amplify_cases as ac
from surfacenetworks_amd import dense_correspondence as dc


def _host(kind, name):
    out = []
    for M in dc.amplify_sequence(ac.laplacian(kind, name)):
        M = M.copy()
        M.sort_indices()
        out.append(M)
    return out


@pytest.mark.parametrize("kind,name", ac.CASES)
def test_emulation_against_host_sequence(kind, name):
    host = _host(kind, name)
    (M0, M1, M2), (S1, S2), dropped = ac.emulated_sequence(kind, name)
    for t, (E, H) in enumerate(((M0, host[0]), (M1, host[1]))):
        assert H.data.dtype == np.float32 and E.shape == H.shape
        assert ac.same_csr(E, H.indptr, H.indices, H.data), f"matrix {t} differs from scipy's"
    ratio, one_sided = ac.compare_within_bound(M2, host[2], ac.product_bound(S2, S2))
    longest = [int(np.diff(M.indptr).max()) for M in (M0, M1, M2)]
    differ = int((abs(M2.astype(np.float64) - host[2].astype(np.float64)).data != 0).sum())
    print(f"{kind}/{name}: longest rows {longest}, matrix 2: {differ} of {M2.nnz} values differ, worst {ratio:.3f} of the bound, "
          f"{one_sided} one-sided entries, dropped zero sums {dropped}")
    assert ratio <= 1.0
    assert one_sided <= 0.01 * M2.nnz


def test_flat_grid_drops_exact_zero_sums():
    """scipy drops a structural entry whose fp32 sum is exactly zero; so does the definition, and they drop the same ones.
    The mesh is the flat 12 x 9 grid: the jittered 12 x 9 torus_grid of this repository has no such sum (amplify_cases.torus)."""
    (M0, M1, M2), _, dropped = ac.emulated_sequence("ext", "flat")
    print("dropped exact-zero sums per squaring:", dropped, "torus:", ac.emulated_sequence("ext", "torus")[2])
    assert sum(dropped) >= 1
    host = _host("ext", "flat")
    assert M2.nnz == host[2].nnz and np.array_equal(M2.indptr, host[2].indptr) and np.array_equal(M2.indices, host[2].indices)


def test_bipyramid_rows_cover_the_matrix():
    (M0, M1, M2), _, _ = ac.emulated_sequence("ext", "bipyramid")
    assert int(np.diff(M0.indptr).max()) == 97 and (np.diff(M1.indptr) == 98).all() and (np.diff(M2.indptr) == 98).all()


def test_emulated_product_is_the_exact_product_on_small_integers():
    """The emulation itself: integer-valued operands make every fp32 operation exact, so any order gives scipy's product."""
    rng = np.random.default_rng(3)
    import scipy.sparse as sp

    A = sp.random(23, 31, 0.2, random_state=rng, data_rvs=lambda n: rng.integers(-4, 5, n)).astype(np.float32).tocsr()
    B = sp.random(31, 17, 0.2, random_state=rng, data_rvs=lambda n: rng.integers(-4, 5, n)).astype(np.float32).tocsr()
    for X in (A, B):
        X.sort_indices()
    C = ac.emulate_spgemm(A, B, keep_zeros=True)
    assert (np.diff(C.indices)[np.diff(np.repeat(np.arange(23), np.diff(C.indptr))) == 0] > 0).all()      # ascending
    assert abs(C - A @ B).sum() == 0
    ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    assert C.nnz == (ones(A) @ ones(B)).nnz                          # the structural pattern, explicit zeros of A and B included
    assert ac.emulate_spgemm(A, B).nnz == np.count_nonzero(C.data)
