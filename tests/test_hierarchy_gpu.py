"""The mesh hierarchy on the device (operators.mesh_hierarchy, sn_mesh_match_f32 + the spgemm products) against its numpy
statement mesh_ops.mesh_hierarchy on the cases of tests/hierarchy_cases.py: equal bit for bit — integers as integers, fp32 by bit
pattern — on every case, level count and mass choice; two runs identical; a batch equals its meshes one by one; levels = 1 is
the identity; max_rounds = 1 raises where more rounds are needed; CPU tensors are refused."""
import numpy as np
import pytest
import torch

import hierarchy_cases as hc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = tuple(hc.cases())


def _device(name, levels, mass_choice, **kw):
    from surfacenetworks_amd import operators
    from surfacenetworks_amd.operators import SparseOperator

    c = hc.cases()[name]
    mass = None if mass_choice is None else torch.from_numpy(c["mass"]).to(DEV)
    return operators.mesh_hierarchy(SparseOperator.from_scipy(c["L"], DEV), levels=levels, mass=mass, blocks=c["blocks"], **kw)


def _same_operator(op, M, what):
    assert tuple(op.shape) == M.shape, what
    assert np.array_equal(op.rowptr.cpu().numpy(), M.indptr), what
    assert np.array_equal(op.colind.cpu().numpy(), M.indices), what
    assert np.array_equal(op.vals.cpu().numpy().view(np.uint32), M.data.astype(np.float32).view(np.uint32)), what


def _equal(h, want, what):
    assert len(h.L) == len(want.L)
    assert h.status == 0 and h.sizes == want.sizes and h.singletons == want.singletons and h.rounds == want.rounds, what
    for k in range(len(want.L)):
        _same_operator(h.L[k], want.L[k], (what, k))
        assert np.array_equal(h.real[k].cpu().numpy(), want.real[k]), (what, k)
        assert np.array_equal(h.positions[k].cpu().numpy(), want.positions[k]), (what, k)
    assert np.array_equal(h.order.cpu().numpy(), want.order) and np.array_equal(h.position.cpu().numpy(), want.position), what


@pytest.mark.parametrize("levels", hc.LEVELS)
@pytest.mark.parametrize("mass_choice", hc.MASSES)
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_statement_bit_for_bit(name, mass_choice, levels):
    _equal(_device(name, levels, mass_choice), hc.statement(name, levels, mass_choice), (name, mass_choice, levels))


def test_two_runs_are_identical():
    a, b = _device("cloth71", 4, "barycentric"), _device("cloth71", 4, "barycentric")
    for k in range(4):
        for x, y in ((a.L[k].rowptr, b.L[k].rowptr), (a.L[k].colind, b.L[k].colind), (a.L[k].vals.view(torch.int32), b.L[k].vals.view(torch.int32)),
                     (a.real[k], b.real[k])):
            assert torch.equal(x, y)
    assert torch.equal(a.order, b.order) and a.rounds == b.rounds and a.singletons == b.singletons


def test_a_batch_equals_its_meshes_one_by_one():
    from surfacenetworks_amd import operators
    from surfacenetworks_amd.operators import SparseOperator

    case = hc.cases()["batch_two_grids"]
    h = _device("batch_two_grids", 4, "barycentric")
    per = h.L[0].shape[0] // 2
    for b, part in enumerate(case["parts"]):
        hb = operators.mesh_hierarchy(SparseOperator.from_scipy(part["L"], DEV), levels=4, mass=torch.from_numpy(part["mass"]).to(DEV))
        for k in range(4):
            lo, hi = (b * per) << k, ((b + 1) * per) << k
            real = lo + torch.nonzero(h.real[k][lo:hi]).reshape(-1)
            mine = torch.nonzero(hb.real[k]).reshape(-1)
            assert torch.equal(real - lo, mine)
            A, C = h.L[k].to_scipy()[real.cpu().numpy()][:, real.cpu().numpy()], hb.L[k].to_scipy()[mine.cpu().numpy()][:, mine.cpu().numpy()]
            assert A.nnz == C.nnz and abs(A - C).max() == 0


def test_levels_one_is_the_identity():
    from surfacenetworks_amd import operators
    from surfacenetworks_amd.operators import SparseOperator

    L = SparseOperator.from_scipy(hc.cases()["grid12"]["L"], DEV)
    h = operators.mesh_hierarchy(L, levels=1)
    assert h.L[0] is L and torch.equal(h.order, torch.arange(L.shape[0], device=DEV)) and bool(h.real[0].all())


def test_max_rounds_and_refusals():
    from surfacenetworks_amd import operators
    from surfacenetworks_amd.operators import SparseOperator

    assert hc.statement("grid12", 2, None).rounds[1] > 1
    with pytest.raises(RuntimeError, match="max_rounds"):
        _device("grid12", 2, None, max_rounds=1)
    c = hc.cases()["grid12"]["L"]
    cpu = SparseOperator(torch.from_numpy(c.indptr), torch.from_numpy(c.indices), torch.from_numpy(c.data), c.shape)
    with pytest.raises(RuntimeError, match="no CPU"):
        operators.mesh_hierarchy(cpu, levels=2)
    with pytest.raises(ValueError):
        operators.mesh_hierarchy(SparseOperator.from_scipy(c, DEV), levels=2, blocks=[3, 4])
    h = _device("grid12", 3, None, pad_coarsest_to=16)
    want = __import__("surfacenetworks_amd.mesh_ops", fromlist=["x"]).mesh_hierarchy(c, levels=3, pad_coarsest_to=16)
    _equal(h, want, "pad_coarsest_to")
    assert h.L[0].shape[0] % 16 == 0
