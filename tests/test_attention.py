"""Graph attention, host side (no GPU): the torch statement of the definition against an independent dense statement, the
state_dict layout of the model, the refused options, and the binding of the new entry points."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import attention_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_ENTRIES = ("sn_attn_supported", "sn_attn_elu_scores_f32", "sn_attn_propagate_fwd_f32", "sn_attn_propagate_bwd_workspace_bytes",
                "sn_attn_propagate_bwd_f32")


def _cloth20():
    M = ac.cloth_laplacian(5, 4, seed=4)
    assert M.shape == (20, 20)
    return M


def _with_empty_rows():
    """The 20-vertex cloth with the rows of vertices 0, 6 and 19 emptied (their columns stay referenced)."""
    M = _cloth20().tolil()
    for r in (0, 6, 19):
        M.rows[r], M.data[r] = [], []
    M = M.tocsr()
    assert np.diff(M.indptr)[[0, 6, 19]].tolist() == [0, 0, 0] and M.nnz > 0
    return M


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("make", [_cloth20, _with_empty_rows], ids=["cloth20", "empty_rows"])
def test_reference_statement_equals_the_dense_statement(make, heads):
    from surfacenetworks_amd import attention

    M = make()
    x, a, _ = ac.operands(20, 16, seed=9)
    x, a = x.double(), a.double()
    got = attention.attn_propagate_reference(ac.host_operator(M), x, a, heads)
    want = ac.dense_statement(M, x, a, heads)
    assert got.shape == want.shape == (20, 32) and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12
    empty = np.flatnonzero(np.diff(M.indptr) == 0)
    assert not got[torch.from_numpy(empty), 16:].any()                # a row without entries is exactly zero
    assert float(got[:, 16:].abs().max()) > 0.1                       # (the comparison is not between zeros)


def test_reference_statement_ignores_the_values_and_counts_explicit_zeros():
    from surfacenetworks_amd import attention

    M = _cloth20()
    x, a, _ = ac.operands(20, 16, seed=9)
    Z = sp.csr_matrix((np.zeros_like(M.data), M.indices, M.indptr), shape=M.shape)      # every entry an explicit zero
    a_, b_ = (attention.attn_propagate_reference(ac.host_operator(m), x.double(), a.double(), 4) for m in (M, Z))
    assert torch.equal(a_, b_)


def test_state_dict_is_lap_deep_plus_the_score_vectors():
    from surfacenetworks_amd import attention
    from surfacenetworks_amd import normal_predict as NP

    mine = attention.LapGatModel(layers=3).state_dict()
    lap = NP.LapDeepModel(layers=3).state_dict()
    extra = {"rn0.att0", "rn0.att1", "rn2.att0", "rn2.att1"}
    assert set(mine) == set(lap) | extra
    assert all(mine[k].shape == lap[k].shape for k in lap)
    assert all(tuple(mine[k].shape) == (2, 128) for k in extra)
    restated = ac.RefLapGat(3, 3, 3).state_dict()
    assert list(restated) == list(mine) and all(restated[k].shape == mine[k].shape for k in mine)
    att = attention.GatResNet2(128).att0.detach()
    bound = 1.414 * (6.0 / (16 + 16)) ** 0.5                         # xavier_uniform_ on the (2 H, C / H) = (16, 16) view
    assert float(att.abs().max()) <= bound and float(att.abs().max()) > 0.5 * bound


def test_refused_options_raise():
    from surfacenetworks_amd import attention
    from surfacenetworks_amd import normal_predict as NP

    for heads in (3, 64):                                            # 128 % 3 != 0; 128 / 64 = 2 channels per head
        with pytest.raises(ValueError, match="heads"):
            attention.GatResNet2(128, heads=heads)
        with pytest.raises(ValueError, match="heads"):
            attention.LapGatModel(layers=1, heads=heads)
    with pytest.raises(TypeError, match="sparse operator"):
        attention.GatResNet2(16, heads=2)(torch.eye(5).unsqueeze(0), None, torch.zeros(1, 5, 16))
    with pytest.raises(ValueError, match="in_features"):
        attention.LapGatModel(in_features=2)
    with pytest.raises(NotImplementedError, match=r"normal_predict\.GatDeepModel.*attention\.LapGatModel"):
        NP.GatDeepModel()
    attention.LapGatModel(in_features=6, layers=1)                   # more input channels than three are taken


def test_cpu_tensors_and_bad_shapes_are_refused_before_any_launch():
    from surfacenetworks_amd import attention

    op = ac.host_operator(_cloth20())
    x, a, _ = ac.operands(20, 16, seed=9)
    with pytest.raises(RuntimeError, match="no CPU"):
        attention.attn_propagate(op, x, a, 4)
    with pytest.raises(ValueError):
        attention.attn_propagate(op, x[:, :6].contiguous(), a[:, :6].contiguous(), 1)          # C = 6
    with pytest.raises(ValueError):
        attention.attn_propagate(op, x, a, 8)                                                  # C / H = 2
    with pytest.raises(ValueError):
        attention.attn_propagate(op, x[:19], a, 4)                                             # rows do not fit the operator
    with pytest.raises(ValueError):
        attention.attn_propagate_reference(op, x, a[:, :8], 4)


def test_new_entry_points_are_declared_bound_and_planned():
    import ctypes

    from surfacenetworks_amd import _lib, constants

    full = open(os.path.join(ROOT, "include", "sn_spmm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    lib = _lib.load()
    for name in ATTN_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name), name
        launcher = _lib.SIGNATURES[name][0] is ctypes.c_int and name.endswith("_f32")
        assert (f"SN_PLAN_FN({name})\n" in table) == launcher, name
        assert (lib.sn_plan_lookup(name.encode()) >= 0) == launcher, name
    assert "Graph attention" in full and constants.ATTN_SLOPE == 0.2 and constants.ATTN_MAX_CHANNELS == 256
    # the supported set, asked of the library and of the package
    from surfacenetworks_amd import attention

    for C, H in [(16, 1), (16, 4), (128, 8), (128, 32), (256, 1), (4, 1), (24, 2), (6, 1), (128, 3), (128, 64), (260, 1), (0, 1)]:
        assert bool(lib.sn_attn_supported(C, H)) == attention.heads_supported(C, H) == \
            (4 <= C <= 256 and C % 4 == 0 and C % H == 0 and (C // H) % 4 == 0), (C, H)
    # argument errors come back as status codes, before any launch (no device needed)
    fwd, bwd = lib.sn_attn_propagate_fwd_f32, lib.sn_attn_propagate_bwd_f32
    assert lib.sn_attn_elu_scores_f32(None, 6, None, 4, 6, 1, None, 6, None, None) == -7              # SN_E_UNSUPPORTED: C = 6
    assert lib.sn_attn_elu_scores_f32(None, 16, None, 4, 16, 8, None, 16, None, None) == -7           # C / H = 2
    assert lib.sn_attn_elu_scores_f32(None, 8, None, 4, 16, 4, None, 16, None, None) == -4            # SN_E_LD
    assert lib.sn_attn_elu_scores_f32(None, 16, None, 4, 16, 4, None, 16, None, None) == -1           # SN_E_NULL
    assert lib.sn_attn_elu_scores_f32(None, 16, None, 0, 16, 4, None, 16, None, None) == 0            # nothing to do
    assert fwd(None, None, 4, 5, 0, None, 16, None, 16, 4, None, 16, None, None, None) == -2           # SN_E_SHAPE: not square
    assert fwd(None, None, 4, 4, 0, None, 16, None, 260, 1, None, 260, None, None, None) == -7
    assert fwd(None, None, 4, 4, 0, None, 16, None, 16, 4, None, 16, None, None, None) == -1
    assert bwd(None, None, None, None, 4, 5, 0, None, 16, None, 0, None, 16, None, 16, None, None, None, None, 16, 4, None, 16, None,
               None, 0, None) == -2
    assert lib.sn_attn_propagate_bwd_workspace_bytes(0, 6, 1) == 0
    rows, C, H = 1000, 128, 8
    assert lib.sn_attn_propagate_bwd_workspace_bytes(rows, C, H) >= rows * H * 5 * 4        # q (R, H, 4) and ds_dst (R, H)
