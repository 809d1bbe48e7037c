"""Host part of the dense-correspondence evaluation (predicted matches and their geodesic error): the cumulative curve and the
true matches against restatements in numpy, the refusal of CPU tensors, and the two new C entry points in the header, the
ctypes table and the launch-plan table.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from surfacenetworks_amd import dense_correspondence as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _curve(err, th):
    e = np.asarray(err, np.float64)
    e = e[np.isfinite(e)]
    return np.array([np.mean(e <= np.float32(t)) if e.size else np.nan for t in th])


def test_curve_matches_the_numpy_restatement():
    rng = np.random.default_rng(0)
    err = rng.random(257).astype(np.float32)
    err[::7] = 0.0                                               # exact matches
    err[3::11] = np.nan                                          # vertices without a true match
    err[5] = np.inf
    th = [0.0, 0.1, 0.25, float(err[2]), 0.999, 1.0, 7.0, float("inf"), -1.0]
    got = dc.correspondence_curve(torch.from_numpy(err), th)
    assert got.dtype == torch.float64 and got.shape == (len(th),)
    assert np.array_equal(got.numpy(), _curve(err, th))
    assert got[-1].item() == 0.0 and got[-2].item() == 1.0       # below every error; +inf counts the finite errors only
    # thresholds as a tensor, unsorted
    th2 = torch.tensor([0.5, 0.2, 0.9])
    assert np.array_equal(dc.correspondence_curve(torch.from_numpy(err), th2).numpy(), _curve(err, th2.numpy()))


def test_curve_of_no_finite_error_is_nan():
    for err in (torch.empty(0), torch.full((4,), float("nan"))):
        got = dc.correspondence_curve(err, [0.0, 1.0])
        assert got.shape == (2,) and torch.isnan(got).all()
    assert dc.correspondence_curve(torch.tensor([0.5, 2.0]), []).shape == (0,)


def test_true_matches_on_hand_written_labels():
    # A: vertex r carries label lA[r]; B: label c sits at vertex liB[c]
    lA = torch.tensor([2, 0, 3, 1, 4])
    lB = torch.tensor([1, 2, 0])                                 # B has three vertices: labels 3 and 4 have no vertex there
    liB = torch.argsort(lB)                                      # [2, 0, 1]
    got = dc.true_matches([(None, lA, None)], [(None, lB, liB)])
    assert got.dtype == torch.int64 and got.tolist() == [1, 2, -1, 0, -1]
    for r, t in enumerate(got.tolist()):
        assert t == -1 or lB[t] == lA[r]
    # equal counts: liB[lA], main.py:206
    lA, lB = torch.tensor([1, 3, 0, 2]), torch.tensor([3, 2, 1, 0])
    liB = torch.argsort(lB)
    assert torch.equal(dc.true_matches([(None, lA, None)], [(None, lB, liB)]), liB[lA])


def test_geodesic_errors_gather_and_nan():
    GB = torch.arange(9, dtype=torch.float32).reshape(3, 3)
    lA, lB = torch.tensor([2, 0, 3, 1]), torch.tensor([1, 2, 0])
    liB = torch.argsort(lB)
    a2b = torch.tensor([0, 2, 1, 1])
    got = dc.geodesic_errors(a2b, [(None, lA, None)], [(GB, lB, liB)])
    assert got[[0, 1, 3]].tolist() == [GB[1, 0].item(), GB[2, 2].item(), GB[0, 1].item()] and torch.isnan(got[2])
    m = dc.PairMatches(a2b, None, err=torch.zeros(4))
    assert dc.geodesic_errors(m, [(None, lA, None)], [(GB, lB, liB)]) is m.err


def test_matches_to_dataset_order():
    from surfacenetworks_amd import mesh_ops

    class DS:
        orders = [mesh_ops.MeshOrder([2, 0, 1], [0]), mesh_ops.MeshOrder([1, 2, 0], [0])]

    a2b = torch.tensor([0, 2, 1])                 # stored r -> stored a2b[r]: file 2 -> file 1, file 0 -> file 0, file 1 -> file 2
    assert dc.matches_to_dataset_order(DS, 0, 1, a2b).tolist() == [0, 2, 1]
    assert dc.matches_to_dataset_order(DS, 0, 0, a2b).tolist() == [1, 0, 2]
    assert dc.matches_to_dataset_order(object(), 0, 1, a2b) is a2b


def test_cpu_tensors_raise():
    from surfacenetworks_amd import kernels

    FA, FB = torch.zeros(1, 8, 4), torch.zeros(1, 8, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        dc.match_features(FA, FB, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        kernels.pair_match(FA[0], FB[0], 8, 8)


def test_header_ctypes_and_plan_table_agree_on_the_new_symbols():
    import ctypes as C

    from surfacenetworks_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sn_spmm.h")).read(), flags=re.S)
    table = open(os.path.join(ROOT, "surfacenetworks_amd", "csrc", "sn_plan_table.inc")).read()
    ctype = {"size_t": C.c_size_t, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}
    for name in ("sn_pair_match_workspace_bytes", "sn_pair_match_f32"):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in the header"
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)]
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in m.group(2).split(",")]
        assert list(args) == want, name
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert "SN_PLAN_FN(sn_pair_match_f32)\n" in table and "sn_pair_match_workspace_bytes" not in table
    lib = _lib.load()
    assert lib.sn_plan_lookup(b"sn_pair_match_f32") >= 0
    # header | R of both sides | 8 ranges x 4 floats per row of both sides; no transposed copies, no gradient partials
    for ra, rb in ((64, 64), (7000, 7005), (1, 33)):
        pa, pb = (ra + 31) // 32 * 32, (rb + 31) // 32 * 32
        assert lib.sn_pair_match_workspace_bytes(ra, rb) == 256 + (pa + pb) * (128 * 2 * 2 + 8 * 4 * 4)
        assert lib.sn_pair_match_workspace_bytes(ra, rb) < lib.sn_pair_fused_workspace_bytes(ra, rb)
    assert lib.sn_pair_match_workspace_bytes(-1, 4) == 0
