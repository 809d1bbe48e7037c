"""Predicted matches and their geodesic error from the tower features (sn_pair_match_f32; dense_correspondence.match_features,
evaluate_pair) against src/dense_correspondence/models.py:203 followed by a row / column arg-max, restated on the materialised
product: exactly (int64) where the arithmetic is exact, in float64 under a tie rule otherwise.

The tie rule: tau = 1e-4 max|S64|, ten times the worst-case fp32 bound of a 128-term dot product at this scale.  A prediction
must score within tau of the row's float64 maximum, and must BE the float64 arg-max wherever the float64 runner-up is at least
tau behind; at most 2 % of the rows may be that close (the float64 reference alone: 0 - 0.49 % on these inputs)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

from surfacenetworks_amd import dense_correspondence as dc  # noqa: E402
from surfacenetworks_amd import kernels  # noqa: E402

SHAPES = [(7, 7, 7), (33, 33, 1), (80, 63, 70), (300, 257, 290), (1024, 1000, 1021)]
RANDOM = [(7, 7, 7, 120), (80, 63, 70, 120), (33, 33, 1, 5), (300, 257, 290, 128), (1024, 1000, 1021, 64), (7000, 6890, 6890, 120)]
TAU_REL, EXEMPT_MAX = 1e-4, 0.02


def _features(rows, K, seed):
    """The features of test_pair_losses_gpu._case: N(0, 0.7^2), views with a leading dimension larger than the row."""
    g = torch.Generator().manual_seed(seed)
    FA = (torch.randn(1, rows, K + 8, generator=g) * 0.7).to(DEV)[:, :, :K]
    FB = (torch.randn(1, rows + 5, K + 4, generator=g) * 0.7).to(DEV)[:, :, :K]
    return FA, FB


def _integer_case(rows, NA, NB, K):
    """Integers in [-8, 8]; a third of the scored rows of either side are copies of other rows — among them copies in the other
    half of a tile's columns (j -> j + 4), in another range of the streamed side (j -> j + 128 k) and at the ragged end."""
    g = torch.Generator().manual_seed(rows * 131 + K)
    FA = torch.randint(-8, 9, (1, rows, K + 8), generator=g).float()
    FB = torch.randint(-8, 9, (1, rows + 5, K + 4), generator=g).float()
    for F_, n in ((FA, NA), (FB, NB)):
        pairs = [(0, 4), (1, 129), (2, n - 1), (3, 3 + 128 * 5), (n - 2, 5), (40, 36)]
        src = torch.randint(0, n, (n // 3,), generator=g).tolist()
        dst = torch.randint(0, n, (n // 3,), generator=g).tolist()
        for s_, d_ in pairs + list(zip(src, dst)):
            if 0 <= s_ < n and 0 <= d_ < n:
                F_[0, d_] = F_[0, s_]
    return FA.to(DEV)[:, :, :K], FB.to(DEV)[:, :, :K]


@pytest.mark.parametrize("K", [5, 64, 128])
@pytest.mark.parametrize("rows,NA,NB", SHAPES)
def test_exact_integers_ties_included(rows, NA, NB, K):
    FA, FB = _integer_case(rows, NA, NB, K)
    assert FA.stride(1) > K and FB.stride(1) > K
    # the int64 product: every entry is an integer below 2^53, so the float64 product IS it
    S = (FA[0, :NA].cpu().double().numpy() @ FB[0, :NB].cpu().double().numpy().T).astype(np.int64)
    assert np.abs(S).max() <= 64 * K
    m = dc.match_features(FA, FB, NA, NB, both=True)
    dup_rows = int(((S == S.max(1, keepdims=True)).sum(1) > 1).sum())
    dup_cols = int(((S == S.max(0, keepdims=True)).sum(0) > 1).sum())
    print(f"pairmatch exact rows={rows} K={K}: rows with a duplicated maximum {dup_rows}/{NA}, columns {dup_cols}/{NB}")
    assert NB == 1 or dup_rows >= NA // 8
    assert dup_cols >= NB // 8
    assert m.a2b.dtype == torch.int64 and m.b2a.dtype == torch.int64 and m.err is None
    assert np.array_equal(m.a2b.cpu().numpy(), S.argmax(1)) and np.array_equal(m.b2a.cpu().numpy(), S.argmax(0))
    assert np.array_equal(m.score_a.cpu().numpy().astype(np.float64), S.max(1).astype(np.float64))
    assert np.array_equal(m.score_b.cpu().numpy().astype(np.float64), S.max(0).astype(np.float64))
    one = dc.match_features(FA, FB, NA, NB, both=False)
    assert one.b2a is None and one.score_b is None and torch.equal(one.a2b, m.a2b) and torch.equal(one.score_a, m.score_a)


def _check_direction(S64, pred, best, tau, what):
    """S64: (n, m) float64 on the device; pred / best: the kernel's arg-max and maximum of every row."""
    n, m = S64.shape
    top = torch.topk(S64, min(2, m), dim=1)
    rowmax, am = top.values[:, 0], top.indices[:, 0]
    gap = top.values[:, 0] - top.values[:, 1] if m > 1 else torch.full_like(rowmax, float("inf"))
    assert int(pred.min()) >= 0 and int(pred.max()) < m
    at = S64.gather(1, pred[:, None])[:, 0]
    exempt = gap < tau
    share = exempt.double().mean().item()
    print(f"pairmatch {what}: exempt {share:.4%}, worst score shortfall {(rowmax - at).max().item():.3e}, "
          f"worst |best - max| {(best.double() - rowmax).abs().max().item():.3e}, tau {tau:.3e}")
    assert bool((at >= rowmax - tau).all())
    assert bool(((best.double() - rowmax).abs() <= tau).all())
    assert torch.equal(pred[~exempt], am[~exempt])
    assert share <= EXEMPT_MAX
    return exempt


@pytest.mark.parametrize("rows,NA,NB,K", RANDOM)
def test_random_features_against_float64(rows, NA, NB, K):
    FA, FB = _features(rows, K, rows + K)
    S64 = torch.mm(FA[0, :NA].double(), FB[0, :NB].double().t())
    tau = TAU_REL * S64.abs().max().item()
    m = dc.match_features(FA, FB, NA, NB)
    _check_direction(S64, m.a2b, m.score_a, tau, f"rows={rows} a2b")
    _check_direction(S64.t(), m.b2a, m.score_b, tau, f"rows={rows} b2a")
    m2 = dc.match_features(FA, FB, NA, NB)
    for f in ("a2b", "score_a", "b2a", "score_b"):
        assert torch.equal(getattr(m, f), getattr(m2, f)), f


@pytest.mark.parametrize("rows,NA,NB", [(80, 63, 70), (300, 257, 290), (1024, 1000, 1021)])
def test_padding_never_wins(rows, NA, NB):
    FA, FB = _features(rows, 120, rows)
    clean = dc.match_features(FA, FB, NA, NB)
    FA2, FB2 = FA.clone(), FB.clone()
    FA2[0, NA:] = 1e6
    FB2[0, NB:] = 1e6
    dirty = dc.match_features(FA2, FB2, NA, NB)
    for f in ("a2b", "score_a", "b2a", "score_b"):
        assert torch.equal(getattr(clean, f), getattr(dirty, f)), f


def test_non_finite_features_stay_inside_the_corner():
    FA, FB = _features(80, 120, 3)
    FA, FB = FA.clone(), FB.clone()
    FA[0, 5, 7], FA[0, 9, 0], FB[0, 11, 3] = float("nan"), float("inf"), float("-inf")
    m = dc.match_features(FA, FB, 63, 70)
    assert 0 <= int(m.a2b.min()) and int(m.a2b.max()) < 70 and 0 <= int(m.b2a.min()) and int(m.b2a.max()) < 63


@pytest.mark.parametrize("rows,NA,NB", [(80, 70, 63), (300, 290, 257), (80, 63, 70)])
def test_geodesic_error_path(rows, NA, NB):
    g = torch.Generator().manual_seed(rows + NA)
    FA, FB = _features(rows, 120, rows + 1)
    GB = torch.rand(NB, NB + 12, generator=g).to(DEV)[:, :NB]                    # not symmetric, ldgB > NB
    lA, lB = torch.randperm(NA, generator=g).to(DEV), torch.randperm(NB, generator=g).to(DEV)
    liB = torch.argsort(lB)
    tX, tY = [(None, lA, torch.argsort(lA))], [(GB, lB, liB)]
    truth = dc.true_matches(tX, tY)
    has = lA < NB
    assert torch.equal(truth[has], liB[lA[has]]) and bool((truth[~has] == -1).all())
    assert int((~has).sum()) == max(NA - NB, 0)
    colA, bestA, rowB, bestB, errA = kernels.pair_match(FA[0], FB[0], NA, NB, both=False, geoB=GB, truthA=truth)
    assert rowB is None and bestB is None
    plain = dc.match_features(FA, FB, NA, NB, both=False)
    assert torch.equal(colA, plain.a2b) and torch.equal(bestA, plain.score_a)
    assert torch.equal(torch.isnan(errA), ~has)
    assert torch.equal(errA[has], GB[truth[has], colA[has]])
    via = dc.geodesic_errors(colA, tX, tY)                                       # the separate gather: the same numbers
    assert torch.equal(torch.isnan(via), ~has) and torch.equal(via[has], errA[has])
    m = dc.match_features(FA, FB, NA, NB, geoB=GB, truthA=truth)
    assert dc.geodesic_errors(m, tX, tY) is m.err and torch.equal(m.err[has], errA[has]) and m.b2a is not None


def test_status_codes():
    from surfacenetworks_amd import _lib

    lib = _lib.load()
    f = torch.zeros(64, 120, device=DEV)
    wide = torch.zeros(64, 200, device=DEV)
    geo = torch.zeros(64, 64, device=DEV)
    ci, cj = torch.zeros(64, dtype=torch.int64, device=DEV), torch.zeros(64, dtype=torch.int64, device=DEV)
    truth = torch.zeros(64, dtype=torch.int64, device=DEV)
    ba, bb, err = (torch.zeros(64, device=DEV) for _ in range(3))
    need = lib.sn_pair_match_workspace_bytes(64, 64)
    assert 0 < need < lib.sn_pair_fused_workspace_bytes(64, 64)                  # no T, no gradient partials
    assert need == 256 + 2 * 64 * (128 * 2 * 2 + 8 * 4 * 4)
    assert lib.sn_pair_match_workspace_bytes(7000, 7000) < lib.sn_pair_fused_workspace_bytes(7000, 7000) // 4
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    p = lambda x: x.data_ptr()
    SN_E_NULL, SN_E_SHAPE, SN_E_ALIGN, SN_E_WORKSPACE, SN_E_UNSUPPORTED = -1, -2, -5, -6, -7
    mf = lib.sn_pair_match_f32
    #     0     1    2     3    4   5   6   7   8    9      10     11     12     13      14  15        16      17     18    19
    ok = [p(f), 120, p(f), 120, 64, 64, 64, 64, 120, p(ci), p(ba), p(cj), p(bb), p(geo), 64, p(truth), p(err), p(ws), need, None]
    assert mf(*ok) == 0
    ch = lambda *kv: [dict(zip(kv[::2], kv[1::2])).get(j, a) for j, a in enumerate(ok)]
    assert mf(*ch(11, None, 12, None)) == 0                                      # one direction
    assert mf(*ch(13, None, 15, None, 16, None)) == 0                            # no error path
    assert mf(*ch(18, need - 1)) == SN_E_WORKSPACE
    assert mf(*ch(17, p(ws) + 4)) == SN_E_ALIGN
    assert mf(*ch(0, p(wide), 1, 200, 2, p(wide), 3, 200, 8, 129)) == SN_E_UNSUPPORTED
    assert mf(*ch(4, 65)) == SN_E_SHAPE and mf(*ch(5, 65)) == SN_E_SHAPE        # NA > rowsA, NB > rowsB
    assert mf(*ch(1, 119)) == SN_E_SHAPE                                         # lda < K
    assert mf(*ch(14, 63)) == SN_E_SHAPE                                         # ldgB < NB
    for i in (0, 2, 9, 10, 17):
        assert mf(*ch(i, None)) == SN_E_NULL, i
    assert mf(*ch(11, None)) == SN_E_NULL and mf(*ch(12, None)) == SN_E_NULL    # rowB and bestB come together
    for i in (13, 15, 16):                                                       # geoB, truthA, errA: all or none
        assert mf(*ch(i, None)) == SN_E_NULL, i
    assert mf(*ch(13, None, 15, None)) == SN_E_NULL
    torch.cuda.synchronize()


def test_no_score_sized_temporary():
    rows, n, K = 7000, 6890, 120
    from surfacenetworks_amd import _lib

    FA, FB = _features(rows, K, 77)
    need = _lib.load().sn_pair_match_workspace_bytes(rows, rows + 5)
    outputs = 2 * n * (8 + 4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = dc.match_features(FA, FB, n, n)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"pairmatch peak: {rise / 2**20:.2f} MiB (workspace {need / 2**20:.2f} MiB; a score matrix: {n * n * 4 / 2**20:.0f} MiB)")
    assert m.a2b.numel() == n
    assert rise <= need + outputs + (1 << 20)


# ---- evaluate_pair ------------------------------------------------------------------------------------------------------------
FRAME = os.path.join(os.path.dirname(__file__), "golden", "data_faust_frame.npz")


def _dataset(kind):
    if kind == "torus":
        return dc.TorusBodies(3, n=9, m=14, pad_to=160, seed=4, device=DEV), "lap"
    from surfacenetworks_amd import datasets

    tower = kind.split("_")[1]
    return datasets.faust_from_files([FRAME, FRAME, FRAME], device=DEV, model=tower, pad_to=64), tower


def _reference(model, ds, ia, ib):
    """S64 of the pair from the model in evaluation mode: the towers' features multiplied in float64."""
    inX, tX, mX, LX = ds.sample(ia)
    inY, tY, mY, LY = ds.sample(ib)
    NA, NB = tX[0][1].numel(), tY[0][1].numel()
    was = model.training
    model.eval()
    with torch.no_grad():
        FA, FB = model.towers(dc._operation(LX, mX), dc._operation(LY, mY), inX, inY)
        out = model(dc._operation(LX, mX), dc._operation(LY, mY), inX, inY)
    model.train(was)
    S64 = torch.mm(FA[0, :NA].double(), FB[0, :NB].double().t())
    # (model(...)'s own fp32 output is that product up to the library GEMM's fp32 rounding)
    assert (out[0, :NA, :NB].double() - S64).abs().max().item() <= 1e-5 * S64.abs().max().item()
    return S64, tX, tY


@pytest.mark.parametrize("kind", ["torus", "faust_lap", "faust_dir"])
def test_evaluate_pair_end_to_end(kind):
    from helpers import deterministic_init

    ds, tower = _dataset(kind)
    model = deterministic_init(dc.SiameseModel(tower, 3), 12).to(DEV).train()
    S64, tX, tY = _reference(model, ds, 0, 1)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    th = [0.0, 0.05, 0.1, 0.3, 1.0, 10.0]
    got = dc.evaluate_pair(model, ds, 0, 1, thresholds=th)
    assert all(m.training for m in model.modules())
    assert all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
    tau = TAU_REL * S64.abs().max().item()
    # (evaluate_pair returns no scores: `best` below is S64 at the predicted index, so _check_direction's |best - max| check
    # repeats its shortfall check here; the kernel's own scores are held to tau in test_random_features_against_float64)
    _check_direction(S64, got["a2b"], S64.gather(1, got["a2b"][:, None])[:, 0].float(), tau, f"{kind} a2b")
    _check_direction(S64.t(), got["b2a"], S64.t().gather(1, got["b2a"][:, None])[:, 0].float(), tau, f"{kind} b2a")
    # the derived quantities, in float64 from the matches
    GB, lA, liB = tY[0][0], tX[0][1], tY[0][2]
    truth = liB[lA]                                                               # (equal vertex counts in these datasets)
    assert torch.equal(dc.true_matches(tX, tY), truth)
    err = GB[truth, got["a2b"]]
    assert torch.equal(got["err"], err)
    e64 = err.double().cpu().numpy()
    assert abs(got["mean_error"].item() - e64.mean()) <= 1e-12 * max(e64.mean(), 1e-300)
    n = truth.numel()                                   # (shares as correctly rounded quotients of integer counts)
    assert got["exact"].item() == int((got["a2b"] == truth).sum()) / n
    want_curve = np.array([np.mean(e64 <= np.float32(t)) for t in th])
    assert np.array_equal(got["curve"].cpu().numpy(), want_curve)
    r = torch.arange(truth.numel(), device=DEV)
    assert got["mutual"].item() == int((got["b2a"][got["a2b"]] == r).sum()) / n
    print(f"pairmatch evaluate {kind}: mean error {got['mean_error'].item():.4f} exact {got['exact'].item():.3f} "
          f"mutual {got['mutual'].item():.3f}")
    # default thresholds, model left in evaluation mode
    model.eval()
    d = dc.evaluate_pair(model, ds, 0, 1)
    assert not any(m.training for m in model.modules())
    assert d["curve"].shape == (101,) and d["thresholds"].shape == (101,) and torch.equal(d["a2b"], got["a2b"])
    assert bool((d["curve"][1:] >= d["curve"][:-1]).all())


@pytest.mark.parametrize("tower", ["lap", "dir"])
def test_stored_numbering_does_not_change_the_evaluation(tower):
    """A shuffled copy of the fixture frame, stored renumbered (reorder=True) and as it comes (reorder=False): the matches in
    the file's own numbering agree outside the rows exempt under tau, the mean error within 2 x 2e-6 relative (the project's
    fused-pair value bound, once per dataset)."""
    from helpers import deterministic_init
    from surfacenetworks_amd import datasets, mesh_ops

    fr = datasets.load_faust_frame(FRAME, DEV)
    nv, nf = int(fr["V"].shape[0]), int(fr["F"].shape[0])
    rng = np.random.default_rng(5)
    frames = [dc._renumbered_frame(fr, mesh_ops.MeshOrder(rng.permutation(nv), np.arange(nf))) for _ in range(2)]
    model = deterministic_init(dc.SiameseModel(tower, 3), 12).to(DEV).eval()
    res = {}
    for reorder in (True, False):
        ds = dc.FaustFrames(frames, model=tower, pad_to=64, device=DEV, reorder=reorder)
        assert all(o.identity != reorder for o in ds.orders)
        got = dc.evaluate_pair(model, ds, 0, 1)
        res[reorder] = (dc.matches_to_dataset_order(ds, 0, 1, got["a2b"]), got["mean_error"].item(), ds)
    S64, _, _ = _reference(model, res[False][2], 0, 1)
    tau = TAU_REL * S64.abs().max().item()
    top = torch.topk(S64, 2, dim=1).values
    exempt = (top[:, 0] - top[:, 1]) < tau
    a, b = res[True][0], res[False][0]
    print(f"pairmatch numbering {tower}: exempt {int(exempt.sum())}/{nv}, differing rows {int((a != b).sum())}, "
          f"mean error {res[True][1]:.8f} / {res[False][1]:.8f}")
    assert torch.equal(a[~exempt], b[~exempt])
    assert exempt.double().mean().item() <= EXEMPT_MAX
    assert abs(res[True][1] - res[False][1]) <= 2 * 2e-6 * abs(res[False][1])
