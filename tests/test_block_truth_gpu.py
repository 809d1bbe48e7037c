"""The whole-block autograd nodes on the MI355X, held to the float64 blocks tensor by tensor (block_truth.py: every output, input
gradient, parameter gradient and BatchNorm buffer; whole-tensor and worst-slice error against oracle/ref_blocks.py in float64; as
close as the float32 reference is, x 4).  Every product form below is the same function mathematically and is compared with
the same truth.  Reads only the repository."""
import pytest
import torch

import block_truth as bt
from block_truth import Case, Form

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _clean():
    from surfacenetworks_amd import plans

    plans.reset()
    yield
    bt.restore()


def _ids(table):
    return ["-".join(str(v) for v in case) + "-" + bt._form_text(form) for case, form, _, _ in table]


def _spy(monkeypatch):
    from surfacenetworks_amd import _lib

    names, orig = [], _lib.call

    def call(name, *a):
        names.append(name)
        return orig(name, *a)

    monkeypatch.setattr(_lib, "call", call)
    return names


def _run(case, form, monkeypatch, launched=(), not_launched=()):
    """block_truth.check + that the operators multiply in the storage form the case names and (eager forms only: a replayed
    plan does not pass through _lib.call) that the launches the form is about did / did not run; planned forms: that every block
    direction of the chain ran from its plan on all three calls."""
    from surfacenetworks_amd import functional as snF, kernels

    if not kernels._split_gemm():              # (SN_GEMM_VARIANT=0, the A/B baseline, has other launches: the values are held all the same)
        launched = not_launched = ()

    def forms(ops):
        if case.chain == "lap3":
            want = form.lap if (form.lap != "ring" or form.ring_rows is not None) else "rb4"     # (ring: from RING_MIN_ROWS rows on)
            assert snF.product_form(ops["L"], 1, case.C)[0] == want
        elif case.chain != "avg1":
            assert snF.product_form(ops["Di"], 4, case.C)[0] == form.dirac and snF.product_form(ops["DiA"].t(), 4, case.C)[0] == form.dirac

    names = _spy(monkeypatch) if (launched or not_launched) else None
    rows = bt.check(case, form, DEV, forms)
    torch.cuda.synchronize()
    if names is not None:
        assert not form.plans
        assert all(n in names for n in launched) and not any(n in names for n in not_launched), (launched, not_launched, sorted(set(names)))
    if form.plans and form.whole and kernels._split_gemm():        # a planned form did run from plans: three calls of every block
        from surfacenetworks_amd import plans

        st = plans.stats()
        half = case.C == 128 and case.train                          # (the half-width averaging node; else full width, eager)
        sites = {"dir3": ["dirac_fwd", "dirac_bwd"], "dir1": ["dirac_fwd", "dirac_bwd"], "conv": ["dirac_fwd"] + (["elu_conv_fwd", "elu_conv_bwd"] if case.C == 128 else []),     # (64 inputs: a torch GEMM inside, eager)
                
                 "lap3": ["propagate_fwd", "propagate_bwd"], "avg1": []}[case.chain]
        if half and case.chain != "dir1" and case.chain != "conv":
            sites = sites + (["avg_ragged_fwd", "avg_ragged_bwd"] if case.batch == "packed" else ["avg_fwd", "avg_bwd"])
        if not case.train:                       # (an eval-mode backward computes with torch ops inside the block: refused, eager)
            sites = [x for x in sites if x.endswith("_fwd")]
        for site in sites:
            assert st[site]["replayed"] >= 3 and st[site]["refused"] == 0, (site, st[site])
    return rows


RAW, TAIL, FINISH = "sn_linear_dgrad_elu_rawlow_f32", "sn_spmm_q3_elubwd_tail_absmax_f32", "sn_elu_tail_finish_f32"

DIRAC = [
    # the default configuration = the headline path: q3 + deferral + plans + f=None + f_out_needed=False + avg_next given
    (Case("dir3", 128, "u11"), Form(plans=True), (), ()),
    (Case("dir3", 64, "u11"), Form(plans=True), (), ()),                          # C = 64 + deferral: the N = 16 product
    # every switch flipped alone (eager ones also say which launches ran)
    (Case("dir3", 128, "u11"), Form(), (RAW, TAIL), (FINISH,)),                   # plans off
    (Case("dir3", 64, "u11"), Form(), (RAW, TAIL), (FINISH,)),
    (Case("dir3", 128, "u11"), Form(plans=True, defer=False), (), ()),
    (Case("dir3", 128, "u11"), Form(defer=False), (), (RAW, TAIL, FINISH)),
    (Case("dir3", 128, "u11", need_f=True), Form(plans=True), (), ()),
    (Case("dir3", 128, "u11", need_f=True), Form(), (), (RAW, TAIL, FINISH)),
    (Case("dir3", 128, "u11"), Form(plans=True, fnone=False), (), ()),
    (Case("dir3", 128, "u11"), Form(plans=True, avg_next="none"), (), ()),
    (Case("dir3", 128, "u11"), Form(plans=True, whole=False), (), ()),
    (Case("dir3", 128, "u11", train=False), Form(plans=True), (), ()),
    (Case("dir3", 64, "u11", train=False), Form(), (), ()),
    (Case("dir3", 64, "u11"), Form(plans=True, whole=False), (), ()),
    (Case("dir3", 64, "u11", need_f=True), Form(plans=True, defer=False), (), ()),
    # storage forms; bsr4 / csr + deferral: the finishing-kernel path
    (Case("dir3", 128, "u11"), Form(plans=True, dirac="bsr4"), (), ()),
    (Case("dir3", 128, "u11"), Form(dirac="bsr4"), (RAW, FINISH), (TAIL,)),
    (Case("dir3", 128, "u11"), Form(plans=True, dirac="csr"), (), ()),
    (Case("dir3", 64, "u11"), Form(dirac="csr"), (RAW, FINISH), (TAIL,)),
    (Case("dir3", 64, "u11"), Form(plans=True, dirac="bsr4", defer=False), (), ()),
    # tile-sum hand-offs into the averaging blocks (they exist from 32 768 rows on: forced), given and learnt
    (Case("dir3", 128, "u11"), Form(tiles=True), ("sn_linear_fwd_tiles_f32", "sn_avg_stats_from_tiles_f32"), ()),
    (Case("dir3", 128, "u11"), Form(plans=True, tiles=True), (), ()),
    (Case("dir3", 128, "u11"), Form(plans=True, tiles=True, avg_next="none"), (), ()),
    (Case("dir3", 128, "packed"), Form(tiles=True), ("sn_avg_stats_from_tiles_ragged_f32",), ()),
    (Case("dir3", 128, "packed"), Form(plans=True), (), ()),
    # (c) the gradient with respect to f, (e) elu_conv1x1 behind a block
    (Case("dir1", 128, "u11", need_f=True), Form(plans=True), (), ()),
    (Case("dir1", 64, "u11", need_f=True), Form(), (), ()),
    (Case("dir1", 128, "u11", need_f=True), Form(dirac="bsr4"), (), ()),
    (Case("dir1", 64, "u11", need_f=True), Form(plans=True, dirac="csr"), (), ()),
    (Case("dir1", 128, "u11", train=False, need_f=True), Form(plans=True), (), ()),
    (Case("dir1", 128, "u11", need_f=True), Form(whole=False), (), ()),
    (Case("conv", 128, "u11"), Form(plans=True), (), ()),
    (Case("conv", 128, "u11"), Form(), (), ()),
    (Case("conv", 64, "u11"), Form(plans=True), (), ()),
    (Case("conv", 128, "u11", train=False), Form(plans=True), (), ()),
    (Case("conv", 128, "u11"), Form(whole=False), (), ()),
]


@pytest.mark.parametrize("case,form,launched,not_launched", DIRAC, ids=_ids(DIRAC))
def test_dirac_chains_equal_the_float64_blocks(case, form, launched, not_launched, monkeypatch):
    """Chains (a) three DirResNet2 with an AvgResNet2 between each pair, (c) one DirResNet2 with a random f that requires grad,
    (e) elu_conv1x1 behind a DirResNet2; 11 meshes of 5 x 7 vertices = 385 vertex rows, 528 face rows (no multiple of the 32-row
    GEMM tile or a 64-row strip).  Covering set (DIRAC above): the default configuration at C = 128 and 64; each of launch plans,
    DEFER_FACE_TAIL, f_out_needed, f=None vs torch.zeros, avg_next given vs not said, USE_WHOLE_BLOCKS, train / eval flipped
    alone; q3 / bsr4 / csr with deferral, eager and planned; C = 64 + deferral; forced tile-sum hand-offs, given and learnt, on
    the uniform and on the packed batch.  A planned form is checked on three calls, each against its own truth."""
    from surfacenetworks_amd import kernels, plans

    _run(case, form, monkeypatch, launched, not_launched)
    if case == Case("dir3", 128, "u11") and form == Form(plans=True) and kernels._split_gemm():
        st = plans.stats()                       # (the headline's form: every block direction ran from its plan)
        assert st["dirac_bwd"]["replayed"] >= 9 and st["dirac_bwd"]["refused"] == 0, st


LAPLACIAN = [
    (Case("lap3", 128, "u11"), Form(plans=True), (), ()),                         # default: "ring" -> rb4 below 131 072 rows
    (Case("lap3", 64, "u11"), Form(plans=True), (), ()),
    (Case("lap3", 128, "u11"), Form(), ("sn_spmm_rb4_stats_f32",), ()),
    (Case("lap3", 128, "u11"), Form(plans=True, lap="csr"), (), ()),
    (Case("lap3", 64, "u11"), Form(lap="csr"), (), ("sn_spmm_rb4_f32",)),
    (Case("lap3", 128, "u11"), Form(plans=True, lap="rb4"), (), ()),
    (Case("lap3", 64, "u11"), Form(lap="rb4"), ("sn_spmm_rb4_f32",), ()),
    (Case("lap3", 128, "u11"), Form(lap="ring", ring_rows=8), ("sn_spmm_csr_ring_stats_f32",), ("sn_spmm_rb4_stats_f32",)),
    (Case("lap3", 128, "u11"), Form(plans=True, lap="ring", ring_rows=8), (), ()),
    (Case("lap3", 64, "u11"), Form(lap="ring", ring_rows=8), ("sn_spmm_csr_ring_f32",), ("sn_spmm_rb4_f32",)),
    (Case("lap3", 128, "u11"), Form(plans=True, avg_next="none"), (), ()),
    (Case("lap3", 128, "u11"), Form(tiles=True), ("sn_linear_fwd_tiles_f32", "sn_avg_stats_from_tiles_f32"), ()),
    (Case("lap3", 128, "u11"), Form(plans=True, tiles=True, avg_next="none"), (), ()),
    (Case("lap3", 128, "u11", train=False), Form(plans=True), (), ()),
    (Case("lap3", 64, "u11", train=False), Form(lap="csr"), (), ()),
    (Case("lap3", 128, "u11"), Form(plans=True, whole=False), (), ()),
]


@pytest.mark.parametrize("case,form,launched,not_launched", LAPLACIAN, ids=_ids(LAPLACIAN))
def test_laplacian_chains_equal_the_float64_blocks(case, form, launched, not_launched, monkeypatch):
    """Chain (b): three LapResNet2 with an AvgResNet2 between each pair on the 385-row batch.  C = 128 and 64; csr / rb4 / ring
    (the sliding-window kernel takes the 385-row operator once kernels.RING_MIN_ROWS is lowered, as tests/test_ring_gpu.py
    does); launch plans on and off; avg_next given, not said, and with forced tile sums; train and eval; per-stage functions."""
    _run(case, form, monkeypatch, launched, not_launched)


MERGED = "sn_avg_bn_bwd_f32"
AVERAGE = [
    (Case("avg1", 128, "u11"), Form(plans=True), (), ()),                         # uniform mask
    (Case("avg1", 128, "u11"), Form(), (MERGED,), ()),
    (Case("avg1", 128, "u11"), Form(tiles=True), ("sn_avg_stats_from_tiles_f32",), ()),
    (Case("avg1", 128, "u11"), Form(whole=False), (), ()),
    (Case("avg1", 128, "u11", train=False), Form(plans=True), (), ()),
    (Case("avg1", 64, "u11"), Form(plans=True), (), ()),                          # (full width: _PropagateBlock without an operator)
    (Case("avg1", 128, "u33"), Form(), (), (MERGED,)),                            # > AVG_BWD_MERGE_MAX meshes: three launches
    (Case("avg1", 128, "u33"), Form(plans=True), (), ()),
    (Case("avg1", 128, "ragged"), Form(plans=True), (), ()),                      # prefix mask, padding rows in the statistics
    (Case("avg1", 128, "ragged"), Form(), (), ()),
    (Case("avg1", 128, "packed"), Form(plans=True), (), ()),                      # PackedSegments in the mask's place
    (Case("avg1", 128, "packed"), Form(), (), ("sn_avg_stats_from_tiles_ragged_f32",)),
    (Case("avg1", 128, "packed"), Form(tiles=True), ("sn_avg_stats_from_tiles_ragged_f32",), ()),
    (Case("avg1", 128, "packed"), Form(plans=True, tiles=True), (), ()),
    (Case("avg1", 128, "packed", train=False), Form(), (), ()),
    (Case("avg1", 64, "packed"), Form(), (), ()),
    (Case("avg1", 128, "packed33"), Form(), ("sn_avg_bwd_segvec_ragged_f32",), (MERGED,)),   # packed, > AVG_BWD_MERGE_MAX meshes
]


@pytest.mark.parametrize("case,form,launched,not_launched", AVERAGE, ids=_ids(AVERAGE))
def test_average_blocks_equal_the_float64_blocks(case, form, launched, not_launched, monkeypatch):
    """Chain (d): one AvgResNet2.  Uniform mask (11 meshes; 33 meshes: more than kernels.AVG_BWD_MERGE_MAX, the backward's three
    separate launches), prefix mask on the padded ragged batch (5 x 7, 6 x 7 and 4 x 9 vertex grids, three of each), and the packed
    form of the same batch (PackedSegments) with and without forced tile sums — its truth is ref_blocks on the packed rows only,
    with a per-mesh mean (block_truth.PackedAvgResNet2) — and repeated to 33 meshes (the packed backward's three separate
    launches).  Plans on and off, train and eval, C = 64 (full width)."""
    from surfacenetworks_amd import kernels

    assert bt.batch("u33").meshes > kernels.AVG_BWD_MERGE_MAX >= bt.batch("u11").meshes
    assert bt.batch("packed33").meshes > kernels.AVG_BWD_MERGE_MAX >= bt.batch("packed").meshes
    _run(case, form, monkeypatch, launched, not_launched)
