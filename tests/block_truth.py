"""Whole-block gradients held to the float64 blocks, tensor by tensor (shared by test_block_truth.py, which runs the product's
host logic on the oracle-backed kernels, and test_block_truth_gpu.py, which runs the HIP kernels).

One case = a chain of residual blocks + a batch + a width + train/eval.  The same chain runs three ways on identical bits (inputs
and loss weights drawn on the CPU from a seeded generator, parameters from helpers.deterministic_init, one seed per block):

  truth      oracle/ref_blocks.py in float64 on the CPU;
  yardstick  oracle/ref_blocks.py in float32 on the CPU — the reference's own error, e_ref;
  product    surfacenetworks_amd.utils_pt in one of its FORMS (storage form, deferral, zero faces, unwritten outputs, tile-sum
             hand-offs, launch plans, per-stage functions ...): all of them are one function mathematically.

Compared: EVERYTHING — every output, every input gradient, every parameter gradient of every module of the chain and every
running_mean / running_var / num_batches_tracked — with two metrics, both against float64:

  whole   helpers.rel_err: the largest error over the largest entry of the tensor;
  slice   the worst row, column (2-D; activations as (rows, C)) or entry (1-D) of  max|a_s - t_s| / max(max|t_s|, 0.1 max|t|):
          an error confined to a small-magnitude row, column or channel does not disappear under the tensor's maximum; the 0.1
          floor keeps exact-zero slices in the check at reduced sensitivity (nothing is skipped).

Criterion (tests/test_blocks_gpu.py::test_blocks_survive_degenerate_column_statistics: as close to float64 as the float32
reference is, x 4), without a hand-picked floor: per case and metric  bound_k = 4 * max(e_ref_k, max_j e_ref_j), the inner maximum
over the tensors of the case — it stands in for a floor, so that a tensor the reference happened to get exactly right is not held
to zero.  The chains are kept well conditioned (11 meshes and more: BatchNorm of a broadcast mean over 3 meshes is not): the
helper asserts max_j e_ref_j <= 1e-5 (whole) and <= 1e-4 (slice) for every case.

With f_out_needed=False the face output is the documented NaN placeholder and no output of the case: it is not in the list (and
not in the loss).  Eval-mode cases load running statistics that describe the data (_eval_buffers).

A planned block is called three times (recording call, second call, replay on fresh tensors of another seed); BatchNorm's
buffers evolve over the calls on both sides, so each call has its own truth.

Packed batches: the reference normalises over padding rows and the product's packed form has none, so the truth of a packed
case is ref_blocks on the packed rows only — ONE batch item of sum(V_i) rows — with the global average taken per mesh
(PackedAvgResNet2 below: ref_blocks.AvgResNet2 with masked_mean replaced by the per-mesh mean, nothing else).
"""
from __future__ import annotations

import collections

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from helpers import deterministic_init, rel_err
from oracle import ref_blocks as OB
from surfacenetworks_amd import mesh_ops

FACTOR = 4.0
COND = (1e-5, 1e-4)           # the reference alone, per case: whole tensor, slice
SEEDS = (1, 1, 2)             # recording call, second call, replay on fresh tensors of another seed
REF_THREADS = 8               # torch's fp32 CPU reductions are partitioned by the thread count (tests/test_oracle_golden.py)

Case = collections.namedtuple("Case", "chain C batch train need_f", defaults=(True, False))
# chain: "dir3"  (a) three DirResNet2, an AvgResNet2 between each pair, zero face features into the first (arap.DirModel)
#        "lap3"  (b) the same shape with LapResNet2
#        "dir1"  (c) one DirResNet2 with a random f that requires grad (need_f is True there)
#        "avg1"  (d) one AvgResNet2
#        "conv"  (e) elu_conv1x1 behind a DirResNet2, fed through the activated hand-off

_FORM_DEFAULTS = dict(dirac="q3", lap="ring", defer=True, fnone=True, avg_next="given", whole=True, plans=False, tiles=False,
                      ring_rows=None)
Form = collections.namedtuple("Form", list(_FORM_DEFAULTS), defaults=list(_FORM_DEFAULTS.values()))
# dirac / lap  functional.set_dirac_format / set_laplacian_format        defer   blocks.DEFER_FACE_TAIL
# fnone        first Dirac block f=None, num_faces=F (else torch.zeros)  whole   utils_pt.USE_WHOLE_BLOCKS
# avg_next     "given" (True where an AvgResNet2 follows) | "none"       plans   plans.set_enabled (three calls when on)
# tiles        blocks._TILE_SUMS_MIN_ROWS = 0: the tile-sum hand-offs exist at these sizes (they start at 32 768 rows)
# ring_rows    kernels.RING_MIN_ROWS lowered to this (the sliding-window kernel starts at 131 072 rows)

GRIDS = {"u11": [(5, 7)] * 11, "u33": [(5, 7)] * 33, "ragged": [(5, 7), (6, 7), (4, 9)] * 3, "packed": [(5, 7), (6, 7), (4, 9)] * 3,
         "packed33": [(5, 7), (6, 7), (4, 9)] * 11}


# ---- batches -------------------------------------------------------------------------------------------------------------------------
class Batch:
    """Block-diagonal operators (float32 scipy CSR) of the meshes grid_cloth(n, m, default_rng(k)); "packed": one batch item of
    sum(V_i) rows; else (B, max V_i) rows per item, a prefix mask and operators padded with empty rows / columns."""

    def __init__(self, name):
        self.name, self.packed = name, name.startswith("packed")
        per = []
        for k, (n, m) in enumerate(GRIDS[name]):
            V, Fc = mesh_ops.grid_cloth(n, m, np.random.default_rng(k))
            per.append((V.shape[0], Fc.shape[0], mesh_ops.mesh_operators(V, Fc)))
        self.lengths = np.array([p[0] for p in per])
        self.meshes = len(per)
        nv, nf = (None, None) if self.packed else (int(self.lengths.max()), max(p[1] for p in per))

        def diag(key, rows_of, cols_of):
            mats = []
            for v, f, ops in per:
                M = ops[key].tocsr().copy()
                if not self.packed:
                    M.resize((rows_of(nv, nf), cols_of(nv, nf)))
                mats.append(M)
            A = sp.block_diag(mats, format="csr").astype(np.float32)
            A.sort_indices()
            return A

        self.mats = {"L": diag("L", lambda v, f: v, lambda v, f: v), "Di": diag("Di", lambda v, f: 4 * f, lambda v, f: 4 * v),
                     "DiA": diag("DiA", lambda v, f: 4 * v, lambda v, f: 4 * f)}
        if self.packed:
            self.B, self.nv, self.nf = 1, int(self.lengths.sum()), sum(p[1] for p in per)
            self.mask = np.ones((1, self.nv, 1), np.float32)
        else:
            self.B, self.nv, self.nf = self.meshes, nv, nf
            self.mask = (np.arange(nv)[None, :, None] < self.lengths[:, None, None]).astype(np.float32)
        assert self.mats["L"].shape == (self.B * self.nv,) * 2 and self.mats["Di"].shape == (4 * self.B * self.nf, 4 * self.B * self.nv)


_BATCHES = {}


def batch(name) -> Batch:
    if name not in _BATCHES:
        _BATCHES[name] = Batch(name)
    return _BATCHES[name]


def inputs(case, seed):
    """v0 (masked), f0 (chain dir1 only), loss weights: float32 CPU tensors, the same bits for the product and the oracle."""
    b = batch(case.batch)
    g = torch.Generator().manual_seed(7919 * seed + case.C)
    J = out_width(case)
    v0 = torch.randn(b.B, b.nv, case.C, generator=g) * torch.from_numpy(b.mask)
    f0 = torch.randn(b.B, b.nf, case.C, generator=g)
    return dict(v0=v0, f0=f0 if case.chain == "dir1" else None, wv=torch.randn(b.B, b.nv, J, generator=g),
                wf=torch.randn(b.B, b.nf, case.C, generator=g))


def out_width(case):
    return case.C if case.chain != "conv" else (120 if case.C == 128 else case.C)     # (the models' last layer: 128 -> 120, 64 -> 64)


# ---- the chains, once: `lib` is oracle.ref_blocks or surfacenetworks_amd.utils_pt ------------------------------------------------------
class PackedAvgResNet2(OB._Res2):
    """ref_blocks.AvgResNet2 on one batch item of sum(V_i) packed rows with the global average taken per mesh."""

    def __init__(self, num_outputs, lengths):
        super().__init__(num_outputs)
        self.ids = torch.from_numpy(np.repeat(np.arange(len(lengths)), lengths))
        self.count = torch.from_numpy(np.asarray(lengths, dtype=np.float64))

    def _mean(self, x):
        s = torch.zeros(self.count.numel(), x.shape[2], dtype=x.dtype).index_add(0, self.ids, x[0])
        return (s / self.count.to(x.dtype)[:, None])[self.ids].unsqueeze(0)

    def forward(self, L, mask, inputs):
        x = F.elu(inputs)
        x = self.bn_fc0(torch.cat([x, self._mean(x)], 2))
        x = F.elu(x)
        x = self.bn_fc1(torch.cat([x, self._mean(x)], 2))
        return x + inputs


def modules(case, lib):
    """{name: module} in chain order, deterministic_init with one seed per block."""
    C, b = case.C, batch(case.batch)
    product = lib is not OB

    def avg():
        return lib.AvgResNet2(C) if (product or not b.packed) else PackedAvgResNet2(C, b.lengths)

    if case.chain in ("dir3", "lap3"):
        kind = lib.DirResNet2 if case.chain == "dir3" else lib.LapResNet2
        mods = [("blk0", kind(C)), ("avg0", avg()), ("blk1", kind(C)), ("avg1", avg()), ("blk2", kind(C))]
    elif case.chain == "dir1":
        mods = [("blk0", lib.DirResNet2(C))]
    elif case.chain == "avg1":
        mods = [("avg0", avg())]
    elif case.chain == "conv":
        mods = [("blk0", lib.DirResNet2(C)), ("conv", lib.GraphConv1x1(C, out_width(case), batch_norm="pre"))]
    else:
        raise KeyError(case.chain)
    out = collections.OrderedDict()
    for i, (name, m) in enumerate(mods):
        out[name] = deterministic_init(m, 10 + i).train(case.train)
    if not case.train:
        for name, stats in _eval_buffers(case).items():
            sd = out[name].state_dict()
            sd.update(stats)
            out[name].load_state_dict(sd)
    return out


_EVAL = {}


def _eval_buffers(case):
    """Running statistics for an eval-mode case: those of the data, as after training — the batch statistics of one float64
    train-mode call of the oracle on the inputs of seed 0 (momentum 1), rounded to float32 for everyone.  With the arbitrary
    statistics of deterministic_init nothing normalises: the features grow block by block and the float32 reference itself is
    off by 7e-5 .. 2e-4 in a weight gradient of the three-block chains (measured), which breaks the conditioning this module asserts."""
    if case not in _EVAL:
        tc, b = case._replace(train=True), batch(case.batch)
        mods = {k: m.double() for k, m in modules(tc, OB).items()}
        for m in mods.values():
            for s in m.modules():
                if isinstance(s, torch.nn.BatchNorm1d):
                    s.momentum = 1.0
        n = torch.get_num_threads()
        torch.set_num_threads(REF_THREADS)
        try:
            step(tc, mods, cpu_ops(b, torch.float64), torch.from_numpy(b.mask).double(), 0, torch.float64)
        finally:
            torch.set_num_threads(n)
        _EVAL[case] = {k: {n_: t.float().clone() for n_, t in m.state_dict().items() if "running" in n_} for k, m in mods.items()}
    return _EVAL[case]


def forward(case, mods, ops, mask, v0, f0, form=None, lib=OB):
    """The chain -> {output name: tensor}.  form=None: the oracle's signatures; else the product's, with the form's arguments."""
    b = batch(case.batch)
    product = form is not None
    v = v0

    def dirac(blk, v, f, follows_avg):
        if not product:
            f = torch.zeros(b.B, b.nf, case.C, dtype=v.dtype) if f is None else f
            return blk(ops["Di"], ops["DiA"], v, f)
        if f is None and not form.fnone:
            f = torch.zeros(b.B, b.nf, case.C, dtype=v.dtype, device=v.device)
        return blk(ops["Di"], ops["DiA"], v, f, f_out_needed=case.need_f, num_faces=b.nf,
                   avg_next=follows_avg if form.avg_next == "given" else None)

    if case.chain in ("dir3", "lap3"):
        f = None
        for i in range(3):
            if case.chain == "dir3":
                v, f = dirac(mods[f"blk{i}"], v, f, i < 2)
            elif product:
                v = mods[f"blk{i}"](ops["L"], mask, v, avg_next=(i < 2) if form.avg_next == "given" else None)
            else:
                v = mods[f"blk{i}"](ops["L"], mask, v)
            if i < 2:
                v = mods[f"avg{i}"](None, mask, v)
        return {"out.v": v, "out.f": f} if (case.chain == "dir3" and case.need_f) else {"out.v": v}
    if case.chain == "dir1":
        v, f = dirac(mods["blk0"], v, f0, False)
        return {"out.v": v, "out.f": f}
    if case.chain == "avg1":
        return {"out.v": mods["avg0"](None, mask, v)}
    v, _ = dirac(mods["blk0"], v, None, False)
    return {"out.v": lib.elu_conv1x1(mods["conv"], v) if product else mods["conv"](F.elu(v))}


def _f64(t):
    return None if t is None else t.detach().double().cpu().numpy().copy()     # (a float64 CPU buffer would be a live view)


def step(case, mods, ops, mask, seed, dtype=torch.float32, dev="cpu", form=None, lib=OB):
    """One forward + backward on fresh tensors of `seed` -> {tensor name: float64 array | None}: the outputs, the input
    gradients, every parameter gradient and every buffer of every module."""
    for m in mods.values():
        m.zero_grad(set_to_none=True)
    t = {k: (None if x is None else x.to(dtype).to(dev)) for k, x in inputs(case, seed).items()}
    v0 = t["v0"].requires_grad_(True)
    f0 = t["f0"].requires_grad_(True) if t["f0"] is not None else None
    outs = forward(case, mods, ops, mask, v0, f0, form, lib)
    loss = (outs["out.v"] * t["wv"]).sum()
    if "out.f" in outs:
        loss = loss + (outs["out.f"] * t["wf"]).sum()
    loss.backward()
    if form is not None:
        from surfacenetworks_amd import kernels

        kernels.clear_absmax()
    res = {k: _f64(o) for k, o in outs.items()}
    res["grad.v0"] = _f64(v0.grad)
    if f0 is not None:
        res["grad.f0"] = _f64(f0.grad)
    for name, m in mods.items():
        for k, p in m.named_parameters():
            res[f"{name}.{k}.grad"] = _f64(p.grad)
        for k, buf in m.named_buffers():
            res[f"{name}.{k}"] = _f64(buf)
    return res


# ---- metrics -------------------------------------------------------------------------------------------------------------------------
def slice_err(a, t):
    """Worst row / column (entry, for a 1-D tensor) of max|a_s - t_s| / max(max|t_s|, 0.1 max|t|).  No slice is left out."""
    a, t = np.asarray(a, np.float64), np.asarray(t, np.float64)
    if t.ndim == 0:
        a, t = a.reshape(1), t.reshape(1)
    d, m = np.abs(a - t), np.abs(t)
    top = max(float(m.max()), 1e-30)
    if t.ndim == 1:
        return float((d / np.maximum(m, 0.1 * top)).max())
    d, m = d.reshape(-1, t.shape[-1]), m.reshape(-1, t.shape[-1])
    return max(float((d.max(ax) / np.maximum(m.max(ax), 0.1 * top)).max()) for ax in (0, 1))


METRICS = (("whole", rel_err), ("slice", slice_err))


# ---- truth and yardstick, cached per case --------------------------------------------------------------------------------------------
_TRUTH = {}


def cpu_ops(b, dtype):
    return {k: OB.sp_to_coo(M.astype(np.float64 if dtype == torch.float64 else np.float32)).coalesce() for k, M in b.mats.items()}


def truth(case):
    """[(t64, e_ref)] per call of SEEDS: the float64 results and, per tensor, the float32 reference's (whole, slice) error;
    asserts the case's conditioning."""
    if case not in _TRUTH:
        b = batch(case.batch)
        n = torch.get_num_threads()
        torch.set_num_threads(REF_THREADS)
        try:
            runs = {}
            for dtype in (torch.float64, torch.float32):
                mods = {k: m.to(dtype) for k, m in modules(case, OB).items()}
                ops, mask = cpu_ops(b, dtype), torch.from_numpy(b.mask).to(dtype)
                runs[dtype] = [step(case, mods, ops, mask, s, dtype) for s in SEEDS]
        finally:
            torch.set_num_threads(n)
        calls = []
        for t64, r32 in zip(runs[torch.float64], runs[torch.float32]):
            assert all(x is not None and np.isfinite(x).all() for x in t64.values()), case
            e_ref = {k: tuple(float(fn(r32[k], t64[k])) for _, fn in METRICS) for k in t64}
            for i, (mname, _) in enumerate(METRICS):
                worst = max(e_ref, key=lambda k: e_ref[k][i])
                assert e_ref[worst][i] <= COND[i], ("ill-conditioned case: change its inputs, not the bound", case, mname, worst,
                                                    e_ref[worst][i])
            calls.append((t64, e_ref))
        _TRUTH[case] = calls
    return _TRUTH[case]


# ---- the product's switches ----------------------------------------------------------------------------------------------------------
def _switch_modules():
    import surfacenetworks_amd.utils_pt as U
    from surfacenetworks_amd import blocks, kernels, plans

    return U, blocks, kernels, plans


_ORIGINAL = {}


def _remember():
    if not _ORIGINAL:
        U, blocks, kernels, plans = _switch_modules()
        _ORIGINAL.update(tiles=blocks._TILE_SUMS_MIN_ROWS, ring=kernels.RING_MIN_ROWS, plans=plans._ENABLED)


def apply(form):
    from surfacenetworks_amd import functional as snF

    U, blocks, kernels, plans = _switch_modules()
    _remember()
    snF.set_dirac_format(form.dirac)
    snF.set_laplacian_format(form.lap)
    blocks.DEFER_FACE_TAIL = form.defer
    blocks._TILE_SUMS_MIN_ROWS = 0 if form.tiles else _ORIGINAL["tiles"]
    kernels.RING_MIN_ROWS = form.ring_rows if form.ring_rows is not None else _ORIGINAL["ring"]
    U.USE_WHOLE_BLOCKS = form.whole
    plans.set_enabled(form.plans)


def restore():
    """Every switch back to the process default (the test files call it in a fixture's teardown)."""
    from surfacenetworks_amd import functional as snF

    U, blocks, kernels, plans = _switch_modules()
    _remember()
    snF.set_dirac_format("q3")
    snF.set_laplacian_format("ring")
    blocks.DEFER_FACE_TAIL = True
    blocks._TILE_SUMS_MIN_ROWS = _ORIGINAL["tiles"]
    kernels.RING_MIN_ROWS = _ORIGINAL["ring"]
    U.USE_WHOLE_BLOCKS = True
    plans.set_enabled(_ORIGINAL["plans"])
    kernels.clear_absmax()


def product_ops(case, dev):
    """(operators, mask) of the case's batch on `dev`, made after the form's switches are set."""
    from surfacenetworks_amd.operators import PackedSegments, SparseOperator

    b = batch(case.batch)
    ops = {k: SparseOperator.from_scipy(M, dev) for k, M in b.mats.items()}
    mask = PackedSegments(b.lengths, dev) if b.packed else torch.from_numpy(b.mask).to(dev)
    return ops, mask


# ---- the check -----------------------------------------------------------------------------------------------------------------------
def check(case, form, dev, on_ops=None):
    """The product in `form` against the truth of `case`: every tensor, both metrics, on every call (three when planned).
    on_ops(ops): called once the operators exist (a test asserts there which storage form they multiply in).
    Prints the worst tensor per call and metric; returns [(call, tensor, metric, e_prod, e_ref, bound)]."""
    import surfacenetworks_amd.utils_pt as U

    calls = truth(case)
    apply(form)
    ops, mask = product_ops(case, dev)
    if on_ops is not None:
        on_ops(ops)
    mods = {k: m.to(dev) for k, m in modules(case, U).items()}
    rows, bad = [], []
    for call in range(3 if form.plans else 1):
        got = step(case, mods, ops, mask, SEEDS[call], torch.float32, dev, form, U)
        t64, e_ref = calls[call]
        assert set(got) == set(t64), (sorted(set(got) ^ set(t64)))
        floor = [max(e[i] for e in e_ref.values()) for i in range(len(METRICS))]
        first = len(rows)
        for name, t in t64.items():                      # the one comparison loop: every tensor of the case, both metrics
            a = got[name]
            if a is None or a.shape != t.shape or not np.isfinite(a).all():
                bad.append((call, name, "missing" if a is None else "shape" if a.shape != t.shape else "not finite"))
                continue
            for i, (mname, fn) in enumerate(METRICS):
                e = float(fn(a, t))
                bound = FACTOR * max(e_ref[name][i], floor[i])
                rows.append((call, name, mname, e, e_ref[name][i], bound))
                if not e <= bound:
                    bad.append((call, name, mname, "product", e, "reference fp32", e_ref[name][i], "bound", bound))
        for i, (mname, _) in enumerate(METRICS):
            mine = [r for r in rows[first:] if r[2] == mname]
            if mine:
                w = max(mine, key=lambda r: r[3] / r[5])
                print(f"blocktruth | {'/'.join(str(x) for x in case)} | {_form_text(form)} | call {call} | {mname} | {w[1]} | "
                      f"e_prod {w[3]:.3g} | e_ref {w[4]:.3g} | e_ref_max {floor[i]:.3g} | ratio {FACTOR * w[3] / w[5]:.3f}")
    assert not bad, (case, form, bad[:12], len(bad))
    return rows


def _form_text(form):
    diff = [f"{k}={getattr(form, k)}" for k in Form._fields if getattr(form, k) != _FORM_DEFAULTS[k]]
    return ",".join(diff) if diff else "default"
