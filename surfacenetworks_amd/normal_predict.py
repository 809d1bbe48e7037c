"""Vertex-normal prediction — counterpart of src/normal_predict/models.py, sampler.py:93-181 and train_4_normal.py:109-283.

`LapDeepModel` (Laplacian / global-average blocks), `DirDeepModel` (Dirac / global-average blocks) and `AvgModel` map the
`in_features` per-vertex channels of a padded batch to three outputs per vertex; the driver trains them with the squared-cosine
loss against the unit vertex normals and reports the mean angle deviation (train_4_normal.py:113-123).  `state_dict` keys and
shapes match the reference (conv1.fc.*, rn{i}.bn_fc{0,1}.*, conv2.bn.*, conv2.fc.* with conv2.fc.weight (3, 128)).

The 128 -> 3 head: the Linear kernels take output widths that are multiples of 4, so conv2 runs as a 4-output layer whose fourth
row of W and b is a zero pad made inside autograd (blocks.elu_conv(pad_to=4), functional.bn_linear_padded).  Its pitch-4 output and
the pitch-4 gradient that comes back are what the loss kernels read and write (kernels.normal_cosine_*: loss, metric and gradient
from one pass); `forward` returns the first three columns.

Not here, and refused rather than approximated: bottleneck widths, nofirstId, bnmode other than '', LapMATModel.  `GatDeepModel`
refuses under its own name: the graph-attention model lives in attention.LapGatModel (the reference's dense-adjacency `pygat` block
is not in its tree; the block there is this project's own definition on the sparse operator's pattern) and runs through
forward_loss / train_step / graphed_train_step / evaluate / predict here unchanged, on NormalFrames(model="lap") batches.
`EfficientCascade` refuses under its own name too: the reference's multiresolution model lives in
cascade.LapCascade (naive pooling, equal widths), which takes the per-level operators of a batch (`Batch.Laps`) and runs through
forward_loss / train_step / graphed_train_step here unchanged; NormalFrames(model="cas") builds each frame's mesh hierarchy
(operators.mesh_hierarchy) and samples such batches, and to_mesh_order maps their rows back to vertex ids.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import blocks as snB
from . import functional as snF
from . import kernels
from . import utils_pt as utils
from .operators import OperatorPool

__all__ = [
    "LapDeepModel", "DirDeepModel", "AvgModel", "GatDeepModel", "EfficientCascade", "LapMATModel", "repeating_expand",
    "loss_reference", "mad_reference", "cosine_loss", "mean_angle_deviation", "loss_and_mad", "Batch", "NormalFrames",
    "to_mesh_order", "forward_loss", "train_step", "graphed_train_step", "make_optimizer", "halve_lr", "evaluate", "predict",
]


# ---- loss and metric -----------------------------------------------------------------------------------------------------------
def _row_select(l, mask):
    return l.reshape(-1) if mask is None else torch.masked_select(l, mask.reshape(l.size(0), l.size(1)).bool())


def loss_reference(outputs, mask, targets):
    """loss_fun of train_4_normal.py:113-117 in plain torch operations, any dtype, any device: mean over the rows the mask selects
    of 1 - (normalize(outputs)·targets)^2.  (The reference selects with `mask.byte()`, which current torch refuses — "expected
    BoolTensor for mask"; `.bool()` selects the same rows.)  mask None: every row."""
    inner = torch.sum(F.normalize(outputs, p=2, dim=2) * targets, dim=2)
    return torch.mean(_row_select(1 - inner ** 2, mask))


def mad_reference(outputs, mask, targets):
    """mean_angle_deviation of train_4_normal.py:118-123 in plain torch operations: mean over the selected rows of
    acos(clamp(|normalize(outputs)·targets|, 0, 1))."""
    inner = torch.sum(F.normalize(outputs, p=2, dim=2) * targets, dim=2)
    return torch.mean(_row_select(torch.acos(torch.clamp(torch.abs(inner), 0, 1)), mask))


def _on_kernels(outputs, targets) -> bool:
    return outputs.is_cuda and outputs.dtype == torch.float32 and targets.dtype == torch.float32 and outputs.dim() == 3 and \
        outputs.shape[-1] == 3 and targets.shape == outputs.shape


def _rows3(t):
    """(B, V, 3) -> (rows, 3) with unit column stride: a view where the rows have one pitch (a contiguous tensor, the first three
    columns of a pitch-4 one), else a copy."""
    t2 = t.reshape(-1, 3)
    return t2 if t2.stride(1) == 1 or t2.shape[1] == 1 else t2.contiguous()


def _mask_rows(mask, rows):
    if mask is None:
        return None
    m = mask.reshape(-1)
    if m.numel() != rows:
        raise ValueError(f"mask holds {m.numel()} entries for {rows} rows")
    return m.to(torch.float32).contiguous()


class _CosineLoss(torch.autograd.Function):
    """(loss, mad) of train_4_normal.py:113-123 as one node: one pass over the rows gives both sums and, when a gradient is
    wanted, the gradient for gloss == 1 (sn_normal_cosine_fwdg_f32); the backward is one launch that returns at once unless
    gloss is something else (sn_normal_cosine_bwdg_f32).  y: (rows, 3) of pitch 3 or 4, or the contiguous (rows, 4) output of
    the padded head, whose gradient then is the pitch-4 buffer itself.  frame: (rows, 3) view added to y inside the kernels.
    want_grad: the caller's `_wants_grad(y)` (inside `forward` grad mode is off whatever the caller's is).
    The buffer the forward pass wrote is used by ONE backward: it is handed to autograd (and may be edited in place downstream, or
    rewritten here for another gloss), so a second backward of the same forward computes its gradient whole into a fresh buffer."""

    @staticmethod
    def forward(ctx, y, frame, target2d, rowmask, want_grad):
        ctx.g = None
        if want_grad:
            out, ctx.g = kernels.normal_cosine_fwdg(y, target2d, rowmask, frame, pitch=y.shape[1] if y.shape[1] == 4 else 0)
            ctx.save_for_backward(y, frame, target2d, rowmask, out)
        else:
            out = kernels.normal_cosine_fwd(y, target2d, rowmask, frame)
        loss, mad = out[0], out[1]
        ctx.mark_non_differentiable(mad)
        return loss, mad

    @staticmethod
    def backward(ctx, gloss, _gmad):
        y, frame, target2d, rowmask, out = ctx.saved_tensors
        g, ctx.g = ctx.g, None                                            # (a second backward recomputes it whole)
        g = kernels.normal_cosine_bwd(y, target2d, rowmask, frame, out, gloss.reshape(1).contiguous(), g=g,
                                      pitch=y.shape[1] if y.shape[1] == 4 else 0)
        return (g if g.shape[1] == y.shape[1] else g[:, :3]), None, None, None, None


def _wants_grad(y) -> bool:
    return bool(y.requires_grad and torch.is_grad_enabled())


def loss_and_mad(outputs, mask, targets, frame=None):
    """(loss, mad): loss_reference and mad_reference of (outputs [+ frame], mask, targets) from ONE launch; the loss carries the
    gradient, the metric none.  frame: a (B, V, 3) tensor that wants no gradient, added inside the kernel (same fp32 add as
    `outputs + frame`).  fp32 device tensors go to the kernels; anything else is computed by the two reference functions."""
    if not _on_kernels(outputs, targets):
        if outputs.is_cuda != targets.is_cuda:
            kernels._dev(outputs, targets)
        o = outputs if frame is None else outputs + frame
        with torch.no_grad():
            mad = mad_reference(o, mask, targets)
        return loss_reference(o, mask, targets), mad
    rows = outputs.shape[0] * outputs.shape[1]
    y = _rows3(outputs)                              # (the first three columns of a pitch-4 tensor stay a view: 16-byte rows)
    if y.stride(0) not in (3, 4) and y.shape[0] > 1:
        y = y.contiguous()
    f2 = None
    if frame is not None:
        f2 = _rows3(frame.detach())
    return _CosineLoss.apply(y, f2, _rows3(targets), _mask_rows(mask, rows), _wants_grad(y))


def cosine_loss(outputs, mask, targets):
    """loss_fun (train_4_normal.py:113-117) as one autograd node returning the scalar loss."""
    return loss_and_mad(outputs, mask, targets)[0]


def mean_angle_deviation(outputs, mask, targets):
    """mean_angle_deviation (train_4_normal.py:118-123), the metric as its own call (no gradient)."""
    with torch.no_grad():
        return loss_and_mad(outputs, mask, targets)[1]


# ---- models --------------------------------------------------------------------------------------------------------------------
def repeating_expand(inputs, out_features):
    """models.py:612-617: the input channels repeated (and cut) to out_features columns."""
    in_features = inputs.size(2)
    times, remin = out_features // in_features, out_features % in_features
    if times == 0:
        return inputs[:, :, :remin]
    if times == 1 and remin == 0:
        return inputs                            # (the reference's one-element torch.cat: the same values, no copy)
    return torch.cat([inputs] * times + ([inputs[:, :, :remin]] if remin else []), dim=2)


def _refuse(name, what):
    raise NotImplementedError(f"normal_predict.{name}: {what} is not built on the HIP path (see the module docstring); "
                              "nothing approximates it")


class _NormalModel(nn.Module):
    """What the three models share: the padded head, the residual frame, fuzzy_load."""

    _HEAD = 4            # output width the head runs at (the Linear kernels' granularity)

    def features4(self, op, mask, inputs):
        """(y4, frame): the head's pitch-4 output (B, V, 4) — column 3 is the pad's exact zero — and the (B, V, 3) residual
        `forward` adds to its first three columns (None: none).  forward_loss hands both to the loss kernel."""
        raise NotImplementedError

    def forward(self, op, mask, inputs, **kwargs):
        y4, frame = self.features4(op, mask, inputs)
        out = y4[:, :, :3]
        return out if frame is None else out + frame

    def fuzzy_load(self, pre_dict):
        """models.py:79-83: entries of `pre_dict` with this model's keys and shapes are loaded, the rest keep their values."""
        model_dict = self.state_dict()
        model_dict.update({k: v for k, v in pre_dict.items() if k in model_dict and model_dict[k].size() == v.size()})
        self.load_state_dict(model_dict)


def _head_elu_conv(conv, x):
    """conv(F.elu(x)) at the head's padded width: (B, V, 4)."""
    if utils.USE_WHOLE_BLOCKS and snB.elu_conv_ok(conv, x):
        return snB.elu_conv(conv, x, pad_to=_NormalModel._HEAD)
    return _head_conv(conv, F.elu(x))


def _head_conv(conv, x):
    """conv(x) at the head's padded width, no activation in front: (B, V, 4)."""
    B, V, C = x.shape
    x2d = x.reshape(B * V, C)
    bn = conv.bn
    if x2d.dtype == torch.float32 and bn.affine and bn.momentum is not None:
        return snF.bn_linear_padded(x2d, bn, conv.fc, _NormalModel._HEAD).view(B, V, _NormalModel._HEAD)
    W, b = snF.padded_linear_params(conv.fc.weight, conv.fc.bias, _NormalModel._HEAD)
    return F.linear(bn(x2d), W, b).view(B, V, _NormalModel._HEAD)


class LapDeepModel(_NormalModel):
    """models.py:39-83.  in_features other than 3 (the wks / curv4 / N / G channels of datasets.normal_frame_from_mesh; the
    reference driver's own --input-type admits V only) work too: conv1 then takes the library GEMM unless the width has a thin
    kernel (1..8 inputs), and the residual is repeating_expand(inputs, 3) as in the reference."""

    def __init__(self, in_features=3, out_features=3, layers=15, bnmode="", nofirstId=False, only_lap=False, bottleneck=False,
                 **useless):
        super().__init__()
        if bottleneck:
            _refuse("LapDeepModel", "bottleneck=True")
        if nofirstId:
            _refuse("LapDeepModel", "nofirstId=True")
        if bnmode != "":
            _refuse("LapDeepModel", f"bnmode={bnmode!r}")
        if out_features != 3:
            _refuse("LapDeepModel", f"out_features={out_features}")
        self.conv1 = utils.GraphConv1x1(in_features, 128, batch_norm=None)      # (the reference passes '', which builds no BatchNorm)
        self.layer_num = layers
        self.only_lap = bool(only_lap)
        for i in range(layers):
            lap = i % 2 == 0 or self.only_lap
            self.add_module("rn{}".format(i), utils.LapResNet2(128) if lap else utils.AvgResNet2(128))
        self.conv2 = utils.GraphConv1x1(128, out_features, batch_norm="pre")

    def features4(self, L, mask, inputs):
        x = self.conv1(inputs)
        for i in range(self.layer_num):
            blk = self._modules["rn{}".format(i)]
            if isinstance(blk, utils.LapResNet2):
                nxt = self._modules.get("rn{}".format(i + 1))
                x = blk(L, mask, x, avg_next=isinstance(nxt, utils.AvgResNet2))
            else:
                x = blk(L, mask, x)
        return _head_elu_conv(self.conv2, x), repeating_expand(inputs, 3)      # (a view of `inputs` from 3 channels up)


class DirDeepModel(_NormalModel):
    """models.py:234-280: called as model((Di, DiA), mask, inputs); conv2 WITHOUT an ELU in front, ELU after it, no residual;
    `do` declared and unused, as in the reference."""

    def __init__(self, in_features=3, out_features=3, layers=15):
        super().__init__()
        if out_features != 3:
            _refuse("DirDeepModel", f"out_features={out_features}")
        self.conv1 = utils.GraphConv1x1(in_features, 128, batch_norm=None)
        self.feature_width = 128
        self.layer_num = layers
        for i in range(layers):
            self.add_module("rn{}".format(i), utils.DirResNet2(128) if i % 2 == 0 else utils.AvgResNet2(128))
        self.do = nn.Dropout2d()
        self.conv2 = utils.GraphConv1x1(128, out_features, batch_norm="pre")

    def features4(self, DiDA, mask, inputs):
        Di, DiA = DiDA
        batch_size = inputs.size(0)
        v = self.conv1(inputs)
        num_faces = DiA.size(2) // 4 if len(Di.size()) == 3 else DiA.size(1) // 4 // batch_size      # (models.py:261)
        f = None                                # zeros(batch, faces, 128) (models.py:263), not materialised
        for i in range(self.layer_num):
            blk = self._modules["rn{}".format(i)]
            if i % 2 == 0:
                v, f = blk(Di, DiA, v, f, num_faces=num_faces, avg_next=i + 1 < self.layer_num)
            else:
                v = blk(None, mask, v)
        return F.elu(_head_conv(self.conv2, v)), None


class AvgModel(_NormalModel):
    """models.py:127-157: global-average blocks only; the residual is the input itself (inp == 3)."""

    def __init__(self, inp, out, layer):
        super().__init__()
        if out != 3:
            _refuse("AvgModel", f"out={out}")
        self.conv1 = utils.GraphConv1x1(inp, 128, batch_norm=None)
        self.layer = layer
        for i in range(layer):
            self.add_module("rn{}".format(i), utils.AvgResNet2(128))
        self.conv2 = utils.GraphConv1x1(128, out, batch_norm="pre")

    def features4(self, L, mask, inputs):
        if inputs.size(2) != 3:
            raise ValueError("AvgModel adds its input to three outputs (models.py:151): inputs must have 3 channels")
        x = self.conv1(inputs)
        for i in range(self.layer):
            x = self._modules["rn{}".format(i)](L, mask, x)
        return _head_elu_conv(self.conv2, x), inputs

    def fuzzy_load(self, pre_dict):
        """models.py:153-157: every entry of `pre_dict` with one of this model's keys is loaded."""
        model_dict = self.state_dict()
        model_dict.update({k: v for k, v in pre_dict.items() if k in model_dict})
        self.load_state_dict(model_dict)


DirDeepModel.fuzzy_load = AvgModel.fuzzy_load        # models.py:276-280 filters by key only, as AvgModel's


class GatDeepModel(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        _refuse("GatDeepModel", "the graph-attention model (models.py:85-124) under this name — attention.LapGatModel is that model "
                                "on the sparse operator's pattern, by this project's own definition of the block the reference names "
                                "and does not contain —")


class EfficientCascade(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        _refuse("EfficientCascade", "the pooling cascade (models.py:529-609) under this name — cascade.LapCascade is that model at "
                                    "naive pooling and equal widths, on a list of per-level operators —")


class LapMATModel(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        _refuse("LapMATModel", "the medial-axis model (models.py:382-410)")


# ---- sampler -------------------------------------------------------------------------------------------------------------------
@dataclass
class Batch:
    inputs: torch.Tensor      # (B, Vmax, in_features)
    targets: torch.Tensor     # (B, Vmax, 3)
    mask: torch.Tensor        # (B, Vmax, 1)
    L: Optional[object]
    Di: Optional[object]
    DiA: Optional[object]
    names: List[object]
    Laps: Optional[List[object]] = None      # cascade.LapCascade: the operators of the hierarchy's levels, coarsest first
    positions: Optional[List[torch.Tensor]] = None      # model="cas": per mesh, vertex id -> row of the node axis (to_mesh_order)

    @property
    def operator(self):
        """What the models take first: Laps where the batch carries them, else L, or (Di, DiA)."""
        if self.Laps is not None:
            return self.Laps
        return self.L if self.L is not None else (self.Di, self.DiA)

    def graph_tensors(self):
        """graphs.batch_tensors' own list — inputs, targets, mask, the arrays of L / Di / DiA — then those of every level of Laps:
        what a captured step reads and GraphedStep.load overwrites."""
        from .graphs import operator_tensors

        out = [t for t in (self.inputs, self.targets, self.mask) if t is not None]
        for op in (self.L, self.Di, self.DiA, *(self.Laps or ())):
            out.extend(operator_tensors(op))
        return out


def _as_scipy(op):
    return op.to_scipy() if hasattr(op, "to_scipy") else op


class NormalFrames:
    """The frames of datasets.normal_frame_from_mesh (the dicts of sampler.py:21-91, read_npz) as a resident dataset: inputs and
    target normals stay where they are, the operators of the requested tower go into OperatorPools; `sample_batch` pads to the
    BATCH maximum of vertices and faces and assembles the block-diagonal operators on the device (sampler.py:93-181)."""

    def __init__(self, frames, model="lap", device="cuda", levels=4, mass=None):
        """model="cas": the frames of model="lap" for cascade.LapCascade.  Each frame's hierarchy is built once from frame["L"]
        (operators.mesh_hierarchy; levels; mass None | "voronoi" | "barycentric": the restriction weights, operators.vertex_mass
        of the frame's V, F), one OperatorPool per level keeps the operators in position order, and inputs and targets are stored
        in position order with zero rows at fake nodes."""
        if model not in ("lap", "dir", "cas"):
            raise ValueError(f'NormalFrames: model must be "lap", "dir" or "cas", got {model!r}')
        if mass not in (None, "voronoi", "barycentric"):
            raise ValueError(f'NormalFrames: mass must be None, "voronoi" or "barycentric", got {mass!r}')
        kept = [fr for fr in frames if fr is not None]
        self.dropped = len(frames) - len(kept)           # frames read_npz gave up on (sampler.py:121 skips them while sampling)
        if not kept:
            raise ValueError("NormalFrames: no frame left")
        self.device = torch.device(device)
        self.kind = model
        self.frames = kept
        self.n = len(kept)
        need = ("Di", "DiA") if model == "dir" else ("L",)
        for fr in kept:
            if any(fr.get(k) is None for k in need):
                raise ValueError(f'NormalFrames(model="{model}"): a frame lacks {need} (build it with model="{"dir" if model == "dir" else "lap"}")')
        self.nv = np.array([int(fr["V"].shape[0]) for fr in kept])
        self.nf = np.array([int(fr["F"].shape[0]) for fr in kept])
        self.inputs = [torch.as_tensor(fr["input"], dtype=torch.float32).to(self.device) for fr in kept]
        self.targets = [torch.as_tensor(fr["target_dist"], dtype=torch.float32).reshape(-1, 3).to(self.device) for fr in kept]
        self.names = [fr.get("name") for fr in kept]
        self.input_features = int(self.inputs[0].shape[1])
        if model == "dir":
            self.pool_Di = OperatorPool([_as_scipy(fr["Di"]) for fr in kept], self.device, want_bsr4=True)
            self.pool_DiA = OperatorPool([_as_scipy(fr["DiA"]) for fr in kept], self.device, want_bsr4=True)
        elif model == "cas":
            self._build_hierarchies(kept, int(levels), mass)
        else:
            self.pool_L = OperatorPool([_as_scipy(fr["L"]) for fr in kept], self.device)
        self.next_id = 0             # sample_batch.train_id / test_id (sampler.py:105-114)
        self.epoch_flag = False      # sample_batch.EPOCH_FLAG: set when the walk wraps around
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _build_hierarchies(self, kept, levels, mass):
        from . import operators as snO

        if levels < 1:
            raise ValueError(f"NormalFrames: levels must be at least 1, got {levels}")
        self.levels = levels
        self.hierarchies, per_level = [], [[] for _ in range(levels)]
        for i, fr in enumerate(kept):
            L = fr["L"] if isinstance(fr["L"], snO.SparseOperator) else snO.SparseOperator.from_scipy(_as_scipy(fr["L"]), self.device)
            m = None
            if mass is not None:
                m = snO.vertex_mass(torch.as_tensor(fr["V"], dtype=torch.float32, device=self.device),
                                    torch.as_tensor(fr["F"], device=self.device), mass)
            h = snO.mesh_hierarchy(L, levels=levels, mass=m)
            self.hierarchies.append(h)
            for k in range(levels):
                per_level[k].append(h.L[k].to_scipy())
            nodes = int(h.real[-1].numel())
            for store in (self.inputs, self.targets):                      # position order, zero rows at fake nodes
                rows = torch.zeros(nodes, store[i].shape[1], device=self.device)
                rows[h.position] = store[i]
                store[i] = rows
        self.pool_Laps = [OperatorPool(mats, self.device) for mats in per_level]
        self.n0 = np.array([int(h.L[0].shape[0]) for h in self.hierarchies])

    @classmethod
    def from_meshes(cls, meshes, model="lap", device="cuda", levels=4, mass=None, **frame_kwargs):
        """From raw (V, F) pairs: datasets.normal_frame_from_mesh builds each frame first (frame_kwargs: its arguments)."""
        from .datasets import normal_frame_from_mesh

        frames = [normal_frame_from_mesh(V, F_, model="lap" if model == "cas" else model, device=device, **{"name": i, **frame_kwargs})
                  for i, (V, F_) in enumerate(meshes)]
        return cls(frames, model=model, device=device, levels=levels, mass=mass)

    def _walk(self, batch_size):
        """sampler.py:101-123 with pre-loaded frames: the next batch_size frames in order, wrapping around (the flag is raised
        when the counter passes the last frame)."""
        ids = []
        for _ in range(batch_size):
            ids.append(self.next_id)
            self.next_id += 1
            if self.next_id >= self.n:
                self.epoch_flag = True
                self.next_id = 0
        return np.asarray(ids, dtype=np.int64)

    def sample_batch(self, batch_size, rng=None, ids=None) -> Batch:
        """ids: the frames to batch; None with an rng: batch_size random ones; None without: the reference's ordered walk
        (`next_id`, `epoch_flag`).  The padded sizes are the maxima of THIS batch (sampler.py:94-95 resets them every call)."""
        if ids is None:
            ids = rng.integers(0, self.n, size=batch_size) if rng is not None else self._walk(batch_size)
        ids = np.asarray(ids, dtype=np.int64)
        B = len(ids)
        if self.kind == "cas":
            return self._sample_cascade(ids)
        nv, nf = int(self.nv[ids].max()), int(self.nf[ids].max())
        inputs = torch.zeros(B, nv, self.input_features, device=self.device)
        targets = torch.zeros(B, nv, 3, device=self.device)
        mask = torch.zeros(B, nv, 1, device=self.device)
        for b, i in enumerate(ids):
            n = int(self.nv[i])
            inputs[b, :n] = self.inputs[i]
            targets[b, :n] = self.targets[i]
            mask[b, :n] = 1
        L = Di = DiA = None
        if self.kind == "dir":
            Di = self.pool_Di.assemble(ids, 4 * nf, 4 * nv)
            DiA = self.pool_DiA.assemble(ids, 4 * nv, 4 * nf)
        else:
            L = self.pool_L.assemble(ids, nv, nv)
        return Batch(inputs, targets, mask, L, Di, DiA, [self.names[i] for i in ids])

    def _sample_cascade(self, ids) -> Batch:
        """Level k of the batch is padded to 2^k max n_0 nodes per mesh (the padding behind a mesh's own nodes, so padded siblings
        have padded parents); `mask` is the real-node mask of the finest level — not a prefix: fake nodes lie between real ones."""
        B, top = len(ids), self.levels - 1
        n0 = int(self.n0[ids].max())
        nodes = n0 << top
        inputs = torch.zeros(B, nodes, self.input_features, device=self.device)
        targets = torch.zeros(B, nodes, 3, device=self.device)
        mask = torch.zeros(B, nodes, 1, device=self.device)
        for b, i in enumerate(ids):
            own = self.inputs[i].shape[0]
            inputs[b, :own] = self.inputs[i]
            targets[b, :own] = self.targets[i]
            mask[b, :own, 0] = self.hierarchies[i].real[-1]
        Laps = [self.pool_Laps[k].assemble(ids, n0 << k, n0 << k) for k in range(self.levels)]
        return Batch(inputs, targets, mask, None, None, None, [self.names[i] for i in ids], Laps=Laps,
                     positions=[self.hierarchies[i].position for i in ids])


def to_mesh_order(batch: Batch, outputs):
    """[(nV_i, C) tensor per mesh]: the rows of `outputs` (B, nodes, C) of a model="cas" batch back in vertex order — row v of
    mesh b is outputs[b, position_b[v]]; fake and padded nodes are dropped."""
    if batch.positions is None:
        raise ValueError("to_mesh_order: the batch carries no positions (it is not a model=\"cas\" batch)")
    return [outputs[b][pos] for b, pos in enumerate(batch.positions)]


# ---- step and evaluation ---------------------------------------------------------------------------------------------------------
FUSED_TAIL = True      # forward_loss hands the head's pitch-4 output and the residual frame to the loss kernel (False: model(...) first)


def forward_loss(model, batch: Batch):
    """(loss, mad, outputs): the model on the batch, loss_fun and mean_angle_deviation (train_4_normal.py:233-238) from one
    launch.  With FUSED_TAIL the residual `+ repeating_expand(inputs, 3)` of LapDeepModel / AvgModel is the loss kernel's frame —
    the same single fp32 add per element, so loss, metric and every gradient have the bits of model(...) followed by
    cosine_loss(...) — and `outputs` is formed under no_grad for the caller only."""
    if FUSED_TAIL and isinstance(model, _NormalModel) and batch.inputs.is_cuda and batch.inputs.dtype == torch.float32:
        y4, frame = model.features4(batch.operator, batch.mask, batch.inputs)
        if y4.dtype == torch.float32 and y4.is_contiguous() and (frame is None or not (frame.requires_grad and torch.is_grad_enabled())):
            rows = y4.shape[0] * y4.shape[1]
            f2 = _rows3(frame.detach()) if frame is not None else None
            loss, mad = _CosineLoss.apply(y4.reshape(rows, 4), f2, _rows3(batch.targets), _mask_rows(batch.mask, rows), _wants_grad(y4))
            with torch.no_grad():
                outputs = y4[:, :, :3] if frame is None else y4[:, :, :3] + frame
            return loss, mad, outputs
        outputs = y4[:, :, :3] if frame is None else y4[:, :, :3] + frame
    else:
        outputs = model(batch.operator, batch.mask, batch.inputs)
    loss, mad = loss_and_mad(outputs, batch.mask, batch.targets)
    return loss, mad, outputs


def make_optimizer(model, lr=1e-3, optimizer="adam", amsgrad=False):
    """train_4_normal.py:154-159: Adam(lr[, amsgrad]) or SGD(lr, weight_decay 1e-5, momentum 0.9)."""
    params = list(model.parameters())
    if optimizer == "adam":
        fused = len(params) > 0 and all(p.is_cuda and p.dtype == torch.float32 for p in params)
        return torch.optim.Adam(params, lr=lr, amsgrad=amsgrad, fused=fused)
    if optimizer == "sgd":
        return torch.optim.SGD(params, lr=lr, weight_decay=1e-5, momentum=0.9)
    raise ValueError(f'make_optimizer: optimizer must be "adam" or "sgd", got {optimizer!r}')


def halve_lr(optimizer, epoch: int, every: int) -> bool:
    """train_4_normal.py:280-282: with --half-lr N > 0 the learning rate halves at the end of every epoch past the hundredth that
    is a multiple of N.  Returns whether it did."""
    if not (every > 0 and epoch > 100 and epoch % every == 0):
        return False
    for group in optimizer.param_groups:
        group["lr"] *= 0.5
    return True


def train_step(model, optimizer, batch: Batch, grad_sync=None):
    """train_4_normal.py:233-243.  Returns (loss, mad)."""
    loss, mad, _ = forward_loss(model, batch)
    optimizer.zero_grad(set_to_none=False)
    loss.backward()
    kernels.clear_absmax()
    if grad_sync is not None:
        grad_sync()
    optimizer.step()
    return loss, mad


def graphed_train_step(model, optimizer, example: Batch, bucket=None):
    """Training step with forward + loss + backward replayed from one hipGraph (graphs.GraphedTrainStep); batches of one
    signature only — check `.matches(batch)`."""
    from .graphs import GraphedTrainStep

    return GraphedTrainStep(model, optimizer, example, lambda m, b: forward_loss(m, b)[0], bucket)


def _eval_batches(frames: NormalFrames, batch_size: int):
    frames.next_id = 0                                   # sampler.sample_batch.test_id = 0 (train_4_normal.py:255)
    for _ in range(int(np.ceil(frames.n / batch_size))):
        yield frames.sample_batch(batch_size)


def evaluate(model, frames: NormalFrames, batch_size: int):
    """The driver's Eval loop (train_4_normal.py:251-273): ceil(n / batch_size) batches walked in order with wrap-around, the
    model as it is (the driver does not switch it to eval mode) under no_grad; {"loss", "mad"}: the means of the per-batch values,
    as device scalars."""
    loss_value, mad_value, trials = 0.0, 0.0, 0
    with torch.no_grad():
        for batch in _eval_batches(frames, batch_size):
            loss, mad, _ = forward_loss(model, batch)
            loss_value, mad_value, trials = loss_value + loss, mad_value + mad, trials + 1
    return {"loss": loss_value / trials, "mad": mad_value / trials}


def predict(model, frames: NormalFrames, batch_size: int):
    """[(name, (nV, 3) tensor)] over the same walk: the model's outputs with the padding stripped — what the driver's
    --only-forward-test writes to one CSV per mesh (train_4_normal.py:266-270, which dumps the padded rows too).  A frame the
    wrap-around visits twice appears twice, as there."""
    found = []
    with torch.no_grad():
        for batch in _eval_batches(frames, batch_size):
            outputs = model(batch.operator, batch.mask, batch.inputs)
            if batch.positions is not None:                          # model="cas": vertex order through the positions
                found.extend((name, out.clone()) for name, out in zip(batch.names, to_mesh_order(batch, outputs)))
                continue
            counts = batch.mask.reshape(batch.mask.shape[0], -1).sum(1).long().tolist()
            for name, out, n in zip(batch.names, outputs, counts):
                found.append((name, out[:n].clone()))
    return found
