"""Graph attention on mesh operators — the propagation rule whose weights are computed from the features, the block built on it
and the normal-prediction model of src/normal_predict/models.py:85-124 (`GatDeepModel`).

The reference names the block (`pygat.GatResNet2`) and contains no code for it, and its driver runs the model on a dense N x N
adjacency only.  The definition here is this project's own — pattern-only attention without dropout:

    e = elu(x),  H heads, slice k = channels [k C / H, (k + 1) C / H),  a (2, C): row 0 scores a row as a source, row 1 as a
    destination,  slope = 0.2
    s_src[j, k] = sum over slice k of a[0, c] e[j, c]          s_dst[i, k] likewise with a[1]
    u_ij^k      = leaky_relu(s_dst[i, k] + s_src[j, k], slope)                 for every STORED entry (i, j) of the operator
    alpha_ij^k  = exp(u_ij^k - m_i^k) / sum over row i of exp(u_il^k - m_i^k),   m_i^k = max over row i
    p[i, slice k] = sum over row i of alpha_ij^k e[j, slice k]

Only the operator's pattern is read (the pattern of a mesh Laplacian is "neighbours and self": GAT's neighbourhood with self-loops);
its values never are, and a stored explicit zero is an entry like any other.  A row without a stored entry — every padded vertex of
a padded batch — gives p = 0 and sends no gradient anywhere.  Gradients flow to x and a, nothing to the operator.

    attn_propagate(A, x2d, a, heads)             [elu(x), p] as one (rows, 2C) buffer: the attention twin of functional.lap_propagate,
                                                 one autograd node over the kernels of csrc/sn_attention.hip (launches only)
    attn_propagate_reference(A, x2d, a, heads)   the same in plain torch operations, any dtype, any device: what the tests evaluate
                                                 in float64
    GatResNet2(num_outputs, heads=8)             LapResNet2's two BatchNorm + Linear stages with the propagate swapped
    LapGatModel(in_features, out_features, layers, heads)      conv1, GatResNet2 / AvgResNet2 blocks, the padded 3-output head

Not here: attention dropout, attention biased by log |L_ij|, head widths other than C / H, a whole-block node or launch-plan site
for GatResNet2, a dense operator (dense attention is what this module replaces).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels
from . import utils_pt as utils
from .constants import ATTN_MAX_CHANNELS, ATTN_SLOPE
from .functional import _rows2d
from .normal_predict import _head_elu_conv, _NormalModel
from .operators import as_operator

__all__ = ["attn_propagate", "attn_propagate_reference", "GatResNet2", "LapGatModel", "heads_supported"]


def heads_supported(C: int, heads: int) -> bool:
    """The widths the kernels take (sn_attn_supported says the same): C % 4 == 0, C <= 256, C % heads == 0, (C / heads) % 4 == 0."""
    C, heads = int(C), int(heads)
    return 4 <= C <= ATTN_MAX_CHANNELS and C % 4 == 0 and heads >= 1 and C % heads == 0 and (C // heads) % 4 == 0


def _check(op, x2d, a, heads, who):
    if x2d.dim() != 2:
        raise ValueError(f"{who}: expected a 2-D dense operand, got {tuple(x2d.shape)}")
    rows, C = x2d.shape
    if int(heads) < 1 or C % int(heads):
        raise ValueError(f"{who}: {C} channels do not split into {heads} heads")
    if tuple(a.shape) != (2, C):
        raise ValueError(f"{who}: a must be (2, {C}), got {tuple(a.shape)}")
    if op.shape[0] != op.shape[1] or op.shape[1] != rows:
        raise ValueError(f"{who}: a square operator over the {rows} rows is required, got {tuple(op.shape)}")


def attn_propagate_reference(A, x2d: torch.Tensor, a: torch.Tensor, heads: int) -> torch.Tensor:
    """[elu(x), p] of the module docstring in plain torch operations (index_select, index_add_, a scatter maximum), in the dtype
    and on the device of x2d; differentiable in x2d and a.  A: a SparseOperator (or what as_operator takes) whose pattern is read."""
    op = as_operator(A)
    _check(op, x2d, a, heads, "attn_propagate_reference")
    R, C = x2d.shape
    H = int(heads)
    D = C // H
    dev = x2d.device
    rp, col = op.rowptr.to(dev).long(), op.colind.to(dev).long()
    row = torch.repeat_interleave(torch.arange(R, device=dev), rp[1:] - rp[:-1])
    e = F.elu(x2d)
    eh = e.reshape(R, H, D)
    s_src = (eh * a[0].reshape(1, H, D)).sum(-1)
    s_dst = (eh * a[1].reshape(1, H, D)).sum(-1)
    u = F.leaky_relu(s_dst.index_select(0, row) + s_src.index_select(0, col), ATTN_SLOPE)            # (nnz, H)
    m = torch.full((R, H), float("-inf"), dtype=u.dtype, device=dev)
    m = m.scatter_reduce(0, row.unsqueeze(1).expand(-1, H), u.detach(), "amax", include_self=True)    # (a shift: no gradient)
    w = torch.exp(u - m.index_select(0, row))
    z = torch.zeros((R, H), dtype=u.dtype, device=dev).index_add_(0, row, w)
    alpha = w / z.index_select(0, row)
    p = torch.zeros((R, H, D), dtype=u.dtype, device=dev).index_add_(0, row, alpha.unsqueeze(-1) * eh.index_select(0, col))
    return torch.cat([e, p.reshape(R, C)], 1)


def _vec_rows(t: torch.Tensor) -> torch.Tensor:
    """t with 16-byte aligned rows (what the kernels' float4 lanes need): itself where it has them, else a copy."""
    if t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) % 4):
        t = t.contiguous()
    return t


class _AttnPropagate(torch.autograd.Function):
    """cat = [e, p], e = elu(x).  Forward: sn_attn_elu_scores_f32 writes e and the scores, sn_attn_propagate_fwd_f32 writes p and
    keeps the row maxima and normalisers.  Backward: sn_attn_propagate_bwd_f32 — both halves of the incoming gradient, the ELU's
    derivative and the gradient of a from one entry point; the transposed pattern is op.t(), cached on the operator."""

    @staticmethod
    def forward(ctx, x, a, op, heads):
        x = _vec_rows(_rows2d(x))
        a = a.contiguous()
        rows, C = x.shape
        cat = torch.empty((rows, 2 * C), dtype=torch.float32, device=x.device)
        e, p = cat[:, :C], cat[:, C:]
        s = kernels.attn_elu_scores(x, a, heads, e)
        m, z = kernels.attn_propagate_fwd(op.rowptr, op.colind, op.shape[0], op.shape[1], e, s, heads, p)
        ctx.op, ctx.heads = op, heads
        ctx.save_for_backward(cat, s, m, z, a)
        return cat

    @staticmethod
    def backward(ctx, g_cat):
        cat, s, m, z, a = ctx.saved_tensors
        op = ctx.op
        g_cat = _vec_rows(_rows2d(g_cat))
        C = cat.shape[1] // 2
        t = op.t()
        dx, da = kernels.attn_propagate_bwd(op.rowptr, op.colind, t.rowptr, t.colind, op.shape[0], op.shape[1], g_cat[:, C:],
                                            g_cat[:, :C], cat[:, :C], cat[:, C:], s, m, z, a, ctx.heads)
        return dx, da, None, None


def attn_propagate(A, x2d: torch.Tensor, a: torch.Tensor, heads: int) -> torch.Tensor:
    """[elu(x2d), p] (rows, 2C) on the device: fp32, C % 4 == 0, C <= 256, (C / heads) % 4 == 0, a square operator (ValueError
    otherwise); CPU tensors are refused."""
    op = as_operator(A)
    _check(op, x2d, a, heads, "attn_propagate")
    if not heads_supported(x2d.shape[1], heads):
        raise ValueError(f"attn_propagate: C = {x2d.shape[1]} channels in {heads} heads is outside the supported set (C % 4 == 0, "
                         f"C <= {ATTN_MAX_CHANNELS}, (C / heads) % 4 == 0)")
    kernels._dev(x2d, a, op.rowptr)
    if a.dtype != torch.float32:
        raise TypeError("the Surface-Network path is fp32")
    return _AttnPropagate.apply(x2d, a, op, int(heads))


class GatResNet2(utils._TwoStage):
    """x + Lin(BN([e1, p(e1)])), e1 = elu(Lin(BN([e0, p(e0)]))), e0 = elu(x): utils_pt.LapResNet2 with attention (att0, att1: the
    (2, C) score vectors of the two stages) in place of the product with L.  Called as block(L, mask, inputs) with the sparse
    operator of the batch, whose pattern alone is read; the mask is never read."""

    def __init__(self, num_outputs, heads=8):
        super().__init__(num_outputs)
        if not heads_supported(num_outputs, heads):
            raise ValueError(f"GatResNet2: {num_outputs} channels in {heads} heads is outside the supported set (C % 4 == 0, C <= "
                             f"{ATTN_MAX_CHANNELS}, C % heads == 0, (C / heads) % 4 == 0)")
        self.heads = int(heads)
        self.att0 = nn.Parameter(torch.empty(2, num_outputs))
        self.att1 = nn.Parameter(torch.empty(2, num_outputs))
        for att in (self.att0, self.att1):
            nn.init.xavier_uniform_(att.data.view(2 * self.heads, num_outputs // self.heads), gain=1.414)

    def forward(self, L, mask, inputs):
        if isinstance(L, torch.Tensor) and L.layout == torch.strided:
            raise TypeError("GatResNet2 takes the sparse operator of the batch (a SparseOperator or a torch sparse COO tensor): "
                            "attention over a dense N x N adjacency is what this block replaces")
        batch, node, feat = inputs.size()
        op = as_operator(L)
        x2d = inputs.reshape(batch * node, feat)
        h = self.bn_fc0.forward2d(attn_propagate(op, x2d, self.att0, self.heads))
        h = self.bn_fc1.forward2d(attn_propagate(op, h, self.att1, self.heads), residual=x2d)      # "+ inputs" rides in the GEMM epilogue
        return h.view(batch, node, feat)


class LapGatModel(_NormalModel):
    """models.py:85-124 on the sparse operator: conv1 without BatchNorm, rn{i} = GatResNet2 for even i and AvgResNet2 for odd i,
    ELU, conv2 with BatchNorm in front through the padded 4-output head, the residual inputs[:, :, :3].  Called as
    model(L, mask, inputs) on the batches of NormalFrames(model="lap")."""

    def __init__(self, in_features=3, out_features=3, layers=15, heads=8):
        super().__init__()
        if in_features < 3:
            raise ValueError(f"LapGatModel adds inputs[:, :, :3] to its three outputs (models.py:122): in_features = {in_features} < 3")
        if out_features != 3:
            raise NotImplementedError(f"attention.LapGatModel: out_features={out_features} is not built on the HIP path; nothing "
                                      "approximates it")
        self.conv1 = utils.GraphConv1x1(in_features, 128, batch_norm=None)
        self.layer_num = layers
        for i in range(layers):
            self.add_module("rn{}".format(i), GatResNet2(128, heads) if i % 2 == 0 else utils.AvgResNet2(128))
        self.conv2 = utils.GraphConv1x1(128, out_features, batch_norm="pre")

    def features4(self, L, mask, inputs):
        x = self.conv1(inputs)
        for i in range(self.layer_num):
            x = self._modules["rn{}".format(i)](L, mask, x)
        return _head_elu_conv(self.conv2, x), inputs[:, :, :3]
