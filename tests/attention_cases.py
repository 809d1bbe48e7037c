"""What the graph-attention path is held to, shared by tests/test_attention.py (CPU) and tests/test_attention_gpu.py: the seeded
patterns and operands, an independent dense statement of the definition (surfacenetworks_amd/attention.py's docstring), the
float64 / fp32 evaluations of attention.attn_propagate_reference that the device results are compared with, and plain-torch
restatements of the block and the model on the oracle's layers.  Imports no GPU code; nothing here runs a kernel."""
import functools

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_blocks as OB

WIDTHS = ((16, 1), (16, 4), (128, 1), (128, 8), (128, 32))        # (C, H)
CLOTHS = ((6, 5), (12, 9), (9, 7))                                # the padded three-cloth batch
FAN_SPOKES = 70
SLOPE = 0.2


# ---- patterns ------------------------------------------------------------------------------------------------------------------
def cloth_laplacian(n=12, m=9, seed=0):
    from surfacenetworks_amd import mesh_ops

    V, F_ = mesh_ops.grid_cloth(n, m, np.random.default_rng(seed))
    return mesh_ops.mesh_operators(V, F_)["L"].tocsr()


def fan_pattern(spokes=FAN_SPOKES):
    """A hub (vertex 0) with `spokes` neighbours on a closed rim, self-loops included: row 0 holds spokes + 1 entries — longer than
    a wave's batch of entries and longer than 64 — every other row four."""
    n = spokes + 1
    rim = np.arange(1, n)
    nxt = np.roll(rim, -1)
    i = np.concatenate([np.zeros(spokes, int), rim, rim, nxt, np.arange(n)])
    j = np.concatenate([rim, np.zeros(spokes, int), nxt, rim, np.arange(n)])
    M = sp.coo_matrix((np.ones(i.size, np.float32), (i, j)), shape=(n, n)).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    assert M[0].nnz == spokes + 1 > 64
    return M


def random_pattern(n=53, seed=11):
    """A seeded non-symmetric square pattern with rows of exactly one entry (3, 20), empty rows (7, 31), a column no row references
    (7, 40): index 7 takes part in nothing, 31 is only read, 40 only reads."""
    rng = np.random.default_rng(seed)
    dense = rng.random((n, n)) < 0.12
    dense[[7, 31], :] = False
    dense[:, [7, 40]] = False
    dense[3, :] = False
    dense[3, 5] = True
    dense[20, :] = False
    dense[20, 20] = True
    dense[40, 2] = True
    M = sp.csr_matrix(dense.astype(np.float32))
    M.sort_indices()
    cnt = np.diff(M.indptr)
    assert cnt[3] == cnt[20] == 1 and cnt[7] == cnt[31] == 0 and not dense[:, 7].any() and not dense[:, 40].any()
    assert (dense != dense.T).any()
    return M


def host_operator(M):
    """A SparseOperator on the host over the pattern of the scipy matrix M (what attn_propagate_reference reads)."""
    from surfacenetworks_amd.operators import SparseOperator

    M = M.tocsr()
    return SparseOperator(torch.from_numpy(M.indptr.astype(np.int32)), torch.from_numpy(M.indices.astype(np.int32)),
                          torch.from_numpy(M.data.astype(np.float32)), tuple(M.shape))


def idle_rows(M):
    """Rows that take part in nothing: no stored entry in the row and none in the column."""
    M = M.tocsr()
    used = np.zeros(M.shape[0], bool)
    used[np.diff(M.indptr) > 0] = True
    used[M.indices] = True
    return np.flatnonzero(~used)


# ---- operands --------------------------------------------------------------------------------------------------------------------
def operands(rows, C, seed):
    """(x, a, g): seeded fp32 features, score vectors and an upstream gradient on both halves of the (rows, 2C) output."""
    gen = torch.Generator().manual_seed(1000 * seed + C)
    x = torch.randn(rows, C, generator=gen)
    a = 0.3 * torch.randn(2, C, generator=gen)
    g = torch.randn(rows, 2 * C, generator=gen)
    return x, a, g


def scale_for_large_scores(x, a, heads, reach=100.0):
    """a scaled so that the largest |s| is `reach`: far past where an unshifted exp overflows fp32 (88.7)."""
    R, C = x.shape
    eh = F.elu(x.double()).reshape(R, heads, C // heads)
    s = torch.stack([(eh * a[k].double().reshape(1, heads, -1)).sum(-1) for k in (0, 1)])
    return a * float(reach / s.abs().max())


def evaluate(op, x, a, g, heads, dtype):
    """(cat, dx, da) of attn_propagate_reference in `dtype` on the host."""
    from surfacenetworks_amd import attention

    xd = x.detach().to(dtype).clone().requires_grad_(True)          # (a copy: .to() of an fp32 tensor to fp32 is the tensor itself)
    ad = a.detach().to(dtype).clone().requires_grad_(True)
    cat = attention.attn_propagate_reference(op, xd, ad, heads)
    cat.backward(g.to(dtype))
    return cat.detach(), xd.grad, ad.grad


def bound(cpu32, f64):
    """4 max(max |cpu32 - f64|, 2^-23 max |f64|): four times the reference's own fp32 error, floored at one ulp of the tensor's
    largest entry (the floor keeps the bound from collapsing where the fp32 evaluation happens to be exact)."""
    return 4.0 * max(float((cpu32.double() - f64).abs().max()), 2.0 ** -23 * float(f64.abs().max()))


def ratio(dev, cpu32, f64):
    """max |dev - f64| over the bound: held when <= 1."""
    return float((dev.detach().double().cpu() - f64).abs().max()) / max(bound(cpu32, f64), 1e-300)


@functools.lru_cache(maxsize=None)
def host_case(pattern, C, heads, large):
    """The operands of a (pattern, C, heads) case and their float64 and fp32 evaluations on the host, computed once.  pattern:
    "cloth" | "fan" | "random" (the three-cloth batch is assembled on the device: the GPU file passes its pattern to `reference`)."""
    M = {"cloth": cloth_laplacian, "fan": fan_pattern, "random": random_pattern}[pattern]()
    return reference(M, C, heads, large, seed={"cloth": 1, "fan": 2, "random": 3}[pattern])


def reference(M, C, heads, large, seed):
    op = host_operator(M)
    x, a, g = operands(M.shape[0], C, seed)
    if large:
        a = scale_for_large_scores(x, a, heads)
    return {"M": M, "x": x, "a": a, "g": g, "f64": evaluate(op, x, a, g, heads, torch.float64),
            "f32": evaluate(op, x, a, g, heads, torch.float32)}


# ---- the independent dense statement ------------------------------------------------------------------------------------------------
def dense_statement(M, x, a, heads):
    """[elu(x), p] through a masked N x N logits matrix with -inf off the pattern, softmax(dim=1) and a matmul per head; a row
    without entries is zero-filled.  Shares no code with attention.attn_propagate_reference."""
    M = M.tocsr()
    N, C = x.shape
    D = C // heads
    mask = torch.zeros(N, N, dtype=torch.bool)
    rows = np.repeat(np.arange(N), np.diff(M.indptr))
    mask[torch.from_numpy(rows), torch.from_numpy(M.indices.astype(np.int64))] = True
    e = torch.where(x > 0, x, torch.expm1(x))
    out = []
    for k in range(heads):
        ek = e[:, k * D:(k + 1) * D]
        src = ek @ a[0, k * D:(k + 1) * D]
        dst = ek @ a[1, k * D:(k + 1) * D]
        pre = dst[:, None] + src[None, :]
        logits = torch.where(pre > 0, pre, SLOPE * pre)
        logits = torch.where(mask, logits, torch.full_like(logits, float("-inf")))
        alpha = torch.softmax(logits, dim=1)
        alpha = torch.where(mask.any(1, keepdim=True), alpha, torch.zeros_like(alpha))
        out.append(alpha @ ek)
    return torch.cat([e] + out, 1)


# ---- the block and the model, restated on the oracle's layers -----------------------------------------------------------------------
class RefGatResNet2(OB._Res2):
    """attention.GatResNet2 in plain torch: the oracle's two BatchNorm + Linear stages around attn_propagate_reference."""

    def __init__(self, num_outputs, heads=8):
        super().__init__(num_outputs)
        self.heads = heads
        self.att0 = nn.Parameter(torch.zeros(2, num_outputs))
        self.att1 = nn.Parameter(torch.zeros(2, num_outputs))

    def _stage(self, L, x, att):
        from surfacenetworks_amd import attention

        b, n, c = x.size()
        return attention.attn_propagate_reference(L, x.reshape(b * n, c), att, self.heads).view(b, n, 2 * c)

    def forward(self, L, mask, inputs):
        x = self.bn_fc0(self._stage(L, inputs, self.att0))
        x = self.bn_fc1(self._stage(L, x, self.att1))
        return x + inputs


class RefLapGat(nn.Module):
    """attention.LapGatModel in plain torch (the layout of src/normal_predict/models.py:85-124)."""

    def __init__(self, in_features=3, out_features=3, layers=15, heads=8):
        super().__init__()
        self.conv1 = OB.GraphConv1x1(in_features, 128, batch_norm=None)
        self.layer_num = layers
        for i in range(layers):
            self.add_module(f"rn{i}", RefGatResNet2(128, heads) if i % 2 == 0 else OB.AvgResNet2(128))
        self.conv2 = OB.GraphConv1x1(128, out_features, batch_norm="pre")

    def forward(self, L, mask, inputs):
        x = self.conv1(inputs)
        for i in range(self.layer_num):
            x = self._modules[f"rn{i}"](L, mask, x)
        return self.conv2(F.elu(x)) + inputs[:, :, :3]
