"""What the cascade model is held to, shared by tests/test_cascade.py (CPU) and tests/test_cascade_gpu.py: a plain-torch
restatement of `EfficientCascade` (src/normal_predict/models.py:529-609) on the oracle's blocks (any dtype; the CPU test pins it
to the reference's own class in float64), torch's own forms of the two pooling operations, and small batches of two meshes of
different size with one operator per level.  Imports no GPU code.

The levels here come from the simplest hierarchy with the numbering the model needs (nodes 2 j and 2 j + 1 of level k are the
children of node j of level k - 1): a mesh's vertices in their own order with fake nodes (empty rows and columns) strewn
between them up to a multiple of 2^(levels-1) — so the real-node mask is no prefix —, and every coarser operator the
aggregation L_{k-1} = 1/2 P^T L_k P over consecutive pairs.  The model's arithmetic does not depend on which hierarchy
supplies the operators."""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

import normal_cases as nc
from oracle import ref_blocks as OB


# ---- the pooling operations as the reference writes them (models.py:568-576, 597) ------------------------------------------------
def torch_pool(x):
    return torch.nn.MaxPool1d(2, stride=2)(x.transpose(1, 2)).transpose(1, 2)


def torch_unpool_add(x, skip):
    x = F.interpolate(x.transpose(1, 2), scale_factor=2).transpose(1, 2)
    x += skip[:, :, :x.size(2)]
    return x


# ---- the model, restated ------------------------------------------------------------------------------------------------------------
class RefCascade(nn.Module):
    """models.py:529-609 at naive_pool=True, bottleneck=False, inner_layers=2, bnmode '': _LapResNet2 at equal widths is the
    utils block (models.py:447-477), whose mask is never read; the pooling modules hold no parameter, so the state_dict is
    conv1, down_rn{levels-1..1}, lap0, up_rn{1..levels-1}, conv2."""

    def __init__(self, in_features=3, out_features=3, cascade_levels=4):
        super().__init__()
        self.conv1 = OB.GraphConv1x1(in_features, 128, batch_norm=None)
        self.cascade_num = cascade_levels
        for i in range(cascade_levels - 1, 0, -1):
            self.add_module(f"down_rn{i}", OB.LapResNet2(128))
        self.lap0 = OB.LapResNet2(128)
        for i in range(1, cascade_levels):
            self.add_module(f"up_rn{i}", OB.LapResNet2(128))
        self.conv2 = OB.GraphConv1x1(128, out_features, batch_norm="pre")

    def forward(self, Laps, mask, inputs):
        x = self.conv1(inputs)
        down_series = []
        for i in range(self.cascade_num - 1, 0, -1):
            down_series.append(x)
            x = self._modules[f"down_rn{i}"](Laps[i], None, x)
            x = torch_pool(x)
        x = self.lap0(Laps[0], None, x)
        for i in range(1, self.cascade_num):
            x = torch_unpool_add(x, down_series[-i])
            x = self._modules[f"up_rn{i}"](Laps[i], None, x)
        x = self.conv2(F.elu(x))
        return x + nc.repeating_expand(inputs, x.size(2))


# ---- operators per level -----------------------------------------------------------------------------------------------------------
def pair_levels(L, levels, nodes, position=None):
    """[L_0 .. L_{levels-1}], coarsest first, fp32 scipy CSR: L padded with empty rows and columns to `nodes` (a multiple of
    2^(levels-1)) is the finest — vertex i at node position[i] (ascending; None: i), the other nodes fake —; L_{k-1} =
    1/2 P^T L_k P with P the 0/1 matrix that joins nodes 2 j and 2 j + 1."""
    assert nodes % (1 << (levels - 1)) == 0 and nodes >= L.shape[0]
    L = sp.csr_matrix(L, dtype=np.float64)
    if position is not None:
        S = sp.csr_matrix((np.ones(L.shape[0]), (position, np.arange(L.shape[0]))), shape=(nodes, L.shape[0]))
        L = (S @ L @ S.T).tocsr()
    L.resize((nodes, nodes))
    out = [L]
    for _ in range(levels - 1):
        n = out[0].shape[0]
        P = sp.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 2)), shape=(n, n // 2))
        out.insert(0, (0.5 * (P.T @ out[0] @ P)).tocsr())
    res = []
    for M in out:
        M = M.astype(np.float32).tocsr()
        M.eliminate_zeros()
        M.sort_indices()
        res.append(M)
    return res


def cascade_batch(levels, sizes=((9, 8), (10, 9)), seed=3, scatter=True):
    """Two cloth meshes of different size as one padded batch on the host.  Returns a dict: Laps (scipy CSR per level, the
    block-diagonal operator of the batch, coarsest first), per_mesh (the same per mesh), inputs (B, V, 3), targets (B, V, 3),
    mask (B, V, 1) fp32 tensors, nv (vertices per mesh), position (node of every vertex, per mesh) and V (the padded node count
    of the finest level).  scatter: the fake nodes lie BETWEEN the real ones, at seeded places, as a matching with singletons
    leaves them — so the mask is no prefix of the node axis; False: all at the end."""
    from surfacenetworks_amd import mesh_ops

    rng = np.random.default_rng(seed)
    samples, Ls = [], []
    for n, m in sizes:
        V, F_ = mesh_ops.grid_cloth(n, m, rng)
        V = V - V.min(axis=0)
        V = (V / V.max()).astype(np.float32)
        Ls.append(mesh_ops.mesh_operators(V.astype(np.float64), F_)["L"].astype(np.float32))
        nrm = torch.from_numpy(np.asarray(mesh_ops.vertex_descriptors(V, F_).n_area, dtype=np.float32).reshape(-1, 3))
        samples.append({"V": V, "F": F_, "input": torch.from_numpy(V), "target_dist": nrm})
    step = 1 << (levels - 1)
    nv = [s["V"].shape[0] for s in samples]
    Vp = -(-max(nv) // step) * step
    B = len(samples)
    inputs, targets, mask = torch.zeros(B, Vp, 3), torch.zeros(B, Vp, 3), torch.zeros(B, Vp, 1)
    position = [np.sort(rng.choice(Vp, n, replace=False)) if scatter else np.arange(n) for n in nv]
    for b, s in enumerate(samples):
        at = torch.from_numpy(position[b])
        inputs[b, at], targets[b, at], mask[b, at] = s["input"], s["target_dist"], 1
    per_mesh = [pair_levels(L, levels, Vp, pos) for L, pos in zip(Ls, position)]
    Laps = [sp.block_diag([pm[k] for pm in per_mesh], format="csr").astype(np.float32) for k in range(levels)]
    for M in Laps:
        M.sort_indices()
    return dict(Laps=Laps, per_mesh=per_mesh, inputs=inputs, targets=targets, mask=mask, nv=nv, position=position, V=Vp)


def host_operators(case, dtype, dense=False):
    """The Laps of a case for a host model: block-diagonal sparse COO of `dtype`, or dense (B, V_k, V_k) tensors."""
    if dense:
        return [torch.stack([torch.from_numpy(pm[k].toarray().astype(np.float64)) for pm in case["per_mesh"]]).to(dtype)
                for k in range(len(case["Laps"]))]
    return [OB.sp_to_coo(M.astype(np.float64)).coalesce().to(dtype) for M in case["Laps"]]
