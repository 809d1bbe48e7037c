"""What the normal-prediction path is held to, shared by tests/test_normal_predict.py (CPU) and the GPU files: plain-torch
restatements of the three models of src/normal_predict/models.py on the oracle's blocks (any dtype; the CPU test pins them to
the reference's classes in float64), small padded batches with explicit operators, and the float64 statement of the loss
definition of include/sn_spmm.h ("Normal prediction") with the error bounds of the kernels' expression.  Imports no GPU code."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_blocks as OB

EPS32 = 2.0 ** -24
COS_EPS = 1e-12


# ---- the three models, restated (src/normal_predict/models.py) -------------------------------------------------------------------
def repeating_expand(inputs, out_features):
    """models.py:612-617."""
    n = inputs.size(2)
    return torch.cat([inputs] * (out_features // n) + [inputs[:, :, :out_features % n]], dim=2)


class RefLapDeep(nn.Module):
    """models.py:39-77 at bnmode '' (conv1 without BatchNorm, _LapResNet2 / _AvgResNet2 at equal widths = the utils blocks,
    models.py:447-477 and 418-444; ELU, conv2 with BatchNorm "pre", + repeating_expand(inputs, 3))."""

    def __init__(self, in_features=3, out_features=3, layers=15, only_lap=False):
        super().__init__()
        self.conv1 = OB.GraphConv1x1(in_features, 128, batch_norm=None)
        self.layer_num = layers
        for i in range(layers):
            self.add_module(f"rn{i}", OB.LapResNet2(128) if (i % 2 == 0 or only_lap) else OB.AvgResNet2(128))
        self.conv2 = OB.GraphConv1x1(128, out_features, batch_norm="pre")

    def forward(self, L, mask, inputs):
        x = self.conv1(inputs)
        for i in range(self.layer_num):
            x = self._modules[f"rn{i}"](L, mask, x)
        x = self.conv2(F.elu(x))
        return x + repeating_expand(inputs, x.size(2))


class RefDirDeep(nn.Module):
    """models.py:234-274: conv2 WITHOUT an ELU in front, ELU after it, no residual; `do` declared and unused."""

    def __init__(self, in_features=3, out_features=3, layers=15):
        super().__init__()
        self.conv1 = OB.GraphConv1x1(in_features, 128, batch_norm=None)
        self.layer_num = layers
        for i in range(layers):
            self.add_module(f"rn{i}", OB.DirResNet2(128) if i % 2 == 0 else OB.AvgResNet2(128))
        self.do = nn.Dropout2d()
        self.conv2 = OB.GraphConv1x1(128, out_features, batch_norm="pre")

    def forward(self, DiDA, mask, inputs):
        Di, DiA = DiDA
        b = inputs.size(0)
        v = self.conv1(inputs)
        f = torch.zeros(b, DiA.size(-1) // 4 // b, 128, dtype=v.dtype, device=v.device)      # models.py:261-263
        for i in range(self.layer_num):
            blk = self._modules[f"rn{i}"]
            if i % 2 == 0:
                v, f = blk(Di, DiA, v, f)
            else:
                v = blk(None, mask, v)
        return F.elu(self.conv2(v))


class RefAvg(nn.Module):
    """models.py:127-151."""

    def __init__(self, inp, out, layer):
        super().__init__()
        self.conv1 = OB.GraphConv1x1(inp, 128, batch_norm=None)
        self.layer = layer
        for i in range(layer):
            self.add_module(f"rn{i}", OB.AvgResNet2(128))
        self.conv2 = OB.GraphConv1x1(128, out, batch_norm="pre")

    def forward(self, L, mask, inputs):
        x = self.conv1(inputs)
        for i in range(self.layer):
            x = self._modules[f"rn{i}"](L, mask, x)
        return self.conv2(F.elu(x)) + inputs


REF_MODELS = {"lap": lambda layers: RefLapDeep(3, 3, layers), "dir": lambda layers: RefDirDeep(3, 3, layers),
              "avg": lambda layers: RefAvg(3, 3, layers)}


# ---- the sampler's padding loop, restated literally (src/normal_predict/sampler.py:125-165) ----------------------------------------
def padded_batch(samples):
    """samples: dicts with 'V', 'F', 'input' (nV, C) and 'target_dist' (nV, 3) host tensors -> (inputs, targets, mask, nV_max,
    nF_max) as sampler.sample_batch builds them."""
    num_vertices = num_faces = 0
    for s in samples:
        num_vertices = max(num_vertices, s["V"].shape[0])
        num_faces = max(num_faces, s["F"].shape[0])
    B = len(samples)
    inputs = torch.zeros(B, num_vertices, samples[0]["input"].shape[1])
    targets = None
    mask = torch.zeros(B, num_vertices, 1)
    for b, sam in enumerate(samples):
        nv, ch = sam["input"].shape
        inputs[b, :nv, :ch] = sam["input"]
        td = sam["target_dist"]
        if targets is None:
            targets = torch.zeros(B, num_vertices, td.size(1))
        mask[b, :nv] = 1
        targets[b, :td.shape[0], :td.size(1)] = td
    return inputs, targets, mask, num_vertices, num_faces


def two_mesh_batch(kind, dtype=torch.float64, sizes=((5, 4), (6, 5)), seed=3):
    """Two cloth meshes of different sizes as one padded batch on the host: (operator(s) as block-diagonal sparse COO of `dtype`,
    mask, inputs, targets) — the host operators of mesh_ops (float32 values, as the samplers store them)."""
    from surfacenetworks_amd import mesh_ops

    rng = np.random.default_rng(seed)
    samples, mats = [], {"L": [], "Di": [], "DiA": []}
    for n, m in sizes:
        V, F_ = mesh_ops.grid_cloth(n, m, rng)
        V = V - V.min(axis=0)
        V = (V / V.max()).astype(np.float32)
        ops = mesh_ops.mesh_operators(V.astype(np.float64), F_)
        for k in mats:
            mats[k].append(ops[k].astype(np.float32))
        nrm = torch.from_numpy(np.asarray(mesh_ops.vertex_descriptors(V, F_).n_area, dtype=np.float32).reshape(-1, 3))
        samples.append({"V": V, "F": F_, "input": torch.from_numpy(V), "target_dist": nrm})
    inputs, targets, mask, nv, nf = padded_batch(samples)
    cat = lambda k, s0, s1: OB.diag_cat([OB.sp_to_coo(a.astype(np.float64)) for a in mats[k]], s0, s1).to(dtype)
    if kind == "dir":
        op = (cat("Di", 4 * nf, 4 * nv), cat("DiA", 4 * nv, 4 * nf))
    else:
        op = cat("L", nv, nv)
    return op, mask.to(dtype), inputs.to(dtype), targets.to(dtype), mats, (nv, nf)


# ---- the loss definition in float64 (include/sn_spmm.h, "Normal prediction") ----------------------------------------------------
def cos_truth(y, t, mask=None, frame=None, gloss=1.0):
    """The definition evaluated in float64 on the given (fp32) operands, row by row, rows outside S left out (never read).
    y, t, frame: (rows, 3); mask: (rows,) or None.  Returns a dict of float64 tensors / numbers:
      S (bool rows), count, o, c, l, a (rows of S; 0 elsewhere), loss, mad, g (rows, 3), and the magnitudes the bounds are built
      from, each the formula with every term replaced by its absolute value: c_scale = sum_k |u_k t_k| and, per element,
      g_scale = (|gloss| / |S|) 2 c_scale (|t| + c_scale |u|) / n."""
    yd, td = y.double(), t.double()
    rows = yd.shape[0]
    S = torch.ones(rows, dtype=torch.bool, device=y.device) if mask is None else (mask.reshape(-1) != 0)
    z = lambda: torch.zeros(rows, dtype=torch.float64, device=y.device)
    o = torch.zeros(rows, 3, dtype=torch.float64, device=y.device)
    o[S] = yd[S] + (frame.double()[S] if frame is not None else 0.0)
    tt = torch.zeros_like(o)
    tt[S] = td[S]
    nrm = o.square().sum(1).sqrt()
    n = nrm.clamp_min(COS_EPS)
    u = o / n[:, None]
    c = (u * tt).sum(1)
    l = 1 - c * c
    a = torch.acos(c.abs().clamp(max=1.0))
    count = int(S.sum())
    k = gloss / count if count else float("inf")
    g = torch.where((nrm >= COS_EPS)[:, None], tt - c[:, None] * u, tt) * ((-2.0 * c) / n)[:, None]
    g = torch.where(S[:, None], k * g, torch.zeros_like(g))
    l, a = torch.where(S, l, z()), torch.where(S, a, z())
    c_scale = (u.abs() * tt.abs()).sum(1)
    g_scale = (abs(k) if count else 0.0) * (2.0 * c_scale / n)[:, None] * (tt.abs() + (c_scale[:, None] * u.abs()))
    g_scale = torch.where(S[:, None], g_scale, torch.zeros_like(g_scale))
    nan = float("nan")
    return dict(S=S, count=count, o=o, n=n, nrm=nrm, u=u, c=c, l=l, a=a, g=g, c_scale=c_scale, g_scale=g_scale,
                loss=float(l.sum() / count) if count else nan, mad=float(a.sum() / count) if count else nan)


def analytic_gradient(outputs, mask, targets):
    """g of the definition for (B, V, 3) float64 operands at gloss = 1: what autograd of loss_reference must give."""
    B, V, _ = outputs.shape
    tr = cos_truth(outputs.reshape(-1, 3), targets.reshape(-1, 3), None if mask is None else mask.reshape(-1))
    return tr["g"].reshape(B, V, 3)


def planted_rows(rows, seed, device="cpu", frame=False):
    """(y, t, frame | None) fp32, t unit vectors; where the row count allows, planted: row 0 zero, row 1 below the 1e-12 norm, rows
    2 / 3 exactly parallel / anti-parallel to their target (axis-aligned: the products are exact), rows 4 / 5 scaled by
    2^20 / 2^-20.  With a frame, y + frame has these properties (y = value - frame would round: the frame rows are zero there)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(rows, 3, generator=g)
    t = F.normalize(torch.randn(rows, 3, generator=g), dim=1)
    fr = 0.5 * torch.randn(rows, 3, generator=g) if frame else None
    special = {0: torch.zeros(3), 1: torch.tensor([3e-13, -2e-13, 1e-13])}
    for r, v in special.items():
        if r < rows:
            y[r] = v
    if rows > 3:
        t[2] = torch.tensor([0.0, 1.0, 0.0])
        y[2] = torch.tensor([0.0, 2.5, 0.0])
        t[3] = torch.tensor([0.0, 0.0, -1.0])
        y[3] = torch.tensor([0.0, 0.0, 0.75])
    if rows > 5:
        y[4] *= 2.0 ** 20
        y[5] *= 2.0 ** -20
    if fr is not None:
        fr[:min(rows, 6)] = 0.0
    return y.to(device), t.to(device), (fr.to(device) if fr is not None else None)
