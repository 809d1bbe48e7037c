"""The multiresolution model of normal prediction — counterpart of `EfficientCascade`, src/normal_predict/models.py:529-609, at
the options the reference's own blocks allow (naive pooling, equal widths, two inner layers, bnmode '').

    down path   per level i = levels-1 .. 1: a Laplacian residual block on Laps[i], then the maximum over sibling pairs of nodes
    coarsest    one block on Laps[0]
    up path     per level i = 1 .. levels-1: every node repeated twice plus the skip from the down path, then a block on Laps[i]

`Laps[k]` is the operator of level k of a mesh hierarchy, coarsest first, whose nodes are numbered so that nodes 2 j and 2 j + 1 of
level k are the children of node j of level k - 1 ("the specific construction of permuted nodes", models.py:591): level k of a
batch of B meshes padded to V_k = 2^k V_0 nodes is one block-diagonal operator of B V_k rows.

At equal widths `_LapResNet2(128, 128, inner_layers=2)` (models.py:447-477) is utils.LapResNet2(128): the same bn_fc0 / bn_fc1 keys,
the same arithmetic, and a mask that is never read — so every block runs on the whole-block kernels (blocks.py), and the two pooling
operations are one streaming pass each (functional.pool_max2, functional.unpool2_add; include/sn_spmm.h "Sibling-pair pooling").
`state_dict` keys and shapes are the reference's: conv1, down_rn{i}, lap0, up_rn{i}, conv2; the pooling modules hold no parameter.

Fake and padded nodes take part in the BatchNorm statistics and in the maximum, as in the reference (and as padded rows do in
every model of normal_predict).

The operators come from operators.mesh_hierarchy (this project's definition of the coarsening the reference names and does not
contain); normal_predict.NormalFrames(model="cas") builds one hierarchy per frame and samples batches with `Laps`.

Refused rather than approximated: bottleneck=True, naive_pool=False (_LaplacianPooling), inner_layers other than 2, bnmode other
than '', out_features other than 3.
"""
from __future__ import annotations

from . import functional as snF
from . import utils_pt as utils
from .normal_predict import _head_elu_conv, _NormalModel, repeating_expand

__all__ = ["LapCascade"]


def _refuse(what):
    raise NotImplementedError(f"cascade.LapCascade: {what} is not built on the HIP path (see the module docstring); "
                              "nothing approximates it")


class LapCascade(_NormalModel):
    """models.py:529-609.  Called as model(Laps, mask, inputs) with inputs (B, V, in_features), V a multiple of
    2^(cascade_levels - 1), and Laps the cascade_levels operators of the batch, coarsest first.  `with_avg` is accepted and
    unused, as in the reference."""

    def __init__(self, in_features=3, out_features=3, cascade_levels=4, inner_layers=2, bnmode="", with_avg=False, naive_pool=True,
                 bottleneck=False, **kwargs):
        super().__init__()
        if bottleneck:
            _refuse("bottleneck=True")
        if not naive_pool:
            _refuse("naive_pool=False")
        if inner_layers != 2:
            _refuse(f"inner_layers={inner_layers}")
        if bnmode != "":
            _refuse(f"bnmode={bnmode!r}")
        if out_features != 3:
            _refuse(f"out_features={out_features}")
        if cascade_levels < 1:
            raise ValueError(f"LapCascade: cascade_levels must be at least 1, got {cascade_levels}")
        self.conv1 = utils.GraphConv1x1(in_features, 128, batch_norm=None)
        self.cascade_num = int(cascade_levels)
        for i in range(self.cascade_num - 1, 0, -1):                      # 3, 2, 1: the reference's registration order
            self.add_module(f"down_rn{i}", utils.LapResNet2(128))
        self.lap0 = utils.LapResNet2(128)
        for i in range(1, self.cascade_num):
            self.add_module(f"up_rn{i}", utils.LapResNet2(128))
        self.conv2 = utils.GraphConv1x1(128, out_features, batch_norm="pre")

    # the two pooling operations (EfficientCascade._Pooling and the skip of models.py:597); tests swap torch's own in here
    def down_pool(self, x):
        return snF.pool_max2(x)

    def up_pool_add(self, x, skip):
        return snF.unpool2_add(x, skip)

    def features4(self, Laps, mask, inputs):
        n = self.cascade_num
        if len(Laps) != n:
            raise ValueError(f"LapCascade: {n} levels take {n} operators, coarsest first; got {len(Laps)}")
        B, V, _ = inputs.shape
        if V % (1 << (n - 1)):
            raise ValueError(f"LapCascade: {V} nodes per mesh are no multiple of 2^{n - 1} (pad the finest level of the hierarchy)")
        for k, L in enumerate(Laps):
            rows = B * (V >> (n - 1 - k))
            if tuple(L.shape) != (rows, rows):
                raise ValueError(f"LapCascade: Laps[{k}] is {tuple(L.shape)}, level {k} of this batch has {rows} nodes")
        x = self.conv1(inputs)
        down_series = []
        for i in range(n - 1, 0, -1):
            down_series.append(x)
            x = self._modules[f"down_rn{i}"](Laps[i], None, x)            # (the block never reads its mask)
            x = self.down_pool(x)
        x = self.lap0(Laps[0], None, x)
        for i in range(1, n):
            x = self.up_pool_add(x, down_series[-i])
            x = self._modules[f"up_rn{i}"](Laps[i], None, x)
        return _head_elu_conv(self.conv2, x), repeating_expand(inputs, 3)

    def fuzzy_load(self, pre_dict):
        """models.py:605-609: every entry of `pre_dict` with one of this model's keys is loaded."""
        model_dict = self.state_dict()
        model_dict.update({k: v for k, v in pre_dict.items() if k in model_dict})
        self.load_state_dict(model_dict)
