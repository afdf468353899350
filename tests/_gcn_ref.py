"""GCN restated in plain torch on the CPU: the reference of the GCN tests.  TEST INFRASTRUCTURE
ONLY; dgl and dgllife are not available here, so parity with them is unpinned ("GCN")
and the sources are cited by file and function, not by line:
  * dgl 0.9.1 python/dgl/nn/pytorch/conv/graphconv.py, GraphConv.forward: the source-side factor
    (norm 'left' / 'both': out-degrees clamped to 1, ^-1 / ^-1/2) scales feat; when in_feats >
    out_feats the product comes before update_all(copy_u('h', 'm'), sum('m', 'h')), else after;
    the destination-side factor (norm 'right' / 'both': in-degrees clamped to 1) scales the sum;
    then + bias, then the activation;
  * dgllife 0.3.0 model/gnn/gcn.py, GCNLayer.forward and GCN.forward;
  * dgllife 0.3.0 model/model_zoo/gcn_predictor.py, GCNPredictor.forward.

Every function runs in the dtype of its inputs (float64 for parity, float32 for the reference's
own error) and is differentiable with torch autograd, which supplies the reference backward.  The
modules hold their parameters under the product's state_dict keys, so a product model's state_dict
loads with load_state_dict(strict=True).

ReLU sides: every forward takes `sides`, None or a dict {"conv": [bool per layer], "res": [bool per
layer], "predict": bool}, the side of each ReLU's kink per element (the product's post-ReLU output
> 0), and `record`, None or a dict that receives the pre-activations under the same keys."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _predictor_ref import _ReadoutParams
from _readout_ref import wsum_max_ref
from oracle.gnn_ref import relu_branch

NORMS = ("none", "both", "right", "left")


def _long(a):
    return torch.as_tensor(a).to(torch.long)


def degree_scales(src, dst, n, norm, dtype):
    """(source-side, destination-side) factors of GraphConv's norm, [n] each."""
    src, dst = _long(src), _long(dst)
    outdeg = torch.bincount(src, minlength=n).clamp(min=1).to(dtype)
    indeg = torch.bincount(dst, minlength=n).clamp(min=1).to(dtype)
    one = torch.ones(n, dtype=dtype)
    if norm == "none":
        return one, one
    if norm == "both":
        return outdeg ** -0.5, indeg ** -0.5
    if norm == "right":
        return one, 1.0 / indeg
    if norm == "left":
        return 1.0 / outdeg, one
    raise ValueError(norm)


def neighbour_sum(src, dst, X, src_scale=None, dst_scale=None):
    """dst_scale[v] * sum over edges (u -> v) of src_scale[u] * X[u]."""
    src, dst = _long(src), _long(dst)
    h = X if src_scale is None else X * src_scale.unsqueeze(1)
    out = torch.zeros_like(X).index_add(0, dst, h[src])
    return out if dst_scale is None else out * dst_scale.unsqueeze(1)


def _act(pre, relu, side, record, key):
    if record is not None:
        record.setdefault(key, []).append(pre.detach())
    if not relu:
        return pre
    return F.relu(pre) if side is None else relu_branch(pre, side)


def graph_conv_ref(src, dst, X, weight, bias, norm="both", relu=False, order=None, side=None, record=None):
    """GraphConv.forward.  order: None (dgl's rule: the product first when in_feats > out_feats),
    "project" or "aggregate" — the same function either way."""
    n = X.shape[0]
    s, d = degree_scales(src, dst, n, norm, X.dtype)
    if order is None:
        order = "project" if weight.shape[0] > weight.shape[1] else "aggregate"
    if order == "project":
        rst = neighbour_sum(src, dst, (X * s.unsqueeze(1)) @ weight) * d.unsqueeze(1)
    else:
        rst = (neighbour_sum(src, dst, X * s.unsqueeze(1)) @ weight) * d.unsqueeze(1)
    if bias is not None:
        rst = rst + bias
    return _act(rst, relu, side, record, "conv")


class _GraphConvParams(nn.Module):
    def __init__(self, in_feats, out_feats):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(in_feats, out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats))


class GCNLayerRef(nn.Module):
    """dgllife GCNLayer; activation F.relu (relu=True) or None (identity on both branches: the
    product's documented deviation)."""

    def __init__(self, in_feats, out_feats, gnn_norm="none", relu=True, residual=True, batchnorm=True, dropout=0.):
        super().__init__()
        self.norm, self.relu = gnn_norm, relu
        self.graph_conv = _GraphConvParams(in_feats, out_feats)
        self.dropout = nn.Dropout(dropout)
        self.residual = residual
        if residual:
            self.res_connection = nn.Linear(in_feats, out_feats)
        self.bn = batchnorm
        if batchnorm:
            self.bn_layer = nn.BatchNorm1d(out_feats)

    def forward(self, graph, X, conv_side=None, res_side=None, record=None, mask=None):
        """mask: optional [N, out_feats] multiplier standing in for Dropout's draw (already scaled
        by 1 / (1 - p))."""
        new = graph_conv_ref(graph["src"], graph["dst"], X, self.graph_conv.weight, self.graph_conv.bias, self.norm,
                             self.relu, side=conv_side, record=record)
        if self.residual:
            new = new + _act(self.res_connection(X), self.relu, res_side, record, "res")
        new = self.dropout(new) if mask is None else new * mask
        if self.bn:
            b = self.bn_layer
            if b.training:
                b.num_batches_tracked += 1
            new = F.batch_norm(new, b.running_mean, b.running_var, b.weight, b.bias, b.training, b.momentum, b.eps)
        return new


class GCNRef(nn.Module):
    def __init__(self, in_feats, hidden_feats=None, gnn_norm=None, relu=None, residual=None, batchnorm=None):
        super().__init__()
        hidden_feats = list(hidden_feats) if hidden_feats is not None else [64, 64]
        n = len(hidden_feats)
        gnn_norm = gnn_norm or ["none"] * n
        relu = relu if relu is not None else [True] * n
        residual = residual if residual is not None else [True] * n
        batchnorm = batchnorm if batchnorm is not None else [True] * n
        self.hidden_feats = hidden_feats
        self.gnn_layers = nn.ModuleList()
        for i in range(n):
            self.gnn_layers.append(GCNLayerRef(in_feats, hidden_feats[i], gnn_norm[i], relu[i], residual[i], batchnorm[i]))
            in_feats = hidden_feats[i]

    def forward(self, graph, X, sides=None, record=None):
        for i, layer in enumerate(self.gnn_layers):
            X = layer(graph, X, None if sides is None else sides["conv"][i],
                      None if sides is None else sides["res"][i], record)
        return X


class _MLPPredictorRef(nn.Module):
    def __init__(self, in_feats, hidden_feats, n_tasks):
        super().__init__()
        self.predict = nn.Sequential(nn.Dropout(0.), nn.Linear(in_feats, hidden_feats), nn.ReLU(),
                                     nn.BatchNorm1d(hidden_feats), nn.Linear(hidden_feats, n_tasks))

    def forward(self, feats, side=None, record=None):
        drop, lin1, _, bn, lin2 = self.predict
        pre = lin1(drop(feats))
        if record is not None:
            record["predict"] = pre.detach()
        return lin2(bn(F.relu(pre) if side is None else relu_branch(pre, side)))


class GCNPredictorRef(nn.Module):
    """GCN -> WeightedSumAndMax -> MLPPredictor; graph is the oracle-side dict (src, dst,
    node_offsets).  argmax: the atoms that own the readout's maxima (tests/_readout_ref.py)."""

    def __init__(self, in_feats, hidden_feats=None, gnn_norm=None, predictor_hidden_feats=128, n_tasks=1):
        super().__init__()
        self.gnn = GCNRef(in_feats, hidden_feats, gnn_norm)
        last = self.gnn.hidden_feats[-1]
        self.readout = _ReadoutParams(last)
        self.predict = _MLPPredictorRef(2 * last, predictor_hidden_feats, n_tasks)

    def forward(self, graph, X, sides=None, record=None, argmax=None):
        h = self.gnn(graph, X, sides, record)
        lin = self.readout.weight_and_sum.atom_weighting[0]
        ro, _ = wsum_max_ref(graph["node_offsets"], h, lin.weight, lin.bias, argmax=argmax)
        return self.predict(ro, None if sides is None else sides["predict"], record)
