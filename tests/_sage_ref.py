"""GraphSAGE restated in plain torch on the CPU: the reference of the GraphSAGE tests.  TEST
INFRASTRUCTURE ONLY; dgl and dgllife are not available here, so parity with them is unpinned
("GraphSAGE") and the sources are cited by file and function, not by line:
  * dgl 0.9.1 python/dgl/nn/pytorch/conv/sageconv.py, SAGEConv.forward: h = feat_drop(feat);
    mean: h_neigh = fc_neigh(mean over in-edges of h), the product first when in_feats > out_feats;
    gcn: h_neigh = fc_neigh((sum over in-edges of h + h) / (in_degree + 1)), same order rule;
    pool: h_neigh = fc_neigh(max over in-edges of relu(fc_pool(h)));
    rst = fc_self(h) + h_neigh (gcn: h_neigh alone), + bias, then the activation.  An atom without
    in-edges has a neighbour mean / sum / max of 0;
  * dgllife 0.3.0 model/gnn/graphsage.py, GraphSAGE.forward;
  * dgllife 0.3.0 model/model_zoo/graphsage_predictor.py, GraphSAGEPredictor.forward.

Every function runs in the dtype of its inputs (float64 for parity, float32 for the reference's
own error) and is differentiable with torch autograd, which supplies the reference backward.  The
modules hold their parameters under the product's state_dict keys, so a product model's state_dict
loads with load_state_dict(strict=True).

Sides from outside: every forward takes `sides`, None or a dict {"out": [bool tensor or None per
layer], "pool": [bool tensor or None per layer], "arg": [int tensor or None per layer], "predict":
bool tensor or None}: the side of each ReLU's kink per element (the product's post-ReLU output > 0)
and, for a pool layer, the global in-CSR slot that owns each maximum (-1: a row without in-edges).
`record`, None or a dict, receives under "out" / "pool" the pre-activations and under "arg" a tuple
(own argmax, pooled values, in_src) per pool layer."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _gcn_ref import _MLPPredictorRef, _act, _long, neighbour_sum
from _predictor_ref import _ReadoutParams
from _readout_ref import wsum_max_ref

AGGREGATORS = ("mean", "gcn", "pool")


def in_csr(src, dst, n):
    """(rowptr [n + 1], in_src [E], order [E]): the edges sorted by destination, stable in edge id,
    as mvml_build_csr lays the in-CSR out; slot s holds edge order[s]."""
    src, dst = _long(src), _long(dst)
    order = torch.argsort(dst, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return rowptr, src[order], order


def first_argmax(src, dst, X):
    """arg[v, c]: the global in-CSR slot of the first slot in row order that attains
    max_s X[in_src[s], c] over v's row; -1 for a row without entries."""
    n, D = X.shape
    _, in_src, order = in_csr(src, dst, n)
    E = int(order.numel())
    if E == 0:
        return torch.full((n, D), -1, dtype=torch.long)
    in_dst = _long(dst)[order]
    vals = X.detach()[in_src]
    idx = in_dst.unsqueeze(1).expand(E, D)
    mx = torch.full((n, D), float("-inf"), dtype=X.dtype).scatter_reduce(0, idx, vals, "amax", include_self=True)
    slot = torch.arange(E).unsqueeze(1).expand(E, D)
    cand = torch.where(vals == mx[in_dst], slot, torch.full_like(slot, E))
    arg = torch.full((n, D), E, dtype=torch.long).scatter_reduce(0, idx, cand, "amin", include_self=True)
    return torch.where(arg == E, torch.full_like(arg, -1), arg)


def neighbour_max(src, dst, X, arg=None):
    """(out, own): out[v, c] = X[in_src[a[v, c]], c] with a = arg if given, else own = first_argmax;
    0 where a is -1.  Differentiable in X: the gradient goes to the row at a."""
    n = X.shape[0]
    own = first_argmax(src, dst, X)
    use = own if arg is None else _long(arg)
    _, in_src, _ = in_csr(src, dst, n)
    if in_src.numel() == 0:
        return torch.zeros_like(X), own
    rows = in_src[use.clamp(min=0)]
    out = torch.where(use >= 0, torch.gather(X, 0, rows), torch.zeros_like(X))  # (+0, not -0 * x)
    return out, own


def sage_conv_ref(src, dst, X, params, aggr, relu=False, side=None, pool_side=None, arg=None, record=None):
    """SAGEConv.forward after feat_drop.  params: an object with fc_pool / fc_self / fc_neigh / bias
    (those the aggregator has)."""
    n, fin = X.shape
    src, dst = _long(src), _long(dst)
    indeg = torch.bincount(dst, minlength=n).to(X.dtype)
    fout = params.fc_neigh.weight.shape[0]
    first = fin > fout  # dgl's lin_before_mp
    if aggr == "mean":
        inv = 1.0 / indeg.clamp(min=1)
        h_neigh = (neighbour_sum(src, dst, params.fc_neigh(X), None, inv) if first
                   else params.fc_neigh(neighbour_sum(src, dst, X, None, inv)))
    elif aggr == "gcn":
        t = params.fc_neigh(X) if first else X
        h_neigh = (neighbour_sum(src, dst, t) + t) / (indeg + 1).unsqueeze(1)
        if not first:
            h_neigh = params.fc_neigh(h_neigh)
    elif aggr == "pool":
        p = _act(params.fc_pool(X), True, pool_side, record, "pool")
        m, own = neighbour_max(src, dst, p, arg)
        if record is not None:
            record.setdefault("arg", []).append((own, p.detach(), in_csr(src, dst, n)[1]))
        h_neigh = params.fc_neigh(m)
    else:
        raise KeyError(aggr)
    rst = h_neigh if aggr == "gcn" else params.fc_self(X) + h_neigh
    if params.bias is not None:
        rst = rst + params.bias
    return _act(rst, relu, side, record, "out")


class SAGEConvRef(nn.Module):
    def __init__(self, in_feats, out_feats, aggregator_type, relu=False, bias=True):
        super().__init__()
        self.aggr, self.relu = aggregator_type, relu
        if aggregator_type == "pool":
            self.fc_pool = nn.Linear(in_feats, in_feats)
        if aggregator_type != "gcn":
            self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_feats))
        else:
            self.register_buffer("bias", None)

    def forward(self, graph, X, side=None, pool_side=None, arg=None, record=None, mask=None):
        """mask: optional [N, in_feats] multiplier standing in for feat_drop's draw (already
        scaled by 1 / (1 - p)); both branches read the masked tensor."""
        h = X if mask is None else X * mask
        return sage_conv_ref(graph["src"], graph["dst"], h, self, self.aggr, self.relu, side, pool_side, arg, record)


class GraphSAGERef(nn.Module):
    def __init__(self, in_feats, hidden_feats=None, relu=None, aggregator_type=None):
        super().__init__()
        hidden_feats = list(hidden_feats) if hidden_feats is not None else [64, 64]
        n = len(hidden_feats)
        relu = relu if relu is not None else [True] * n
        aggregator_type = aggregator_type if aggregator_type is not None else ["mean"] * n
        self.hidden_feats = hidden_feats
        self.gnn_layers = nn.ModuleList()
        for i in range(n):
            self.gnn_layers.append(SAGEConvRef(in_feats, hidden_feats[i], aggregator_type[i], relu[i]))
            in_feats = hidden_feats[i]

    def forward(self, graph, X, sides=None, record=None):
        for i, layer in enumerate(self.gnn_layers):
            s = (lambda k: None) if sides is None else (lambda k: sides[k][i])
            X = layer(graph, X, s("out"), s("pool"), s("arg"), record)
        return X


class GraphSAGEPredictorRef(nn.Module):
    """GraphSAGE -> WeightedSumAndMax -> MLPPredictor; graph is the oracle-side dict (src, dst,
    node_offsets).  argmax: the atoms that own the readout's maxima (tests/_readout_ref.py)."""

    def __init__(self, in_feats, hidden_feats=None, aggregator_type=None, predictor_hidden_feats=128, n_tasks=1):
        super().__init__()
        self.gnn = GraphSAGERef(in_feats, hidden_feats, None, aggregator_type)
        last = self.gnn.hidden_feats[-1]
        self.readout = _ReadoutParams(last)
        self.predict = _MLPPredictorRef(2 * last, predictor_hidden_feats, n_tasks)

    def forward(self, graph, X, sides=None, record=None, argmax=None):
        h = self.gnn(graph, X, sides, record)
        lin = self.readout.weight_and_sum.atom_weighting[0]
        ro, _ = wsum_max_ref(graph["node_offsets"], h, lin.weight, lin.bias, argmax=argmax)
        return self.predict(ro, None if sides is None else sides["predict"], record)
