"""GIN with bond embeddings restated in plain torch on the CPU: the reference of the GIN tests.
TEST INFRASTRUCTURE ONLY; dgl and dgllife are not available here, so parity with them is unpinned
("GIN") and the sources are cited by file and function, not by line:
  * dgllife 0.3.0 model/gnn/gin.py, GINLayer.forward: edge_embeds = sum_t edge_embeddings[t](cat_t);
    update_all(u_add_e, sum): h[v] = sum over in-edges (u -> v) of (node_feats[u] + edge_embeds[uv]);
    h = mlp(h) with mlp = Linear(D, 2D), ReLU, Linear(2D, D); then bn and the activation;
  * the same file, GIN.forward: h_0 = sum_t node_embeddings[t](idx_t); h_{l+1} =
    dropout(layer_l(g, h_l, edge_feats)); JK 'last' / 'concat' (dim 1) / 'sum' over [h_0 .. h_L];
  * dgllife 0.3.0 model/model_zoo/gin_predictor.py, GINPredictor.forward: dgl's SumPooling /
    AvgPooling / MaxPooling per molecule, then predict = Linear.

Every function runs in the dtype of its float inputs (float64 for parity, float32 for the
reference's own error) and is differentiable with torch autograd, which supplies the reference
backward.  The modules hold their parameters under the product's state_dict keys, so a product
model's state_dict loads with load_state_dict(strict=True).

Sides from outside: the forwards take `sides`, None or a dict {"hidden": [bool tensor per layer],
"out": [bool tensor or None per layer], "argmax": int tensor or None}: the side of each ReLU's kink
per element (the product's post-ReLU value > 0) and, for the max readout, the atom that owns each
maximum (-1: an empty molecule).  `record`, None or a dict, receives under "hidden" / "out" the
pre-activations and under "argmax" a tuple (own argmax, pooled rows).  masks: None or one [N, D]
multiplier per layer standing in for the Dropout draw (already scaled by 1 / (1 - p))."""
import torch
import torch.nn as nn

from _gcn_ref import _act, _long

POOLS = ("sum", "mean", "max")


def edge_term(tables, cats):
    """sum_t tables[t][cats[t]]: [E, D]."""
    e = tables[0][_long(cats[0])]
    for w, c in zip(tables[1:], cats[1:]):
        e = e + w[_long(c)]
    return e


def gin_agg_ref(src, dst, X, tables, cats):
    """h[v] = sum over edges (u -> v) of (X[u] + e_uv); a row without in-edges is 0."""
    src, dst = _long(src), _long(dst)
    if src.numel() == 0:
        return torch.zeros_like(X)
    return torch.zeros_like(X).index_add(0, dst, X[src] + edge_term(tables, cats))


def embed_sum_ref(tables, idx):
    return edge_term(tables, idx)


def first_owner(offsets, X):
    """argmax[g, c]: the lowest atom index that attains max_n X[n, c] over molecule g; -1 for an
    empty molecule."""
    offsets = [int(o) for o in offsets]
    B, D = len(offsets) - 1, X.shape[1]
    arg = torch.full((B, D), -1, dtype=torch.long)
    for g in range(B):
        a, b = offsets[g], offsets[g + 1]
        if b > a:
            rows = X.detach()[a:b]
            # (argmax of the 0 / 1 mask: torch returns the first of several maximal values)
            arg[g] = (rows == rows.max(dim=0).values).to(torch.uint8).argmax(dim=0) + a
    return arg


def segment_pool_ref(offsets, X, mode, argmax=None):
    """(out [B, D], own argmax or None): dgl's SumPooling / AvgPooling / MaxPooling; an empty
    molecule gives 0.  max gathers at `argmax` when given (differentiable: the gradient goes to the
    owning atom's row)."""
    offsets = [int(o) for o in offsets]
    B, D = len(offsets) - 1, X.shape[1]
    if mode == "max":
        own = first_owner(offsets, X)
        use = own if argmax is None else _long(argmax)
        if X.shape[0] == 0:
            return torch.zeros((B, D), dtype=X.dtype), own
        out = torch.where(use >= 0, torch.gather(X, 0, use.clamp(min=0)), torch.zeros((B, D), dtype=X.dtype))
        return out, own
    rows = []
    for g in range(B):
        a, b = offsets[g], offsets[g + 1]
        s = X[a:b].sum(dim=0) if b > a else torch.zeros(D, dtype=X.dtype)
        rows.append(s / (b - a) if mode == "mean" and b > a else s)
    return (torch.stack(rows) if rows else torch.zeros((0, D), dtype=X.dtype)), None


class GINLayerRef(nn.Module):
    def __init__(self, num_edge_emb_list, emb_dim, batch_norm=True, relu=False):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.ReLU(), nn.Linear(2 * emb_dim, emb_dim))
        self.edge_embeddings = nn.ModuleList(nn.Embedding(n, emb_dim) for n in num_edge_emb_list)
        self.bn = nn.BatchNorm1d(emb_dim) if batch_norm else None
        self.relu = relu

    def forward(self, graph, X, cats, hidden_side=None, out_side=None, record=None):
        h = gin_agg_ref(graph["src"], graph["dst"], X, [e.weight for e in self.edge_embeddings], cats)
        h = _act(self.mlp[0](h), True, hidden_side, record, "hidden")
        h = self.mlp[2](h)
        if self.bn is not None:
            h = self.bn(h)
        return _act(h, self.relu, out_side, record, "out")


class GINRef(nn.Module):
    def __init__(self, num_node_emb_list, num_edge_emb_list, num_layers=5, emb_dim=300, JK="last"):
        super().__init__()
        self.JK = JK
        self.node_embeddings = nn.ModuleList(nn.Embedding(n, emb_dim) for n in num_node_emb_list)
        self.gnn_layers = nn.ModuleList(GINLayerRef(num_edge_emb_list, emb_dim, relu=layer < num_layers - 1)
                                        for layer in range(num_layers))

    def forward(self, graph, node_cats, edge_cats, sides=None, record=None, masks=None):
        hs = [embed_sum_ref([e.weight for e in self.node_embeddings], node_cats)]
        for i, layer in enumerate(self.gnn_layers):
            s = (lambda k: None) if sides is None else (lambda k: sides[k][i])
            h = layer(graph, hs[-1], edge_cats, s("hidden"), s("out"), record)
            hs.append(h if masks is None or masks[i] is None else h * masks[i])
        if self.JK == "last":
            return hs[-1]
        if self.JK == "concat":
            return torch.cat(hs, dim=1)
        out = hs[0]
        for h in hs[1:]:
            out = out + h
        return out


class GINPredictorRef(nn.Module):
    """graph: the oracle-side dict (src, dst, node_offsets)."""

    def __init__(self, num_node_emb_list, num_edge_emb_list, num_layers=5, emb_dim=300, JK="last", readout="mean",
                 n_tasks=1):
        super().__init__()
        self.gnn = GINRef(num_node_emb_list, num_edge_emb_list, num_layers, emb_dim, JK)
        self.readout = readout
        self.predict = nn.Linear((num_layers + 1) * emb_dim if JK == "concat" else emb_dim, n_tasks)

    def forward(self, graph, node_cats, edge_cats, sides=None, record=None, masks=None):
        h = self.gnn(graph, node_cats, edge_cats, sides, record, masks)
        ro, own = segment_pool_ref(graph["node_offsets"], h, self.readout, None if sides is None else sides.get("argmax"))
        if record is not None and own is not None:
            record["argmax"] = (own, h.detach())
        return self.predict(ro)
