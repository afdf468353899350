"""Weave's layers (dgllife 0.3.0 WeaveLayer / WeaveGNN / WeavePredictor, restated) in plain torch,
dtype-generic, edge-list form with every [E, H] intermediate materialised.  `sd` maps the state_dict keys
below `pre` to tensors of the working dtype; edge rows are in edge-id order."""
import torch
import torch.nn.functional as F

import _weave_ref as G

LINEARS = ("node_to_node", "edge_to_node", "update_node", "left_node_to_edge", "right_node_to_edge", "edge_to_edge",
           "update_edge")


def layer(sd, pre, src, dst, x, e, node_only=False):
    lin = lambda name, t: F.linear(t, sd[pre + name + ".weight"], sd[pre + name + ".bias"])
    S = torch.zeros((x.shape[0], sd[pre + "edge_to_node.bias"].shape[0]), dtype=x.dtype).index_add_(
        0, dst, F.relu(lin("edge_to_node", e)))
    xn = F.relu(lin("update_node", torch.cat([F.relu(lin("node_to_node", x)), S], 1)))
    if node_only:
        return xn
    L, R = lin("left_node_to_edge", x), lin("right_node_to_edge", x)
    pair = F.relu(L[src] + R[dst]) + F.relu(R[src] + L[dst])
    return xn, F.relu(lin("update_edge", torch.cat([pair, F.relu(lin("edge_to_edge", e))], 1)))


def gnn(sd, pre, src, dst, x, e, num_layers):
    for i in range(num_layers - 1):
        x, e = layer(sd, f"{pre}gnn_layers.{i}.", src, dst, x, e)
    return layer(sd, f"{pre}gnn_layers.{num_layers - 1}.", src, dst, x, e, node_only=True)


def predictor(sd, src, dst, gid, B, x, e, num_layers, means, stds, eps=1e-5):
    """Train mode: BatchNorm1d with the batch's biased statistics."""
    h = gnn(sd, "gnn.", src, dst, x, e, num_layers)
    h = torch.tanh(F.linear(h, sd["node_to_graph.0.weight"], sd["node_to_graph.0.bias"]))
    h = (h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + eps) * sd["node_to_graph.2.weight"] + sd["node_to_graph.2.bias"]
    y = G.gather(h, gid, B, means, stds, sd["readout.to_out.weight"], sd["readout.to_out.bias"])
    return F.linear(y, sd["predict.weight"], sd["predict.bias"])
