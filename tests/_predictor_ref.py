"""GATPredictor / GATv2Predictor restated in plain torch on the CPU (dgllife 0.3.0's model_zoo
classes): the reference of the predictor tests.  TEST INFRASTRUCTURE ONLY; dgl and dgllife are not
available here, so parity with them is unpinned ("GATPredictor / BatchNorm1d").

The composition is conv -> WeightedSumAndMax -> MLPPredictor from
  * oracle.gnn_ref's GAT layers (gat_layer_ref), or tests/_gatv2_ref.py for GATv2,
  * tests/_readout_ref.py (wsum_max_ref),
  * plain torch Dropout(0), Linear, ReLU, BatchNorm1d, Linear.
The modules below only hold parameters under the product's state_dict keys, so a product model's
state_dict loads with load_state_dict(strict=True); .double() gives the float64 reference, the
float32 original the reference's own error.  Kinks (LeakyReLU sides, ReLU sides, the max's ties)
can be evaluated on the product's side, as everywhere in the parity tests."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _gatv2_ref import gatv2_layer_ref
from _readout_ref import wsum_max_ref
from oracle.gnn_ref import _GATConvParams, gat_layer_ref, relu_branch


class _GATv2ConvParams(nn.Module):
    """Parameter layout of dgl 0.9.1 GATv2Conv with a projecting residual (registration order:
    attn, fc_src, fc_dst, res_fc)."""

    def __init__(self, in_feats, out_feats, num_heads):
        super().__init__()
        self.fc_src = nn.Linear(in_feats, out_feats * num_heads)
        self.fc_dst = nn.Linear(in_feats, out_feats * num_heads)
        self.attn = nn.Parameter(torch.zeros(1, num_heads, out_feats))
        self.res_fc = nn.Linear(in_feats, out_feats * num_heads)


class _Layer(nn.Module):
    def __init__(self, kind, in_feats, out_feats, num_heads):
        super().__init__()
        if kind == "gat":
            self.gat_conv = _GATConvParams(in_feats, out_feats, num_heads)
        else:
            self.gatv2_conv = _GATv2ConvParams(in_feats, out_feats, num_heads)


class _Stack(nn.Module):
    def __init__(self, kind, in_feats, hidden_feats, num_heads, agg_modes):
        super().__init__()
        self.gnn_layers = nn.ModuleList()
        for hf, nh, mode in zip(hidden_feats, num_heads, agg_modes):
            if in_feats == hf * nh:
                raise ValueError("the reference composes projected residuals only")
            self.gnn_layers.append(_Layer(kind, in_feats, hf, nh))
            in_feats = hf * nh if mode == "flatten" else hf


class _WeightAndSumParams(nn.Module):
    def __init__(self, in_feats):
        super().__init__()
        self.atom_weighting = nn.Sequential(nn.Linear(in_feats, 1), nn.Sigmoid())


class _ReadoutParams(nn.Module):
    def __init__(self, in_feats):
        super().__init__()
        self.weight_and_sum = _WeightAndSumParams(in_feats)


class MLPPredictorRef(nn.Module):
    """dgllife MLPPredictor in plain torch.  forward(feats, relu_side=None): relu_side (bool, the
    product's post-ReLU output > 0) evaluates the ReLU on that side of its kink."""

    def __init__(self, in_feats, hidden_feats, n_tasks, dropout=0.):
        super().__init__()
        self.predict = nn.Sequential(nn.Dropout(dropout), nn.Linear(in_feats, hidden_feats), nn.ReLU(),
                                     nn.BatchNorm1d(hidden_feats), nn.Linear(hidden_feats, n_tasks))

    def forward(self, feats, relu_side=None):
        if relu_side is None:
            return self.predict(feats)
        drop, lin1, _, bn, lin2 = self.predict
        return lin2(bn(relu_branch(lin1(drop(feats)), relu_side)))


class PredictorRef(nn.Module):
    """kind "gat": GATPredictor; "gatv2": GATv2Predictor (dgllife's defaults otherwise: ELU on all
    but the last layer, slope 0.2, projected residuals, biases).  forward(graph, X, ...) with graph
    the oracle-side dict (numpy src, dst, node_offsets) returns (B, n_tasks) logits."""

    def __init__(self, kind, in_feats, hidden_feats, num_heads, agg_modes=None, predictor_hidden_feats=128,
                 n_tasks=1, predictor_dropout=0.):
        super().__init__()
        n = len(hidden_feats)
        self.kind = kind
        self.hidden_feats, self.num_heads = list(hidden_feats), list(num_heads)
        self.agg_modes = list(agg_modes) if agg_modes is not None else ["flatten"] * (n - 1) + ["mean"]
        self.activations = [F.elu] * (n - 1) + [None]
        self.gnn = _Stack(kind, in_feats, self.hidden_feats, self.num_heads, self.agg_modes)
        last = self.hidden_feats[-1] * (self.num_heads[-1] if self.agg_modes[-1] == "flatten" else 1)
        self.gnn_out_feats = last
        self.readout = _ReadoutParams(last)
        self.predict = MLPPredictorRef(2 * last, predictor_hidden_feats, n_tasks, predictor_dropout)

    def node_feats(self, graph, X, branches=None):
        h = X
        for i, layer in enumerate(self.gnn.gnn_layers):
            br = None if branches is None else branches[i]
            args = (self.num_heads[i], self.hidden_feats[i], self.agg_modes[i], self.activations[i])
            if self.kind == "gat":
                h = gat_layer_ref(graph["src"], graph["dst"], h, dict(layer.gat_conv.named_parameters()), *args,
                                  branch=br)
            else:
                h = gatv2_layer_ref(graph["src"], graph["dst"], h, dict(layer.gatv2_conv.named_parameters()), *args,
                                    branch=br)
        return h

    def forward(self, graph, X, branches=None, relu_side=None, argmax=None):
        h = self.node_feats(graph, X, branches)
        lin = self.readout.weight_and_sum.atom_weighting[0]
        ro, _ = wsum_max_ref(graph["node_offsets"], h, lin.weight, lin.bias, argmax=argmax)
        return self.predict(ro, relu_side)
