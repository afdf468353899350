"""nn.Modules with the reference's constructor signatures and state_dict layout.

Drop-in replacements, on the MI355X HIP path, for
  * dgl 0.9.1 ``GATConv`` and dgllife 0.3.0 ``GATLayer`` / ``GAT`` (model.py:6, 81, 91),
  * dgl 0.9.1 ``Set2Set`` (model.py:7, 82-84, 92),
  * dgllife 0.3.0 ``WeightAndSum`` / ``WeightedSumAndMax`` (a second readout; not in model.py),
  * torch_geometric 2.2.0 ``GraphNorm`` (model.py:10, 85, 93),
  * ``GNNModule`` itself (model.py:77-95),
  * dgllife 0.3.0 ``MLPPredictor`` / ``GATPredictor`` / ``GATv2Predictor`` (the single-view graph
    classifiers; not in model.py),
  * dgl 0.9.1 ``GraphConv`` and dgllife 0.3.0 ``GCNLayer`` / ``GCN`` / ``GCNPredictor`` (the GCN
    baseline; not in model.py),
  * dgl 0.9.1 ``SAGEConv`` and dgllife 0.3.0 ``GraphSAGE`` / ``GraphSAGEPredictor`` (the GraphSAGE
    baseline; not in model.py),
  * dgllife 0.3.0 ``GINLayer`` / ``GIN`` / ``GINPredictor`` (the bond-aware gin_supervised_* family
    over categorical atom and bond features; not in model.py).
Parameter names/shapes/registration order follow the reference so a ``net_i.pkl``
``model_state_dict`` (keys under ``gnn.``) loads unchanged.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from .batching import BatchedMolGraph


class GATConv(nn.Module):
    """dgl.nn.pytorch.GATConv (0.9.1) parameters, with feat/attn dropout 0.  The residual kind
    follows DGL's rule: residual=True makes res_fc a bias-free Linear when in_feats !=
    heads*out_feats and nn.Identity() when they are equal (rst += feat.view(N, H, F)); residual=
    False registers res_fc as a None buffer; bias=False registers bias as one.  So the state_dict
    has res_fc.weight only for a projecting residual and bias only with bias=True, as DGL's.
    forward() returns rst (N, H, F) like DGL (activation None)."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0,
                 negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False, bias=True):
        super().__init__()
        if feat_drop or attn_drop:
            raise NotImplementedError("GATConv: feat_drop/attn_drop > 0 are not on the fused path")
        # the aggregation kernels' range (csrc/gat_agg_common.h check_shapes): refuse here, not in forward
        if num_heads not in (1, 2, 4, 8) or out_feats <= 0 or out_feats % 4 or num_heads * out_feats > 2048:
            raise ValueError(
                f"GATConv: num_heads must be 1, 2, 4 or 8 and out_feats a positive multiple of 4 with "
                f"num_heads * out_feats <= 2048 (got num_heads={num_heads}, out_feats={out_feats})")
        self._num_heads = num_heads
        self._in_feats = in_feats
        self._out_feats = out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self.negative_slope = negative_slope
        self.activation = activation
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        if bias:
            self.bias = nn.Parameter(torch.empty(num_heads * out_feats))
        else:
            self.register_buffer("bias", None)
        if not residual:
            self.res_kind = Fn.RES_NONE
            self.register_buffer("res_fc", None)
        elif in_feats == num_heads * out_feats:
            self.res_kind = Fn.RES_IDENTITY
            self.res_fc = nn.Identity()
        else:
            self.res_kind = Fn.RES_PROJ
            self.res_fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
        # GEMM operand precision of fc / res_fc (forward and both backward products): None =
        # fp32-accurate (the reference's fp32), torch.bfloat16 = bf16 operands with fp32
        # accumulation (BASELINE config 4, accuracy bar 2e-2).  Parameters stay fp32.
        self.proj_dtype = None
        self.reset_parameters()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        """Accept both DGL GATConv parameter layouts.  dgl 0.9.1 (README.md pins) keeps an
        explicit ``bias`` and a bias-free ``res_fc``; later DGL releases fold the bias into the
        residual Linear (``res_fc.bias``, no ``bias``) when ``res_fc`` projects.  The arithmetic
        is the same (res_fc(x) + b), so the folded form loads into ``bias`` here (a projecting
        res_fc with a bias only: the other kinds have no res_fc keys at all)."""
        rb, b = prefix + "res_fc.bias", prefix + "bias"
        if self.res_kind == Fn.RES_PROJ and self.bias is not None and rb in state_dict and b not in state_dict:
            state_dict[b] = state_dict.pop(rb)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if self.bias is not None:
            nn.init.constant_(self.bias, 0)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def _check_graph(self, graph):
        if not isinstance(graph, BatchedMolGraph):
            raise TypeError("graph must be a mvml_gat.BatchedMolGraph (see mvml_gat.batch)")
        if graph.device.type != "cuda":
            raise RuntimeError("graph must be moved to the GPU with .to('cuda') first")
        if graph.has_zero_in_degree and not self._allow_zero_in_degree:
            raise RuntimeError(
                "There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                "Adding self-loop on the input graph by calling `g = dgl.add_self_loop(g)` will resolve "
                "the issue. Setting ``allow_zero_in_degree`` to be `True` when constructing this module "
                "will suppress the check and let the code run.")

    def fused(self, graph, feat, mode):
        self._check_graph(graph)
        res_w = self.res_fc.weight if self.res_kind == Fn.RES_PROJ else None
        return Fn.GATLayerFunction.apply(feat, self.fc.weight, res_w, self.attn_l,
                                         self.attn_r, self.bias, graph, self._num_heads,
                                         self._out_feats, self.negative_slope, mode,
                                         "bf16" if self.proj_dtype == torch.bfloat16 else None,
                                         self.res_kind)

    def forward(self, graph, feat):
        rst = self.fused(graph, feat, Fn.MODE_FLATTEN).view(-1, self._num_heads, self._out_feats)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class GATLayer(nn.Module):
    """dgllife.model.gnn.gat.GATLayer (0.3.0): gat_conv -> flatten(1) | mean(1) -> activation,
    fused into one kernel for the (flatten, ELU) and (mean, None) combinations GAT uses."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, alpha=0.2,
                 residual=True, agg_mode="flatten", activation=None, bias=True,
                 allow_zero_in_degree=False):
        super().__init__()
        self.gat_conv = GATConv(in_feats, out_feats, num_heads, feat_drop, attn_drop, alpha,
                                residual, None, allow_zero_in_degree, bias)
        assert agg_mode in ["flatten", "mean"]
        self.agg_mode = agg_mode
        self.activation = activation

    def forward(self, bg, feats):
        act = self.activation
        if self.agg_mode == "flatten":
            if act is F.elu:
                return self.gat_conv.fused(bg, feats, Fn.MODE_FLATTEN_ELU)
            out = self.gat_conv.fused(bg, feats, Fn.MODE_FLATTEN)
        else:
            out = self.gat_conv.fused(bg, feats, Fn.MODE_MEAN)
        return act(out) if act is not None else out


class GAT(nn.Module):
    """dgllife.model.gnn.gat.GAT (0.3.0) with its defaults: 4 heads per layer, alpha 0.2,
    residual, 'flatten' + ELU for all but the last layer, 'mean' + no activation last.
    ``residuals`` / ``biases`` are passed through per layer; a layer whose input width equals
    heads * hidden gets DGL's identity residual (e.g. every layer after the first of
    hidden_feats = [64, 64])."""

    def __init__(self, in_feats, hidden_feats=None, num_heads=None, feat_drops=None,
                 attn_drops=None, alphas=None, residuals=None, agg_modes=None, activations=None,
                 biases=None, allow_zero_in_degree=False):
        super().__init__()
        hidden_feats = list(hidden_feats) if hidden_feats is not None else [32, 32]
        n = len(hidden_feats)
        num_heads = num_heads or [4] * n
        feat_drops = feat_drops or [0.0] * n
        attn_drops = attn_drops or [0.0] * n
        alphas = alphas or [0.2] * n
        residuals = residuals or [True] * n
        if agg_modes is None:
            agg_modes = ["flatten"] * (n - 1) + ["mean"]
        if activations is None:
            activations = [F.elu] * (n - 1) + [None]
        biases = biases or [True] * n
        self.hidden_feats = hidden_feats
        self.num_heads = num_heads
        self.agg_modes = agg_modes
        self.gnn_layers = nn.ModuleList()
        for i in range(n):
            self.gnn_layers.append(GATLayer(in_feats, hidden_feats[i], num_heads[i], feat_drops[i],
                                            attn_drops[i], alphas[i], residuals[i], agg_modes[i],
                                            activations[i], biases[i], allow_zero_in_degree))
            in_feats = hidden_feats[i] * num_heads[i] if agg_modes[i] == "flatten" else hidden_feats[i]

    def reset_parameters(self):
        for layer in self.gnn_layers:
            layer.gat_conv.reset_parameters()

    def forward(self, g, feats):
        # inside the stack a flatten + ELU layer's output feeds only the next layer: its ELU
        # backward may run in that layer's data-gradient GEMM (functional.EluLink)
        prev, Fn.ELU_LINK[0] = Fn.ELU_LINK[0], True
        try:
            for gnn in self.gnn_layers:
                feats = gnn(g, feats)
        finally:
            Fn.ELU_LINK[0] = prev
        return feats


class GATv2Conv(nn.Module):
    """dgl.nn.pytorch.GATv2Conv (0.9.1) parameters, with feat/attn dropout 0 (restated; parity with
    dgl is unpinned).  fc_src = Linear(in, H F, bias=bias); fc_dst is the same module with
    share_weights, else a second such Linear; attn (1, H, F); res_fc a Linear(in, H F, bias=bias)
    when residual and in_feats != H F, nn.Identity() when they are equal, a None buffer with
    residual=False.  There is no separate bias parameter.  forward() returns rst (N, H, F), and
    with get_attention=True also the attention (E, H, 1) in edge-id order, detached."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0,
                 negative_slope=0.2, residual=False, activation=None, allow_zero_in_degree=False,
                 bias=True, share_weights=False):
        super().__init__()
        if feat_drop or attn_drop:
            raise NotImplementedError("GATv2Conv: feat_drop/attn_drop > 0 are not on the fused path")
        # the aggregation kernels' range (csrc/gatv2_agg.hip check_shapes): refuse here, not in forward
        if num_heads not in (1, 2, 4, 8) or out_feats <= 0 or out_feats % 4 or num_heads * out_feats > 2048:
            raise ValueError(
                f"GATv2Conv: num_heads must be 1, 2, 4 or 8 and out_feats a positive multiple of 4 with "
                f"num_heads * out_feats <= 2048 (got num_heads={num_heads}, out_feats={out_feats})")
        self._num_heads = num_heads
        self._in_feats = in_feats
        self._out_feats = out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self.negative_slope = negative_slope
        self.activation = activation
        self.share_weights = share_weights
        self.bias = bias
        self.fc_src = nn.Linear(in_feats, out_feats * num_heads, bias=bias)
        self.fc_dst = self.fc_src if share_weights else nn.Linear(in_feats, out_feats * num_heads, bias=bias)
        self.attn = nn.Parameter(torch.empty(1, num_heads, out_feats))
        if not residual:
            self.res_kind = Fn.RES_NONE
            self.register_buffer("res_fc", None)
        elif in_feats == num_heads * out_feats:
            self.res_kind = Fn.RES_IDENTITY
            self.res_fc = nn.Identity()
        else:
            self.res_kind = Fn.RES_PROJ
            self.res_fc = nn.Linear(in_feats, num_heads * out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        linears = [self.fc_src] + ([] if self.share_weights else [self.fc_dst])
        if isinstance(self.res_fc, nn.Linear):
            linears.append(self.res_fc)
        for lin in linears:
            nn.init.xavier_normal_(lin.weight, gain=gain)
            if lin.bias is not None:
                nn.init.constant_(lin.bias, 0)
        nn.init.xavier_normal_(self.attn, gain=gain)

    _check_graph = GATConv._check_graph

    def fused(self, graph, feat, mode):
        """(out, attention in in-CSR slot order) of the fused layer kernel for `mode`."""
        self._check_graph(graph)
        res = self.res_fc if self.res_kind == Fn.RES_PROJ else None
        dst = None if self.share_weights else self.fc_dst
        return Fn.GATv2LayerFunction.apply(
            feat, self.fc_src.weight, dst.weight if dst is not None else None,
            res.weight if res is not None else None, self.fc_src.bias,
            dst.bias if dst is not None else None, res.bias if res is not None else None, self.attn,
            graph, self._num_heads, self._out_feats, self.negative_slope, mode, self.res_kind)

    def forward(self, graph, feat, get_attention=False):
        rst, a = self.fused(graph, feat, Fn.MODE_FLATTEN)
        rst = rst.view(-1, self._num_heads, self._out_feats)
        if self.activation is not None:
            rst = self.activation(rst)
        if not get_attention:
            return rst
        # slot order -> edge-id order: slot k of the in-CSR holds edge in_eid[k]
        att = torch.empty_like(a)
        att[graph.in_eid.long()] = a.detach()
        return rst, att.unsqueeze(-1)


class GATv2Layer(nn.Module):
    """dgllife.model.gnn.gatv2.GATv2Layer (0.3.0): gatv2_conv (its activation applied per head)
    -> flatten(1) | mean(1); (flatten, ELU), (flatten, None) and (mean, None) are one kernel, any
    other activation runs the flatten kernel followed by torch ops."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2,
                 residual=True, activation=None, allow_zero_in_degree=False, bias=True,
                 share_weights=False, agg_mode="flatten"):
        super().__init__()
        self.gatv2_conv = GATv2Conv(in_feats, out_feats, num_heads, feat_drop, attn_drop, negative_slope,
                                    residual, activation, allow_zero_in_degree, bias, share_weights)
        assert agg_mode in ["flatten", "mean"]
        self.agg_mode = agg_mode

    def forward(self, bg, feats):
        conv = self.gatv2_conv
        act = conv.activation
        if act is None:
            return conv.fused(bg, feats, Fn.MODE_MEAN if self.agg_mode == "mean" else Fn.MODE_FLATTEN)[0]
        if act is F.elu and self.agg_mode == "flatten":
            return conv.fused(bg, feats, Fn.MODE_FLATTEN_ELU)[0]
        rst = act(conv.fused(bg, feats, Fn.MODE_FLATTEN)[0].view(-1, conv._num_heads, conv._out_feats))
        return rst.flatten(1) if self.agg_mode == "flatten" else rst.mean(1)


class GATv2(nn.Module):
    """dgllife.model.gnn.gatv2.GATv2 (0.3.0) with GAT's defaults: 4 heads per layer, slope 0.2,
    residual, bias, 'flatten' + ELU for all but the last layer, 'mean' + no activation last;
    share_weights defaults to False per layer."""

    def __init__(self, in_feats, hidden_feats=None, num_heads=None, feat_drops=None, attn_drops=None,
                 alphas=None, residuals=None, activations=None, allow_zero_in_degree=False, biases=None,
                 share_weights=None, agg_modes=None):
        super().__init__()
        hidden_feats = list(hidden_feats) if hidden_feats is not None else [32, 32]
        n = len(hidden_feats)
        num_heads = num_heads or [4] * n
        feat_drops = feat_drops or [0.0] * n
        attn_drops = attn_drops or [0.0] * n
        alphas = alphas or [0.2] * n
        residuals = residuals or [True] * n
        if activations is None:
            activations = [F.elu] * (n - 1) + [None]
        biases = biases or [True] * n
        share_weights = share_weights or [False] * n
        if agg_modes is None:
            agg_modes = ["flatten"] * (n - 1) + ["mean"]
        self.hidden_feats = hidden_feats
        self.num_heads = num_heads
        self.agg_modes = agg_modes
        self.gnn_layers = nn.ModuleList()
        for i in range(n):
            self.gnn_layers.append(GATv2Layer(in_feats, hidden_feats[i], num_heads[i], feat_drops[i],
                                              attn_drops[i], alphas[i], residuals[i], activations[i],
                                              allow_zero_in_degree, biases[i], share_weights[i], agg_modes[i]))
            in_feats = hidden_feats[i] * num_heads[i] if agg_modes[i] == "flatten" else hidden_feats[i]

    def reset_parameters(self):
        for layer in self.gnn_layers:
            layer.gatv2_conv.reset_parameters()

    def forward(self, g, feats):
        for gnn in self.gnn_layers:
            feats = gnn(g, feats)
        return feats


class Set2Set(nn.Module):
    """dgl.nn.pytorch.glob.Set2Set (0.9.1): lstm = nn.LSTM(2*input_dim, input_dim, n_layers)
    (the module is a parameter container; the recurrence runs on the HIP kernels)."""

    def __init__(self, input_dim, n_iters, n_layers):
        super().__init__()
        # the segment kernels' range (csrc/set2set.hip check_d): refuse here, not in forward
        if input_dim <= 0 or input_dim % 4 or input_dim > 1024:
            raise ValueError(f"Set2Set: input_dim must be a positive multiple of 4 <= 1024 (got {input_dim})")
        self.input_dim = input_dim
        self.output_dim = 2 * input_dim
        self.n_iters = n_iters
        self.n_layers = n_layers
        self.lstm = nn.LSTM(self.output_dim, self.input_dim, n_layers)
        self.reset_parameters()

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def lstm_params(self):
        out = []
        for l in range(self.n_layers):
            out += [getattr(self.lstm, f"weight_ih_l{l}"), getattr(self.lstm, f"weight_hh_l{l}"),
                    getattr(self.lstm, f"bias_ih_l{l}"), getattr(self.lstm, f"bias_hh_l{l}")]
        return out

    def forward(self, graph, feat):
        return Fn.Set2SetFunction.apply(feat, graph, self.n_iters, self.n_layers, *self.lstm_params())


class WeightAndSum(nn.Module):
    """dgllife.model.readout.WeightAndSum (0.3.0): atom_weighting = Linear(in_feats, 1) + Sigmoid,
    forward(bg, feats) = sum_nodes(atom_weighting(feats) * feats), (B, in_feats).  The module is a
    parameter container (keys atom_weighting.0.weight [1, D], atom_weighting.0.bias [1]); the
    gate, the sum and their backward run in the readout kernels (csrc/readout.hip)."""

    def __init__(self, in_feats):
        super().__init__()
        # the readout kernels' range (csrc/readout.hip check_d): refuse here, not in forward
        if in_feats <= 0 or in_feats % 4 or in_feats > 1024:
            raise ValueError(f"WeightAndSum: in_feats must be a positive multiple of 4 <= 1024 (got {in_feats})")
        self.in_feats = in_feats
        self.atom_weighting = nn.Sequential(nn.Linear(in_feats, 1), nn.Sigmoid())

    def _both(self, bg, feats):
        lin = self.atom_weighting[0]
        return Fn.WeightedSumAndMaxFunction.apply(feats, lin.weight, lin.bias, bg)

    def forward(self, bg, feats):
        # the sum half of the fused pass (the max half costs no extra read of the rows)
        return self._both(bg, feats)[:, :self.in_feats]


class WeightedSumAndMax(nn.Module):
    """dgllife.model.readout.WeightedSumAndMax (0.3.0), GATPredictor's readout:
    forward(bg, feats) = cat([weight_and_sum(bg, feats), max_nodes(feats)], 1), (B, 2 in_feats)
    — Set2Set's output width.  A column's max gradient goes to the lowest-index atom attaining
    it; a molecule without atoms reads 0 in both halves (parity with dgllife/dgl is unpinned)."""

    def __init__(self, in_feats):
        super().__init__()
        self.weight_and_sum = WeightAndSum(in_feats)

    def forward(self, bg, feats):
        return self.weight_and_sum._both(bg, feats)


class GraphNorm(nn.Module):
    """torch_geometric.nn.GraphNorm (2.2.0).  forward(x, batch=None) normalises over the whole
    input like the reference (model.py:93); ``group_offsets`` (int64[G+1], rows) evaluates many
    reference mini-batches in one launch with independent statistics."""

    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels = in_channels
        self.eps = eps
        self.weight = nn.Parameter(torch.empty(in_channels))
        self.bias = nn.Parameter(torch.empty(in_channels))
        self.mean_scale = nn.Parameter(torch.empty(in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.ones_(self.weight)
        nn.init.zeros_(self.bias)
        nn.init.ones_(self.mean_scale)

    def forward(self, x, batch=None, group_offsets=None):
        if batch is not None:
            raise NotImplementedError("GraphNorm: pass contiguous groups via group_offsets")
        if group_offsets is None:
            group_offsets = torch.tensor([0, x.shape[0]], dtype=torch.int64, device=x.device)
        return Fn.GraphNormFunction.apply(x, self.weight, self.bias, self.mean_scale,
                                          group_offsets, self.eps)


class GNNModule(nn.Module):
    """model.py:77-95 — GAT -> Set2Set -> GraphNorm -> Linear+ReLU+Dropout, on the HIP path.

    forward(graphs, atom_feats): graphs is a BatchedMolGraph already on the GPU, atom_feats
    (N, in_feats) float32 on the same device; returns (B, hidden_feats[-1]).  GraphNorm
    statistics are per ``graphs.group_offsets`` (default: the whole batch, as model.py:93).

    ``readout``: "set2set" (the reference's, the default) or "weighted_sum_max" (dgllife's
    WeightedSumAndMax, the same 2 * hidden_feats[-1] output width; num_step_set2set and
    num_layer_set2set are then unused and the state_dict has readout.weight_and_sum.* instead of
    readout.lstm.*).

    ``conv``: "gat" (the reference's dgllife GAT, the default: the modules, keys and launches are
    unchanged) or "gatv2" (dgllife's GATv2 with its defaults; keys conv.gnn_layers.{i}.gatv2_conv.*;
    fp32-accurate projection only).
    """

    READOUTS = ("set2set", "weighted_sum_max")
    CONVS = ("gat", "gatv2")

    def __init__(self, in_feats=64, hidden_feats=None, dropout=0.2, num_step_set2set=6,
                 num_layer_set2set=3, proj_dtype=None, readout="set2set", conv="gat"):
        super().__init__()
        if hidden_feats is None:
            raise TypeError("GNNModule needs hidden_feats (the reference indexes hidden_feats[-1])")
        if readout not in self.READOUTS:
            raise ValueError(f"GNNModule: readout must be one of {self.READOUTS} (got {readout!r})")
        if conv not in self.CONVS:
            raise ValueError(f"GNNModule: conv must be one of {self.CONVS} (got {conv!r})")
        hidden_feats = list(hidden_feats)
        self.conv = GAT(in_feats, hidden_feats) if conv == "gat" else GATv2(in_feats, hidden_feats)
        if readout == "set2set":
            self.readout = Set2Set(input_dim=hidden_feats[-1], n_iters=num_step_set2set,
                                   n_layers=num_layer_set2set)
        else:
            self.readout = WeightedSumAndMax(hidden_feats[-1])
        self.norm = GraphNorm(hidden_feats[-1] * 2)
        self.fc = nn.Sequential(nn.Linear(hidden_feats[-1] * 2, hidden_feats[-1]), nn.ReLU(),
                                nn.Dropout(p=dropout))
        self.set_projection_dtype(proj_dtype)

    def set_projection_dtype(self, dtype):
        """GAT projection GEMM precision: None (fp32-accurate, default) or torch.bfloat16
        (bf16 operands on MFMA, fp32 accumulate — BASELINE config 4)."""
        if dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("proj_dtype must be None, torch.float32 or torch.bfloat16")
        if isinstance(self.conv, GATv2):
            if dtype == torch.bfloat16:
                raise NotImplementedError("GNNModule: the bf16 projection is not implemented for conv='gatv2'")
            return
        if dtype == torch.bfloat16 and any(layer.gat_conv.res_kind != Fn.RES_PROJ
                                           for layer in self.conv.gnn_layers):
            raise NotImplementedError(
                "GNNModule: the bf16 projection is implemented for projected residuals only (a layer "
                "here has an identity or no residual, which is exact and not rounded through Wcat)")
        for layer in self.conv.gnn_layers:
            layer.gat_conv.proj_dtype = None if dtype == torch.float32 else dtype

    def forward(self, graphs, atom_feats):
        node_x = self.conv(graphs, atom_feats)
        graph_x = self.readout(graphs, node_x)
        out = self.norm(graph_x, group_offsets=graphs.group_offsets_rows())
        # fc = Linear -> ReLU -> Dropout (model.py:86-87): the Dropout in place on the ReLU output
        return Fn.LinearReLUFunction.apply(out, self.fc[0].weight, self.fc[0].bias, Fn.dropout_p(self.fc[2]))


class MLPPredictor(nn.Module):
    """dgllife.model.model_zoo.mlp_predictor.MLPPredictor (0.3.0; restated, parity with dgllife is
    unpinned): predict = Sequential(Dropout(dropout), Linear(in_feats, hidden_feats), ReLU(),
    BatchNorm1d(hidden_feats), Linear(hidden_feats, n_tasks)).  The torch modules are parameter
    containers only (keys predict.1.*, predict.3.* with BatchNorm1d's three buffers, predict.4.*);
    forward runs Dropout anywhere -> Linear + ReLU -> BatchNorm1d (csrc/batchnorm.hip; its
    parameters, buffers, eps, momentum and training flag read from predict[3]) -> Linear on the
    HIP kernels.  momentum=None (cumulative average) is refused.  Under data parallelism the batch
    statistics are per rank, as torch's BatchNorm1d without SyncBatchNorm."""

    def __init__(self, in_feats, hidden_feats, n_tasks, dropout=0.):
        super().__init__()
        if not 0.0 <= dropout < 1.0:
            raise ValueError("MLPPredictor: dropout probability must be in [0, 1) on the HIP path")
        self.predict = nn.Sequential(nn.Dropout(dropout), nn.Linear(in_feats, hidden_feats), nn.ReLU(),
                                     nn.BatchNorm1d(hidden_feats), nn.Linear(hidden_feats, n_tasks))

    def forward(self, feats):
        from .fusion import LinearFunction
        drop, lin1, _, bn, lin2 = self.predict
        if bn.momentum is None:
            raise ValueError("MLPPredictor: BatchNorm1d momentum=None (cumulative average) is not implemented")
        h = Fn.dropout(feats, Fn.dropout_p(drop))
        h = Fn.LinearReLUFunction.apply(h, lin1.weight, lin1.bias, 0.0)
        h = Fn.batch_norm1d(h, bn)
        return LinearFunction.apply(h, lin2.weight, lin2.bias)


def _gnn_out_feats(gnn):
    last = -1
    return gnn.hidden_feats[last] * gnn.num_heads[last] if gnn.agg_modes[last] == "flatten" else gnn.hidden_feats[last]


class GATPredictor(nn.Module):
    """dgllife.model.model_zoo.gat_predictor.GATPredictor (0.3.0; restated, parity with dgllife is
    unpinned): gnn = GAT(...) -> readout = WeightedSumAndMax(gnn_out_feats) -> predict =
    MLPPredictor(2 * gnn_out_feats, predictor_hidden_feats, n_tasks, predictor_dropout);
    gnn_out_feats = hidden_feats[-1] * num_heads[-1] when the last agg_mode is "flatten", else
    hidden_feats[-1].  The deprecated classifier_hidden_feats / classifier_dropout override the
    predictor_* pair when only they are non-default (dgllife's rule).  forward(bg, feats) returns
    (B, n_tasks) logits.  feat_drops / attn_drops > 0 stay refused by the conv constructors, and a
    readout width that is no multiple of 4 up to 1024 by WeightAndSum's."""

    def __init__(self, in_feats, hidden_feats=None, num_heads=None, feat_drops=None, attn_drops=None,
                 alphas=None, residuals=None, agg_modes=None, activations=None, biases=None,
                 classifier_hidden_feats=128, classifier_dropout=0., n_tasks=1,
                 predictor_hidden_feats=128, predictor_dropout=0.):
        super().__init__()
        if predictor_hidden_feats == 128 and classifier_hidden_feats != 128:
            predictor_hidden_feats = classifier_hidden_feats
        if predictor_dropout == 0. and classifier_dropout != 0.:
            predictor_dropout = classifier_dropout
        self.gnn = GAT(in_feats=in_feats, hidden_feats=hidden_feats, num_heads=num_heads, feat_drops=feat_drops,
                       attn_drops=attn_drops, alphas=alphas, residuals=residuals, agg_modes=agg_modes,
                       activations=activations, biases=biases)
        self.gnn_out_feats = _gnn_out_feats(self.gnn)
        self.readout = WeightedSumAndMax(self.gnn_out_feats)
        self.predict = MLPPredictor(2 * self.gnn_out_feats, predictor_hidden_feats, n_tasks, predictor_dropout)

    def forward(self, bg, feats):
        node_feats = self.gnn(bg, feats)
        return self.predict(self.readout(bg, node_feats))


class GATv2Predictor(nn.Module):
    """dgllife.model.model_zoo.gatv2_predictor.GATv2Predictor (0.3.0; restated, parity with
    dgllife is unpinned): the GATPredictor stack over GATv2, with nn.GATv2's own argument order:
    gnn = GATv2(...) -> WeightedSumAndMax(gnn_out_feats) -> MLPPredictor(2 * gnn_out_feats,
    predictor_out_feats, n_tasks, predictor_dropout)."""

    def __init__(self, in_feats, hidden_feats=None, num_heads=None, feat_drops=None, attn_drops=None,
                 alphas=None, residuals=None, activations=None, allow_zero_in_degree=False, biases=None,
                 share_weights=None, agg_modes=None, n_tasks=1, predictor_out_feats=128, predictor_dropout=0.):
        super().__init__()
        self.gnn = GATv2(in_feats=in_feats, hidden_feats=hidden_feats, num_heads=num_heads, feat_drops=feat_drops,
                         attn_drops=attn_drops, alphas=alphas, residuals=residuals, activations=activations,
                         allow_zero_in_degree=allow_zero_in_degree, biases=biases, share_weights=share_weights,
                         agg_modes=agg_modes)
        self.gnn_out_feats = _gnn_out_feats(self.gnn)
        self.readout = WeightedSumAndMax(self.gnn_out_feats)
        self.predict = MLPPredictor(2 * self.gnn_out_feats, predictor_out_feats, n_tasks, predictor_dropout)

    def forward(self, bg, feats):
        node_feats = self.gnn(bg, feats)
        return self.predict(self.readout(bg, node_feats))


def _is_relu(activation):
    return activation is F.relu or activation is torch.relu or isinstance(activation, nn.ReLU)


class GraphConv(nn.Module):
    """dgl.nn.pytorch.GraphConv (0.9.1; restated, parity with dgl is unpinned): weight
    [in_feats, out_feats] (xavier-uniform) and bias [out_feats] (zeros), registered in that order;
    forward(graph, feat) = activation(D_dst (A (D_src feat)) weight + bias) with `norm` one of
    "none", "both", "right", "left" (degrees clamped to 1), on Fn.GraphConvFunction: the neighbour
    sum in csrc/gcn_agg.hip, the product on the fp32-accurate GEMM, bias and ReLU in the last
    launch.  activation: None or ReLU (F.relu, torch.relu, nn.ReLU()), the fused epilogue; any
    other callable is refused.  weight=False, a weight passed to forward and edge weights are
    refused."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True, activation=None,
                 allow_zero_in_degree=False):
        super().__init__()
        if norm not in Fn.GCN_NORMS:
            raise ValueError(f'Invalid norm value. Must be either "none", "both", "right" or "left". But got "{norm}".')
        if not weight:
            raise NotImplementedError("GraphConv: weight=False (a weight passed to forward) is not on the HIP path")
        if activation is not None and not _is_relu(activation):
            raise ValueError("GraphConv: activation must be None or ReLU (F.relu, torch.relu, nn.ReLU()) on the HIP path")
        # the aggregation kernel's range (csrc/gcn_agg.hip mvml_gcn_agg): refuse here, not in forward
        if out_feats <= 0 or out_feats % 4 or out_feats > 2048:
            raise ValueError(f"GraphConv: out_feats must be a positive multiple of 4 <= 2048 (got {out_feats})")
        # (the sum runs on the input side only when in_feats <= out_feats: inside the range too)
        if in_feats <= 0:
            raise ValueError(f"GraphConv: in_feats must be positive (got {in_feats})")
        self._in_feats = in_feats
        self._out_feats = out_feats
        self._norm = norm
        self._allow_zero_in_degree = allow_zero_in_degree
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_feats))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self._activation = activation

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    _check_graph = GATConv._check_graph

    def forward(self, graph, feat, weight=None, edge_weight=None):
        if weight is not None:
            raise NotImplementedError("GraphConv: an external weight is not on the HIP path")
        if edge_weight is not None:
            raise NotImplementedError("GraphConv: edge weights are not on the HIP path")
        self._check_graph(graph)
        return Fn.GraphConvFunction.apply(feat, self.weight, self.bias, graph, self._norm,
                                          int(self._activation is not None))


class GCNLayer(nn.Module):
    """dgllife.model.gnn.gcn.GCNLayer (0.3.0; restated, parity with dgllife is unpinned):
    new = graph_conv(g, x) (activation inside); residual: new = new + activation(res_connection(x));
    then dropout and bn_layer.  Members in dgllife's order: graph_conv, dropout, res_connection =
    Linear(in_feats, out_feats), bn_layer = BatchNorm1d(out_feats); the torch modules are parameter
    containers, the arithmetic runs on the HIP kernels (Fn.GCNConvResidualFunction: both branches and
    their sum as one autograd node, so no framework add joins their input gradients; Fn.GraphConvFunction
    without a residual; Fn.dropout, Fn.batch_norm1d).  activation: F.relu (or torch.relu / nn.ReLU())
    or None, anything else is refused here.  Deviation: activation=None with a residual is the
    identity on the residual branch (dgllife would call None)."""

    def __init__(self, in_feats, out_feats, gnn_norm="none", activation=None, residual=True, batchnorm=True,
                 dropout=0., allow_zero_in_degree=False):
        super().__init__()
        if activation is not None and not _is_relu(activation):
            raise ValueError("GCNLayer: activation must be F.relu or None on the HIP path")
        if not 0.0 <= dropout < 1.0:
            raise ValueError("GCNLayer: dropout probability must be in [0, 1) on the HIP path")
        self.activation = activation
        self.graph_conv = GraphConv(in_feats=in_feats, out_feats=out_feats, norm=gnn_norm, activation=activation,
                                    allow_zero_in_degree=allow_zero_in_degree)
        self.dropout = nn.Dropout(dropout)
        self.residual = residual
        if residual:
            self.res_connection = nn.Linear(in_feats, out_feats)
        self.bn = batchnorm
        if batchnorm:
            self.bn_layer = nn.BatchNorm1d(out_feats)

    def reset_parameters(self):
        self.graph_conv.reset_parameters()
        if self.residual:
            self.res_connection.reset_parameters()
        if self.bn:
            self.bn_layer.reset_parameters()

    def forward(self, g, feats):
        conv = self.graph_conv
        if self.residual:
            # both branches read feats: one autograd node, so that their two input gradients are
            # summed by the HIP kernels and not by the autograd engine
            conv._check_graph(g)
            lin = self.res_connection
            new_feats = Fn.GCNConvResidualFunction.apply(feats, conv.weight, conv.bias, lin.weight, lin.bias, g,
                                                         conv._norm, int(self.activation is not None))
        else:
            new_feats = conv(g, feats)
        new_feats = Fn.dropout(new_feats, Fn.dropout_p(self.dropout))
        if self.bn:
            new_feats = Fn.batch_norm1d(new_feats, self.bn_layer)
        return new_feats


class GCN(nn.Module):
    """dgllife.model.gnn.gcn.GCN (0.3.0) with its defaults: hidden_feats [64, 64], per layer
    gnn_norm "none", activation F.relu, residual, batchnorm, dropout 0."""

    def __init__(self, in_feats, hidden_feats=None, gnn_norm=None, activation=None, residual=None,
                 batchnorm=None, dropout=None, allow_zero_in_degree=None):
        super().__init__()
        hidden_feats = list(hidden_feats) if hidden_feats is not None else [64, 64]
        n = len(hidden_feats)
        gnn_norm = gnn_norm if gnn_norm is not None else ["none"] * n
        activation = activation if activation is not None else [F.relu] * n
        residual = residual if residual is not None else [True] * n
        batchnorm = batchnorm if batchnorm is not None else [True] * n
        dropout = dropout if dropout is not None else [0.] * n
        lengths = [len(hidden_feats), len(gnn_norm), len(activation), len(residual), len(batchnorm), len(dropout)]
        assert len(set(lengths)) == 1, (
            "Expect the lengths of hidden_feats, gnn_norm, activation, residual, batchnorm and dropout to "
            f"be the same, got {lengths}")
        self.hidden_feats = hidden_feats
        self.gnn_layers = nn.ModuleList()
        for i in range(n):
            self.gnn_layers.append(GCNLayer(in_feats, hidden_feats[i], gnn_norm[i], activation[i], residual[i],
                                            batchnorm[i], dropout[i], allow_zero_in_degree=allow_zero_in_degree))
            in_feats = hidden_feats[i]

    def reset_parameters(self):
        for gnn in self.gnn_layers:
            gnn.reset_parameters()

    def forward(self, g, feats):
        for gnn in self.gnn_layers:
            feats = gnn(g, feats)
        return feats


class GCNPredictor(nn.Module):
    """dgllife.model.model_zoo.gcn_predictor.GCNPredictor (0.3.0; restated, parity with dgllife is
    unpinned): gnn = GCN(...) -> readout = WeightedSumAndMax(hidden_feats[-1]) -> predict =
    MLPPredictor(2 * hidden_feats[-1], predictor_hidden_feats, n_tasks, predictor_dropout).  The
    deprecated classifier_hidden_feats / classifier_dropout override the predictor_* pair when only
    they are non-default (GATPredictor's rule).  forward(bg, feats) returns (B, n_tasks) logits."""

    def __init__(self, in_feats, hidden_feats=None, gnn_norm=None, activation=None, residual=None,
                 batchnorm=None, dropout=None, classifier_hidden_feats=128, classifier_dropout=0., n_tasks=1,
                 predictor_hidden_feats=128, predictor_dropout=0.):
        super().__init__()
        if predictor_hidden_feats == 128 and classifier_hidden_feats != 128:
            predictor_hidden_feats = classifier_hidden_feats
        if predictor_dropout == 0. and classifier_dropout != 0.:
            predictor_dropout = classifier_dropout
        self.gnn = GCN(in_feats=in_feats, hidden_feats=hidden_feats, gnn_norm=gnn_norm, activation=activation,
                       residual=residual, batchnorm=batchnorm, dropout=dropout)
        gnn_out_feats = self.gnn.hidden_feats[-1]
        self.readout = WeightedSumAndMax(gnn_out_feats)
        self.predict = MLPPredictor(2 * gnn_out_feats, predictor_hidden_feats, n_tasks, predictor_dropout)

    def forward(self, bg, feats):
        node_feats = self.gnn(bg, feats)
        return self.predict(self.readout(bg, node_feats))


class SAGEConv(nn.Module):
    """dgl.nn.pytorch.SAGEConv (0.9.1; restated, parity with dgl is unpinned), aggregator_type
    "mean", "gcn" or "pool".  Members in dgl's order: fc_pool = Linear(in_feats, in_feats) (pool
    only), fc_self = Linear(in_feats, out_feats, bias=False) (absent for gcn), fc_neigh =
    Linear(in_feats, out_feats, bias=False), bias [out_feats] (zeros; a None buffer with
    bias=False); the three weights xavier-uniform with the ReLU gain.  forward(graph, feat) =
    activation(fc_self(h) + h_neigh + bias) (gcn: activation(h_neigh + bias)) with h =
    feat_drop(feat) read by both branches, on Fn.SAGEConvFunction: the neighbour mean / sum on
    csrc/gcn_agg.hip, the neighbour maximum and gcn's self term on csrc/sage_agg.hip, the products
    on the fp32-accurate GEMM.  An atom without in-edges has h_neigh = 0 (mean, pool) or its own
    row (gcn), as in DGL, which has no zero-in-degree check here.  activation: None or ReLU;
    "lstm", norm, edge weights and a (source, destination) feature pair are refused.  A checkpoint
    of a DGL release that keeps the bias inside fc_self (fc_self.bias, no bias) loads into bias."""

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0., bias=True, norm=None, activation=None):
        super().__init__()
        if aggregator_type == "lstm":
            raise NotImplementedError("SAGEConv: the lstm aggregator is not on the HIP path")
        if aggregator_type not in Fn.SAGE_AGGREGATORS:
            raise KeyError(f"Aggregator type {aggregator_type} not recognized.")
        if norm is not None:
            raise NotImplementedError("SAGEConv: norm is not on the HIP path")
        if activation is not None and not _is_relu(activation):
            raise ValueError("SAGEConv: activation must be None or ReLU (F.relu, torch.relu, nn.ReLU()) on the HIP path")
        if not 0.0 <= feat_drop < 1.0:
            raise ValueError("SAGEConv: feat_drop must be in [0, 1) on the HIP path")
        # the aggregation kernels' range (csrc/gcn_agg.hip, csrc/sage_agg.hip): refuse here, not in forward
        if out_feats <= 0 or out_feats % 4 or out_feats > 2048:
            raise ValueError(f"SAGEConv: out_feats must be a positive multiple of 4 <= 2048 (got {out_feats})")
        if in_feats <= 0 or (aggregator_type == "pool" and in_feats > 2048):
            raise ValueError(f"SAGEConv: in_feats must be positive (pool: <= 2048), got {in_feats}")
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._aggre_type = aggregator_type
        self._allow_zero_in_degree = True  # (no such check in DGL's SAGEConv)
        self.norm = norm
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation = activation
        if aggregator_type == "pool":
            self.fc_pool = nn.Linear(in_feats, in_feats)
        if aggregator_type != "gcn":
            self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_feats))
        else:
            self.register_buffer("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if self._aggre_type == "pool":
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)
        if self._aggre_type != "gcn":
            nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        """Accept both DGL SAGEConv layouts: dgl 0.9.1 keeps an explicit ``bias`` and a bias-free
        ``fc_self``; other releases keep it inside fc_self (``fc_self.bias``, no ``bias``).  The
        arithmetic is the same, so the folded form loads into ``bias`` (GATConv's rule for
        res_fc.bias)."""
        sb, b = prefix + "fc_self.bias", prefix + "bias"
        if self._aggre_type != "gcn" and self.bias is not None and sb in state_dict and b not in state_dict:
            state_dict[b] = state_dict.pop(sb)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)

    _check_graph = GATConv._check_graph

    def forward(self, graph, feat, edge_weight=None):
        if edge_weight is not None:
            raise NotImplementedError("SAGEConv: edge weights are not on the HIP path")
        if isinstance(feat, (tuple, list)):
            raise NotImplementedError("SAGEConv: a (source, destination) feature pair is not on the HIP path")
        self._check_graph(graph)
        h = Fn.dropout(feat, Fn.dropout_p(self.feat_drop))
        pool, gcn = self._aggre_type == "pool", self._aggre_type == "gcn"
        return Fn.SAGEConvFunction.apply(h, self.fc_pool.weight if pool else None, self.fc_pool.bias if pool else None,
                                         None if gcn else self.fc_self.weight, self.fc_neigh.weight, self.bias, graph,
                                         self._aggre_type, int(self.activation is not None))


class GraphSAGE(nn.Module):
    """dgllife.model.gnn.graphsage.GraphSAGE (0.3.0; restated, parity with dgllife is unpinned)
    with its defaults: hidden_feats [64, 64], per layer activation F.relu, dropout 0 and
    aggregator_type "mean"; gnn_layers a ModuleList of SAGEConv(in, hidden, aggregator, dropout,
    activation=activation)."""

    def __init__(self, in_feats, hidden_feats=None, activation=None, dropout=None, aggregator_type=None):
        super().__init__()
        hidden_feats = list(hidden_feats) if hidden_feats is not None else [64, 64]
        n = len(hidden_feats)
        activation = activation if activation is not None else [F.relu] * n
        dropout = dropout if dropout is not None else [0.] * n
        aggregator_type = aggregator_type if aggregator_type is not None else ["mean"] * n
        lengths = [len(hidden_feats), len(activation), len(dropout), len(aggregator_type)]
        assert len(set(lengths)) == 1, (
            "Expect the lengths of hidden_feats, activation, dropout and aggregator_type to be the same, "
            f"got {lengths}")
        self.hidden_feats = hidden_feats
        self.gnn_layers = nn.ModuleList()
        for i in range(n):
            self.gnn_layers.append(SAGEConv(in_feats, hidden_feats[i], aggregator_type[i], dropout[i],
                                            activation=activation[i]))
            in_feats = hidden_feats[i]

    def reset_parameters(self):
        for gnn in self.gnn_layers:
            gnn.reset_parameters()

    def forward(self, g, feats):
        for gnn in self.gnn_layers:
            feats = gnn(g, feats)
        return feats


class GraphSAGEPredictor(nn.Module):
    """dgllife.model.model_zoo.graphsage_predictor.GraphSAGEPredictor (0.3.0; restated, parity with
    dgllife is unpinned): gnn = GraphSAGE(...) -> readout = WeightedSumAndMax(hidden_feats[-1]) ->
    predict = MLPPredictor(2 * hidden_feats[-1], predictor_hidden_feats, n_tasks, predictor_dropout).
    forward(bg, feats) returns (B, n_tasks) logits."""

    def __init__(self, in_feats, hidden_feats=None, activation=None, dropout=None, aggregator_type=None,
                 n_tasks=1, predictor_hidden_feats=128, predictor_dropout=0.):
        super().__init__()
        self.gnn = GraphSAGE(in_feats=in_feats, hidden_feats=hidden_feats, activation=activation, dropout=dropout,
                             aggregator_type=aggregator_type)
        gnn_out_feats = self.gnn.hidden_feats[-1]
        self.readout = WeightedSumAndMax(gnn_out_feats)
        self.predict = MLPPredictor(2 * gnn_out_feats, predictor_hidden_feats, n_tasks, predictor_dropout)

    def forward(self, bg, feats):
        node_feats = self.gnn(bg, feats)
        return self.predict(self.readout(bg, node_feats))


def _check_emb_dim(who, emb_dim):
    # the range of mvml_gin_agg_fwd / mvml_embed_sum_fwd (csrc/gin_agg.hip): refuse here, not in forward
    if not isinstance(emb_dim, int) or emb_dim <= 0 or emb_dim % 4 or emb_dim > 1024:
        raise ValueError(f"{who}: emb_dim must be a positive multiple of 4 <= 1024 on the HIP path (got {emb_dim})")


def _check_tables(who, what, sizes, max_total=None, max_each=None):
    sizes = [int(n) for n in sizes]
    if not 1 <= len(sizes) <= Fn.GIN_MAX_TABLES:
        raise ValueError(f"{who}: 1 to {Fn.GIN_MAX_TABLES} {what} embedding tables on the HIP path (got {len(sizes)})")
    if min(sizes) < 1:
        raise ValueError(f"{who}: every {what} embedding table needs at least one row (got {sizes})")
    if max_total is not None and sum(sizes) > max_total:
        raise ValueError(f"{who}: at most {max_total} rows over the {what} embedding tables (got {sum(sizes)})")
    if max_each is not None and max(sizes) > max_each:
        raise ValueError(f"{who}: at most {max_each} rows per {what} embedding table (got {sizes})")
    return sizes


class GINLayer(nn.Module):
    """dgllife.model.gnn.gin.GINLayer (0.3.0; restated, parity with dgllife is unpinned).  Members
    in dgllife's order: mlp = Sequential(Linear(D, 2D), ReLU(), Linear(2D, D)), edge_embeddings =
    ModuleList(Embedding(n, D) for n in num_edge_emb_list) (xavier-uniform), bn = BatchNorm1d(D) when
    batch_norm.  forward(g, node_feats, categorical_edge_feats): e = sum_t edge_embeddings[t](cat_t)
    per edge, h[v] = sum over in-edges (u -> v) of (node_feats[u] + e_uv), then mlp, bn and
    activation.  The torch modules are parameter containers; the arithmetic is one autograd node on
    the HIP kernels (Fn.GINLayerFunction: csrc/gin_agg.hip, the fp32-accurate GEMM,
    csrc/batchnorm.hip).  activation: None or ReLU (F.relu, torch.relu, nn.ReLU()).  Refused at
    construction: emb_dim no positive multiple of 4 or above 1024, more than 4 edge tables, more
    than 256 rows over them."""

    def __init__(self, num_edge_emb_list, emb_dim, batch_norm=True, activation=None):
        super().__init__()
        _check_emb_dim("GINLayer", emb_dim)
        sizes = _check_tables("GINLayer", "edge", num_edge_emb_list, max_total=Fn.GIN_MAX_EDGE_ROWS)
        if activation is not None and not _is_relu(activation):
            raise ValueError("GINLayer: activation must be None or ReLU (F.relu, torch.relu, nn.ReLU()) on the HIP path")
        self.mlp = nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.ReLU(), nn.Linear(2 * emb_dim, emb_dim))
        self.edge_embeddings = nn.ModuleList()
        for num_emb in sizes:
            emb_module = nn.Embedding(num_emb, emb_dim)
            nn.init.xavier_uniform_(emb_module.weight.data)
            self.edge_embeddings.append(emb_module)
        if batch_norm:
            self.bn = nn.BatchNorm1d(emb_dim)
        else:
            self.bn = None
        self.activation = activation
        self._allow_zero_in_degree = True  # (a row without in-edges sums to 0, as in DGL)

    def reset_parameters(self):
        for layer in self.mlp:
            if isinstance(layer, nn.Linear):
                layer.reset_parameters()
        for emb_module in self.edge_embeddings:
            nn.init.xavier_uniform_(emb_module.weight.data)
        if self.bn is not None:
            self.bn.reset_parameters()

    _check_graph = GATConv._check_graph

    def fused(self, g, node_feats, categorical_edge_feats, p=0.0):
        """forward with the Dropout(p) that follows a ReLU layer applied in place on its output."""
        self._check_graph(g)
        bn = self.bn
        return Fn.GINLayerFunction.apply(
            node_feats, self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight, self.mlp[2].bias,
            None if bn is None else bn.weight, None if bn is None else bn.bias, g, list(categorical_edge_feats), bn,
            int(self.activation is not None), float(p) if self.activation is not None else 0.0,
            *[e.weight for e in self.edge_embeddings])

    def forward(self, g, node_feats, categorical_edge_feats):
        return self.fused(g, node_feats, categorical_edge_feats)


class GIN(nn.Module):
    """dgllife.model.gnn.gin.GIN (0.3.0; restated, parity with dgllife is unpinned):
    node_embeddings = ModuleList(Embedding(n, D)) (xavier-uniform), gnn_layers = num_layers GINLayers
    with F.relu on all but the last.  forward(g, categorical_node_feats, categorical_edge_feats):
    h_0 = sum_t node_embeddings[t](idx_t) (Fn.EmbedSumFunction), h_{l+1} = dropout(layer_l(g, h_l,
    edge_feats)), then the jumping knowledge over [h_0, ..., h_L]: 'last', 'concat' (dim 1) or
    'sum'; 'max' is not implemented.  The Dropout after a ReLU layer runs in place inside the
    layer's node, the last layer's through Fn.dropout.  With 'concat' / 'sum' every h_l has two
    consumers; Fn.ForkFunction adds their two gradients with a HIP kernel, so the autograd engine
    adds nothing.  Refused at construction beside GINLayer's rules: num_layers < 2, dropout outside
    [0, 1), more than 4 node tables or more than 128 rows in one, a concat width above 2048."""

    def __init__(self, num_node_emb_list, num_edge_emb_list, num_layers=5, emb_dim=300, JK="last", dropout=0.5):
        super().__init__()
        if num_layers < 2:
            raise ValueError(f"Number of GNN layers must be greater than 1, got {num_layers}")
        _check_emb_dim("GIN", emb_dim)
        node_sizes = _check_tables("GIN", "node", num_node_emb_list, max_each=Fn.EMBED_MAX_ROWS)
        _check_tables("GIN", "edge", num_edge_emb_list, max_total=Fn.GIN_MAX_EDGE_ROWS)
        if not 0.0 <= dropout < 1.0:
            raise ValueError("GIN: dropout probability must be in [0, 1) on the HIP path")
        if JK == "max":
            raise NotImplementedError("GIN: JK='max' is not on the HIP path")
        if JK not in ("last", "concat", "sum"):
            raise ValueError(f"Expect argument JK to be one of 'concat', 'last', 'max' or 'sum', got {JK}")
        if JK == "concat" and (num_layers + 1) * emb_dim > 2048:
            raise ValueError(f"GIN: JK='concat' width (num_layers + 1) * emb_dim must be <= 2048 on the HIP path "
                             f"(got {(num_layers + 1) * emb_dim})")
        self.num_layers = num_layers
        self.JK = JK
        self.dropout = nn.Dropout(dropout)
        self.node_embeddings = nn.ModuleList()
        for num_emb in node_sizes:
            emb_module = nn.Embedding(num_emb, emb_dim)
            nn.init.xavier_uniform_(emb_module.weight.data)
            self.node_embeddings.append(emb_module)
        self.gnn_layers = nn.ModuleList()
        for layer in range(num_layers):
            if layer == num_layers - 1:
                self.gnn_layers.append(GINLayer(num_edge_emb_list, emb_dim))
            else:
                self.gnn_layers.append(GINLayer(num_edge_emb_list, emb_dim, activation=F.relu))

    def reset_parameters(self):
        for emb_module in self.node_embeddings:
            nn.init.xavier_uniform_(emb_module.weight.data)
        for layer in self.gnn_layers:
            layer.reset_parameters()

    def forward(self, g, categorical_node_feats, categorical_edge_feats):
        self.gnn_layers[0]._check_graph(g)
        p = Fn.dropout_p(self.dropout)
        fork = self.JK != "last"
        h = Fn.EmbedSumFunction.apply(list(categorical_node_feats), *[e.weight for e in self.node_embeddings])
        taps = []
        for layer in self.gnn_layers:
            if fork:
                h, tap = Fn.ForkFunction.apply(h)
                taps.append(tap)
            h = layer.fused(g, h, categorical_edge_feats, p)
            if layer.activation is None:
                h = Fn.dropout(h, p)
        if self.JK == "last":
            return h
        taps.append(h)
        return (Fn.JKConcatFunction if self.JK == "concat" else Fn.JKSumFunction).apply(*taps)


class GINPredictor(nn.Module):
    """dgllife.model.model_zoo.gin_predictor.GINPredictor (0.3.0; restated, parity with dgllife is
    unpinned): gnn = GIN(...) -> readout 'sum' / 'mean' / 'max' (dgl's Sum / Avg / MaxPooling per
    molecule, Fn.SegmentPoolFunction) -> predict = Linear((num_layers + 1) * D if JK == 'concat' else
    D, n_tasks).  The 'attention' and 'set2set' readouts are not implemented (dgllife's own
    'set2set' branch cannot be constructed).  forward(g, categorical_node_feats,
    categorical_edge_feats) returns (B, n_tasks)."""

    def __init__(self, num_node_emb_list, num_edge_emb_list, num_layers=5, emb_dim=300, JK="last", dropout=0.5,
                 readout="mean", n_tasks=1):
        super().__init__()
        if num_layers < 2:
            raise ValueError(f"Number of GNN layers must be greater than 1, got {num_layers}")
        if readout in ("attention", "set2set"):
            raise NotImplementedError(f"GINPredictor: readout={readout!r} is not on the HIP path")
        if readout not in Fn.POOL_MODES:
            raise ValueError(f"Expect readout to be 'sum', 'mean', 'max', 'attention' or 'set2set', got {readout}")
        self.gnn = GIN(num_node_emb_list=num_node_emb_list, num_edge_emb_list=num_edge_emb_list,
                       num_layers=num_layers, emb_dim=emb_dim, JK=JK, dropout=dropout)
        self.readout = readout
        self.predict = nn.Linear((num_layers + 1) * emb_dim if JK == "concat" else emb_dim, n_tasks)

    def forward(self, g, categorical_node_feats, categorical_edge_feats):
        node_feats = self.gnn(g, categorical_node_feats, categorical_edge_feats)
        graph_feats = Fn.SegmentPoolFunction.apply(node_feats, g, self.readout)
        from .fusion import LinearFunction
        return LinearFunction.apply(graph_feats, self.predict.weight, self.predict.bias)
