"""GCN without a GPU: the modules' construction (state_dict layout, defaults, exports, refusals)
and hand-derivable known answers of the reference the GPU tests compare against
(tests/_gcn_ref.py)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mvml_gat
from _gcn_ref import GCNLayerRef, GCNPredictorRef, degree_scales, graph_conv_ref
from mvml_gat import GCN, GCNLayer, GCNPredictor, GraphConv

BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def _layer_keys(i):
    p = f"gnn.gnn_layers.{i}."
    return ([p + "graph_conv.weight", p + "graph_conv.bias", p + "res_connection.weight", p + "res_connection.bias"]
            + [p + "bn_layer." + k for k in BN])


def test_predictor_state_dict_order_and_shapes():
    m = GCNPredictor(74, [64, 64])
    sd = m.state_dict()
    want = (_layer_keys(0) + _layer_keys(1)
            + ["readout.weight_and_sum.atom_weighting.0.weight", "readout.weight_and_sum.atom_weighting.0.bias",
               "predict.predict.1.weight", "predict.predict.1.bias"]
            + ["predict.predict.3." + k for k in BN] + ["predict.predict.4.weight", "predict.predict.4.bias"])
    assert list(sd) == want
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes["gnn.gnn_layers.0.graph_conv.weight"] == (74, 64)  # [in, out], not a Linear's [out, in]
    assert shapes["gnn.gnn_layers.1.graph_conv.weight"] == (64, 64)
    assert shapes["gnn.gnn_layers.0.graph_conv.bias"] == (64,)
    assert shapes["gnn.gnn_layers.0.res_connection.weight"] == (64, 74)
    assert shapes["gnn.gnn_layers.0.bn_layer.running_var"] == (64,)
    assert shapes["gnn.gnn_layers.0.bn_layer.num_batches_tracked"] == ()
    assert shapes["readout.weight_and_sum.atom_weighting.0.weight"] == (1, 64)
    assert shapes["predict.predict.1.weight"] == (128, 128)
    assert shapes["predict.predict.4.weight"] == (1, 128)
    # the reference composition takes the product's state_dict as it is
    GCNPredictorRef(74, [64, 64]).load_state_dict(sd, strict=True)


def test_defaults_and_exports():
    for name in ("GraphConv", "GCNLayer", "GCN", "GCNPredictor"):
        assert name in mvml_gat.__all__ and hasattr(mvml_gat, name)
    g = GCN(74)
    assert g.hidden_feats == [64, 64] and len(g.gnn_layers) == 2
    for layer in g.gnn_layers:
        assert layer.graph_conv._norm == "none" and layer.activation is F.relu
        assert layer.residual and layer.bn and layer.dropout.p == 0.0
        assert not layer.graph_conv._allow_zero_in_degree
        assert [n for n, _ in layer.named_children()] == ["graph_conv", "dropout", "res_connection", "bn_layer"]
    conv = GraphConv(8, 12)
    assert conv._norm == "both" and conv._activation is None and tuple(conv.weight.shape) == (8, 12)
    assert [n for n, _ in conv.named_parameters()] == ["weight", "bias"]
    assert float(conv.bias.detach().abs().max()) == 0.0
    bound = (6.0 / (8 + 12)) ** 0.5  # xavier-uniform
    assert float(conv.weight.detach().abs().max()) <= bound and float(conv.weight.detach().abs().max()) > 0.5 * bound
    assert list(GraphConv(8, 12, bias=False).state_dict()) == ["weight"]
    layer = GCNLayer(8, 12)
    assert layer.graph_conv._norm == "none" and layer.activation is None
    assert list(GCNLayer(8, 12, residual=False, batchnorm=False).state_dict()) == ["graph_conv.weight",
                                                                                   "graph_conv.bias"]
    p = GCNPredictor(74, n_tasks=11)
    assert p.predict.predict[1].in_features == 128 and p.predict.predict[4].out_features == 11
    assert p.predict.predict[1].out_features == 128 and p.predict.predict[0].p == 0.0


def test_deprecated_classifier_arguments_follow_gat_predictor_rule():
    p = GCNPredictor(74, classifier_hidden_feats=32, classifier_dropout=0.25)
    assert p.predict.predict[1].out_features == 32 and p.predict.predict[0].p == 0.25
    p = GCNPredictor(74, classifier_hidden_feats=32, classifier_dropout=0.25, predictor_hidden_feats=48,
                     predictor_dropout=0.5)
    assert p.predict.predict[1].out_features == 48 and p.predict.predict[0].p == 0.5


@pytest.mark.parametrize("out_feats", [0, 6, 2052, -4])
def test_out_feats_outside_the_kernel_range_is_refused_at_construction(out_feats):
    for make in (lambda: GraphConv(74, out_feats), lambda: GCNLayer(74, out_feats),
                 lambda: GCN(74, [64, out_feats]), lambda: GCNPredictor(74, [out_feats, 64])):
        with pytest.raises(ValueError, match="out_feats"):
            make()


def test_other_refusals():
    with pytest.raises(ValueError, match="Invalid norm"):
        GraphConv(8, 8, norm="sym")
    with pytest.raises(ValueError, match="Invalid norm"):
        GCN(8, [8], gnn_norm=["mean"])
    with pytest.raises(NotImplementedError, match="weight"):
        GraphConv(8, 8, weight=False)
    for make in (lambda: GCNLayer(8, 8, activation=F.elu), lambda: GCNLayer(8, 8, activation=torch.tanh),
                 lambda: GCN(8, [8, 8], activation=[F.relu, F.elu]), lambda: GraphConv(8, 8, activation=F.elu)):
        with pytest.raises(ValueError, match="activation"):
            make()
    GCNLayer(8, 8, activation=F.relu), GCNLayer(8, 8, activation=nn.ReLU()), GCNLayer(8, 8, activation=None)
    with pytest.raises(ValueError, match="dropout"):
        GCNLayer(8, 8, dropout=1.0)
    with pytest.raises(AssertionError):
        GCN(8, [8, 8], gnn_norm=["none"])
    conv = GraphConv(8, 8)
    x = torch.zeros(3, 8)
    with pytest.raises(NotImplementedError, match="weight"):
        conv(None, x, weight=torch.zeros(8, 8))
    with pytest.raises(NotImplementedError, match="edge weights"):
        conv(None, x, edge_weight=torch.zeros(3))
    with pytest.raises(TypeError, match="BatchedMolGraph"):
        conv(None, x)
    g = mvml_gat.batch([mvml_gat.bigraph_from_bonds(3, [[0, 1], [1, 2]])])
    with pytest.raises(RuntimeError, match="GPU"):  # no CPU fallback
        conv(g, x)
    # a readout width outside WeightAndSum's range is WeightAndSum's refusal
    with pytest.raises(ValueError, match="WeightAndSum"):
        GCNPredictor(74, [64, 1028])


# ---- the reference's known answers: a 3-atom path 0 - 1 - 2 with self-loops -------------------
SRC = [0, 1, 1, 2, 0, 1, 2]
DST = [1, 0, 2, 1, 0, 1, 2]
X3 = torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=torch.float64)


@pytest.mark.parametrize("norm", ["none", "both", "right", "left"])
def test_reference_path_graph_by_hand(norm):
    eye = torch.eye(2, dtype=torch.float64)
    got = graph_conv_ref(SRC, DST, X3, eye, None, norm)
    # in = out degrees (2, 3, 2); neighbours 0: {1, 0}, 1: {0, 2, 1}, 2: {1, 2}
    x0, x1, x2 = X3
    r2, r3 = 2 ** -0.5, 3 ** -0.5
    want = {"none": [x1 + x0, x0 + x2 + x1, x1 + x2],
            "both": [r2 * (r3 * x1 + r2 * x0), r3 * (r2 * x0 + r2 * x2 + r3 * x1), r2 * (r3 * x1 + r2 * x2)],
            "right": [(x1 + x0) / 2, (x0 + x2 + x1) / 3, (x1 + x2) / 2],
            "left": [x1 / 3 + x0 / 2, x0 / 2 + x2 / 2 + x1 / 3, x1 / 3 + x2 / 2]}[norm]
    assert torch.allclose(got, torch.stack(want), rtol=1e-14, atol=0)
    s, d = degree_scales(SRC, DST, 3, norm, torch.float64)
    if norm in ("none", "right"):
        assert torch.equal(s, torch.ones(3, dtype=torch.float64))
    if norm in ("none", "left"):
        assert torch.equal(d, torch.ones(3, dtype=torch.float64))


@pytest.mark.parametrize("relu", [False, True])
def test_reference_atom_without_in_edges_gives_act_bias(relu):
    # 0 -> 1 only: atom 0 (and the isolated atom 2) receive nothing; degrees clamp to 1
    W = torch.randn((2, 4), generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    b = torch.tensor([0.5, -0.25, 1.0, -2.0], dtype=torch.float64)
    for norm in ("none", "both", "right", "left"):
        out = graph_conv_ref([0], [1], X3, W, b, norm, relu=relu)
        want = F.relu(b) if relu else b
        assert torch.equal(out[0], want) and torch.equal(out[2], want)
        assert torch.allclose(out[1], (F.relu(X3[0] @ W + b) if relu else X3[0] @ W + b), rtol=1e-14, atol=0)
        assert bool(torch.isfinite(out).all())


def test_reference_orders_agree():
    gen = torch.Generator().manual_seed(1)
    X = torch.randn((3, 8), generator=gen, dtype=torch.float64)
    b = torch.randn(12, generator=gen, dtype=torch.float64)
    for fin, fout in ((8, 12), (8, 4)):
        W = torch.randn((fin, fout), generator=gen, dtype=torch.float64)
        for norm in ("none", "both", "right", "left"):
            a = graph_conv_ref(SRC, DST, X, W, b[:fout], norm, order="project")
            c = graph_conv_ref(SRC, DST, X, W, b[:fout], norm, order="aggregate")
            auto = graph_conv_ref(SRC, DST, X, W, b[:fout], norm)
            assert (a - c).abs().max().item() <= 1e-12 * c.abs().max().item()
            assert torch.equal(auto, a if fin > fout else c)


def test_reference_layer_is_the_sum_of_its_branches():
    torch.manual_seed(2)
    layer = GCNLayerRef(2, 4, "both", relu=True).double().eval()
    g = {"src": SRC, "dst": DST}
    conv = graph_conv_ref(SRC, DST, X3, layer.graph_conv.weight, layer.graph_conv.bias, "both", relu=True)
    want = conv + F.relu(layer.res_connection(X3))
    want = (want - layer.bn_layer.running_mean) / torch.sqrt(layer.bn_layer.running_var + layer.bn_layer.eps)
    assert torch.allclose(layer(g, X3), want, rtol=1e-13, atol=1e-13)
    layer.train()
    layer(g, X3)
    assert int(layer.bn_layer.num_batches_tracked) == 1


@pytest.mark.parametrize("kind", ["gcn", "predictor"])
def test_adam_seeds_of_the_gpu_test_are_well_conditioned_in_the_reference(kind):
    """tests/_gcn_cases.py ADAM_SEEDS: the float32 reference stays within 2.5e-6 of the float64
    one over three Adam steps at the chosen weight seed (so that test's bar is the 1e-5 floor)."""
    from _gcn_cases import ADAM_SEEDS, adam_e32
    assert adam_e32(kind, ADAM_SEEDS[kind]) <= 2.5e-6
