"""GraphSAGE without a GPU: the modules' construction (signatures, state_dict layout, both
checkpoint layouts, defaults, exports, refusals), hand-derivable known answers of the reference the
GPU tests compare against (tests/_sage_ref.py) and the conditions under which the GPU tests' weight
seeds were chosen (tests/_sage_cases.py)."""
import inspect

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mvml_gat
from _gcn_ref import neighbour_sum
from _sage_ref import GraphSAGEPredictorRef, SAGEConvRef, first_argmax, neighbour_max, sage_conv_ref
from mvml_gat import GraphSAGE, GraphSAGEPredictor, SAGEConv

BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def _params(cls):
    return [(n, p.default) for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]


def test_constructor_signatures():
    E = inspect.Parameter.empty
    assert _params(SAGEConv) == [("in_feats", E), ("out_feats", E), ("aggregator_type", E), ("feat_drop", 0.),
                                 ("bias", True), ("norm", None), ("activation", None)]
    assert _params(GraphSAGE) == [("in_feats", E), ("hidden_feats", None), ("activation", None), ("dropout", None),
                                  ("aggregator_type", None)]
    assert _params(GraphSAGEPredictor) == [("in_feats", E), ("hidden_feats", None), ("activation", None),
                                           ("dropout", None), ("aggregator_type", None), ("n_tasks", 1),
                                           ("predictor_hidden_feats", 128), ("predictor_dropout", 0.)]
    assert list(inspect.signature(SAGEConv.forward).parameters) == ["self", "graph", "feat", "edge_weight"]


def test_state_dict_keys_order_and_shapes():
    # the module's own parameter (bias) comes before its children's in a state_dict, as in dgl's
    want = {"mean": ["bias", "fc_self.weight", "fc_neigh.weight"], "gcn": ["bias", "fc_neigh.weight"],
            "pool": ["bias", "fc_pool.weight", "fc_pool.bias", "fc_self.weight", "fc_neigh.weight"]}
    children = {"mean": ["feat_drop", "fc_self", "fc_neigh"], "gcn": ["feat_drop", "fc_neigh"],
                "pool": ["feat_drop", "fc_pool", "fc_self", "fc_neigh"]}
    for aggr, keys in want.items():
        conv = SAGEConv(74, 64, aggr)
        sd = conv.state_dict()
        assert list(sd) == keys
        assert [n for n, _ in conv.named_children()] == children[aggr]
        assert tuple(sd["fc_neigh.weight"].shape) == (64, 74) and tuple(sd["bias"].shape) == (64,)
        assert float(sd["bias"].abs().max()) == 0.0
        if aggr == "pool":
            assert tuple(sd["fc_pool.weight"].shape) == (74, 74) and tuple(sd["fc_pool.bias"].shape) == (74,)
        if aggr != "gcn":
            assert tuple(sd["fc_self.weight"].shape) == (64, 74) and conv.fc_self.bias is None
        nb = SAGEConv(74, 64, aggr, bias=False)
        assert list(nb.state_dict()) == keys[1:] and nb.bias is None and "bias" in nb._buffers
        SAGEConvRef(74, 64, aggr).load_state_dict(sd, strict=True)
    # xavier-uniform with the ReLU gain
    conv = SAGEConv(8, 12, "pool")
    for w, (fi, fo) in ((conv.fc_pool.weight, (8, 8)), (conv.fc_self.weight, (8, 12)), (conv.fc_neigh.weight, (8, 12))):
        bound = 2 ** 0.5 * (6.0 / (fi + fo)) ** 0.5
        assert 0.5 * bound < float(w.detach().abs().max()) <= bound
    p = GraphSAGEPredictor(74, [64, 20], aggregator_type=["mean", "pool"], n_tasks=11, predictor_hidden_feats=32)
    g = "gnn.gnn_layers."
    assert list(p.state_dict()) == (
        [g + "0.bias", g + "0.fc_self.weight", g + "0.fc_neigh.weight", g + "1.bias", g + "1.fc_pool.weight",
         g + "1.fc_pool.bias", g + "1.fc_self.weight", g + "1.fc_neigh.weight",
         "readout.weight_and_sum.atom_weighting.0.weight", "readout.weight_and_sum.atom_weighting.0.bias",
         "predict.predict.1.weight", "predict.predict.1.bias"] + ["predict.predict.3." + k for k in BN]
        + ["predict.predict.4.weight", "predict.predict.4.bias"])
    assert tuple(p.state_dict()["predict.predict.1.weight"].shape) == (32, 40)
    GraphSAGEPredictorRef(74, [64, 20], ["mean", "pool"], 32, 11).load_state_dict(p.state_dict(), strict=True)


@pytest.mark.parametrize("aggr", ["mean", "pool"])
def test_both_checkpoint_layouts_load_strictly(aggr):
    src = SAGEConv(8, 12, aggr)
    with torch.no_grad():
        src.bias.copy_(torch.arange(12.0))
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    a = SAGEConv(8, 12, aggr)
    a.load_state_dict(sd, strict=True)
    folded = {("fc_self.bias" if k == "bias" else k): v for k, v in sd.items()}
    b = SAGEConv(8, 12, aggr)
    b.load_state_dict(folded, strict=True)
    for k in sd:
        assert torch.equal(a.state_dict()[k], sd[k]) and torch.equal(b.state_dict()[k], sd[k])
    # inside a stack, under the layer's prefix
    stack = GraphSAGE(8, [12], aggregator_type=[aggr])
    stack.load_state_dict({"gnn_layers.0." + k: v for k, v in folded.items()}, strict=True)
    assert torch.equal(stack.gnn_layers[0].bias.detach(), torch.arange(12.0))
    # both at once, or the folded form where there is no bias to receive it, stay errors
    with pytest.raises(RuntimeError):
        SAGEConv(8, 12, aggr).load_state_dict({**sd, "fc_self.bias": sd["bias"]}, strict=True)
    with pytest.raises(RuntimeError):
        SAGEConv(8, 12, aggr, bias=False).load_state_dict(folded, strict=True)


def test_defaults_and_exports():
    for name in ("SAGEConv", "GraphSAGE", "GraphSAGEPredictor"):
        assert name in mvml_gat.__all__ and hasattr(mvml_gat, name)
    g = GraphSAGE(74)
    assert g.hidden_feats == [64, 64] and len(g.gnn_layers) == 2
    for layer in g.gnn_layers:
        assert isinstance(layer, SAGEConv) and layer._aggre_type == "mean" and layer.activation is F.relu
        assert layer.feat_drop.p == 0.0 and layer.bias is not None
    assert g.gnn_layers[0].fc_neigh.in_features == 74 and g.gnn_layers[1].fc_neigh.in_features == 64
    conv = SAGEConv(8, 12, "gcn", feat_drop=0.25)
    assert conv.activation is None and conv.feat_drop.p == 0.25 and not hasattr(conv, "fc_self")
    before = conv.fc_neigh.weight.detach().clone()
    g2 = GraphSAGE(8, [12, 12], dropout=[0.1, 0.2], aggregator_type=["pool", "gcn"], activation=[None, nn.ReLU()])
    assert [l.feat_drop.p for l in g2.gnn_layers] == [0.1, 0.2] and g2.gnn_layers[0].activation is None
    torch.manual_seed(1)
    conv.reset_parameters()
    assert not torch.equal(conv.fc_neigh.weight.detach(), before)
    w = g2.gnn_layers[0].fc_pool.weight.detach().clone()
    g2.reset_parameters()
    assert not torch.equal(g2.gnn_layers[0].fc_pool.weight.detach(), w)
    p = GraphSAGEPredictor(74, n_tasks=11)
    assert p.predict.predict[1].in_features == 128 and p.predict.predict[4].out_features == 11
    assert p.predict.predict[1].out_features == 128 and p.predict.predict[0].p == 0.0
    p = GraphSAGEPredictor(74, [64, 20], predictor_hidden_feats=32, predictor_dropout=0.5)
    assert p.predict.predict[1].in_features == 40 and p.predict.predict[1].out_features == 32
    assert p.predict.predict[0].p == 0.5


@pytest.mark.parametrize("out_feats", [0, 6, 2052, -4])
def test_out_feats_outside_the_kernel_range_is_refused_at_construction(out_feats):
    for make in (lambda: SAGEConv(74, out_feats, "mean"), lambda: SAGEConv(74, out_feats, "pool"),
                 lambda: GraphSAGE(74, [64, out_feats]), lambda: GraphSAGEPredictor(74, [out_feats, 64])):
        with pytest.raises(ValueError, match="out_feats"):
            make()


def test_other_refusals():
    with pytest.raises(NotImplementedError, match="lstm"):
        SAGEConv(8, 8, "lstm")
    with pytest.raises(NotImplementedError, match="lstm"):
        GraphSAGE(8, [8], aggregator_type=["lstm"])
    with pytest.raises(KeyError, match="Aggregator type sum not recognized"):
        SAGEConv(8, 8, "sum")
    with pytest.raises(NotImplementedError, match="norm"):
        SAGEConv(8, 8, "mean", norm=nn.LayerNorm(8))
    for make in (lambda: SAGEConv(8, 8, "mean", activation=F.elu), lambda: SAGEConv(8, 8, "pool", activation=torch.tanh),
                 lambda: GraphSAGE(8, [8, 8], activation=[F.relu, F.elu])):
        with pytest.raises(ValueError, match="activation"):
            make()
    SAGEConv(8, 8, "gcn", activation=F.relu), SAGEConv(8, 8, "gcn", activation=nn.ReLU()), SAGEConv(8, 8, "gcn", activation=torch.relu)
    for p in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="feat_drop"):
            SAGEConv(8, 8, "mean", feat_drop=p)
    with pytest.raises(ValueError, match="in_feats"):
        SAGEConv(2052, 8, "pool")
    with pytest.raises(ValueError, match="in_feats"):
        SAGEConv(0, 8, "mean")
    with pytest.raises(AssertionError, match="lengths"):
        GraphSAGE(8, [8, 8], aggregator_type=["mean"])
    conv = SAGEConv(8, 8, "mean")
    x = torch.zeros(3, 8)
    with pytest.raises(NotImplementedError, match="edge weights"):
        conv(None, x, edge_weight=torch.zeros(3))
    with pytest.raises(NotImplementedError, match="pair"):
        conv(None, (x, x))
    with pytest.raises(TypeError, match="BatchedMolGraph"):
        conv(None, x)
    g = mvml_gat.batch([mvml_gat.bigraph_from_bonds(3, [[0, 1], [1, 2]])])
    with pytest.raises(RuntimeError, match="GPU"):  # no CPU fallback
        conv(g, x)
    with pytest.raises(ValueError, match="WeightAndSum"):
        GraphSAGEPredictor(74, [64, 1028])


# ---- the reference's known answers: a 3-atom path 0 - 1 - 2 with self-loops -------------------
SRC = [0, 1, 1, 2, 0, 1, 2]
DST = [1, 0, 2, 1, 0, 1, 2]
X3 = torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=torch.float64)


def _identity(aggr):
    """A 2 -> 2 reference layer whose Linears are the identity, without bias."""
    r = SAGEConvRef(2, 2, aggr, bias=False).double()
    with torch.no_grad():
        for lin in (m for m in r.children() if isinstance(m, nn.Linear)):
            lin.weight.copy_(torch.eye(2))
            if lin.bias is not None:
                lin.bias.zero_()
    return r


def test_reference_path_graph_by_hand():
    x0, x1, x2 = X3
    # neighbours in in-CSR order (stable in edge id): 0: [1, 0], 1: [0, 2, 1], 2: [1, 2]
    mean = sage_conv_ref(SRC, DST, X3, _identity("mean"), "mean")
    assert torch.allclose(mean, X3 + torch.stack([(x1 + x0) / 2, (x0 + x2 + x1) / 3, (x1 + x2) / 2]), rtol=1e-14, atol=0)
    gcn = sage_conv_ref(SRC, DST, X3, _identity("gcn"), "gcn")
    assert torch.allclose(gcn, torch.stack([(x1 + x0 + x0) / 3, (x0 + x2 + x1 + x1) / 4, (x1 + x2 + x2) / 3]),
                          rtol=1e-14, atol=0)
    pool = sage_conv_ref(SRC, DST, X3, _identity("pool"), "pool")
    assert torch.equal(pool, X3 + torch.stack([x1, x2, x2]))
    # in-CSR slots: row 0 = [0, 1] (sources 1, 0), row 1 = [2, 3, 4] (0, 2, 1), row 2 = [5, 6] (1, 2)
    assert first_argmax(SRC, DST, X3).tolist() == [[0, 0], [3, 3], [6, 6]]


def test_reference_mean_is_the_gcn_reference_sum_with_norm_right():
    from _gcn_cases import features, mixed_batch
    from _gcn_ref import degree_scales
    from _util import graph_dict
    sb = mixed_batch()
    gd, X = graph_dict(sb), features(sb, 20).double()
    s, d = degree_scales(gd["src"], gd["dst"], X.shape[0], "right", torch.float64)
    want = neighbour_sum(gd["src"], gd["dst"], X, s, d)
    ref = SAGEConvRef(20, 20, "mean", bias=False).double()
    with torch.no_grad():
        ref.fc_neigh.weight.copy_(torch.eye(20))
        ref.fc_self.weight.zero_()
    assert torch.equal(ref(gd, X), want)


def test_reference_first_maximiser_ties_empty_rows_and_duplicate_edges():
    # 0 -> 2 twice (a duplicated edge), 1 -> 2; atoms 0, 1 and 3 receive nothing
    src, dst = [0, 1, 0], [2, 2, 2]
    X = torch.tensor([[5.0, 1.0], [5.0, 2.0], [0.0, 0.0], [9.0, 9.0]], dtype=torch.float64, requires_grad=True)
    out, own = neighbour_max(src, dst, X)
    assert own.tolist() == [[-1, -1], [-1, -1], [0, 1], [-1, -1]]  # the tie at 5: the first slot; the 2: slot 1
    assert out.tolist() == [[0.0, 0.0], [0.0, 0.0], [5.0, 2.0], [0.0, 0.0]]
    out.sum().backward()
    assert X.grad.tolist() == [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]]  # once, not per parallel edge
    # an argmax from outside moves the value and the gradient with it
    X2 = X.detach().clone().requires_grad_()
    out2, _ = neighbour_max(src, dst, X2, arg=torch.tensor([[-1, -1], [-1, -1], [2, 1], [-1, -1]]))
    out2.sum().backward()
    assert out2.tolist() == out.tolist() and X2.grad.tolist() == X.grad.tolist()  # slot 2 is source 0 again
    out3, _ = neighbour_max(src, dst, X.detach(), arg=torch.tensor([[-1, -1], [-1, -1], [1, 0], [-1, -1]]))
    assert out3[2].tolist() == [5.0, 1.0]


def test_reference_atom_without_in_edges():
    torch.manual_seed(0)
    for aggr in ("mean", "gcn", "pool"):
        r = SAGEConvRef(2, 4, aggr).double()
        if aggr == "pool":  # a positive row at atom 0, so that atom 1's maximum is not 0
            with torch.no_grad():
                r.fc_pool.weight.abs_()
        out = r({"src": [0], "dst": [1]}, X3)
        # atoms 0 and 2 receive nothing: fc_self alone (mean, pool), fc_neigh of the own row / 1 (gcn)
        want = (r.fc_neigh if aggr == "gcn" else r.fc_self)(X3) + r.bias
        assert torch.allclose(out[0], want[0], rtol=1e-14, atol=0) and torch.allclose(out[2], want[2], rtol=1e-14, atol=0)
        assert not torch.allclose(out[1], want[1])


@pytest.mark.parametrize("kind", ["sage", "predictor"])
def test_weight_seeds_of_the_gpu_tests_are_well_conditioned_in_the_reference(kind):
    """tests/_sage_cases.py STACK_SEEDS / ADAM_SEEDS: float32 against float64 on the CPU, the float64
    reference given the float32 one's sides and argmax stays inside check_sides' cap (it raises
    outside), and over three Adam steps the float32 reference stays within 2.5e-6 of the float64
    one, so the GPU test's bar there is the 1e-5 floor."""
    from _sage_cases import ADAM_SEEDS, STACK_SEEDS, adam_e32, reference_flips
    assert reference_flips(kind, STACK_SEEDS[kind]) <= 2 * 8
    assert adam_e32(kind, ADAM_SEEDS[kind]) < 2.5e-6
