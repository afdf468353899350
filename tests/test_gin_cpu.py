"""GIN without a GPU: the modules' construction (signatures, state_dict layout, defaults, exports,
refusals), edge data through MolGraph / batch / from_arrays, hand-derivable known answers of the
reference the GPU tests compare against (tests/_gin_ref.py) and the conditions under which the GPU
tests' weight seeds were chosen (tests/_gin_cases.py)."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mvml_gat
from _gin_ref import GINLayerRef, GINPredictorRef, GINRef, embed_sum_ref, first_owner, gin_agg_ref, segment_pool_ref
from mvml_gat import GIN, GINLayer, GINPredictor
from mvml_gat import functional as Fn

BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def _params(cls):
    return [(n, p.default) for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]


def test_constructor_signatures():
    E = inspect.Parameter.empty
    assert _params(GINLayer) == [("num_edge_emb_list", E), ("emb_dim", E), ("batch_norm", True), ("activation", None)]
    assert _params(GIN) == [("num_node_emb_list", E), ("num_edge_emb_list", E), ("num_layers", 5), ("emb_dim", 300),
                            ("JK", "last"), ("dropout", 0.5)]
    assert _params(GINPredictor) == [("num_node_emb_list", E), ("num_edge_emb_list", E), ("num_layers", 5),
                                     ("emb_dim", 300), ("JK", "last"), ("dropout", 0.5), ("readout", "mean"),
                                     ("n_tasks", 1)]
    assert list(inspect.signature(GINLayer.forward).parameters) == ["self", "g", "node_feats", "categorical_edge_feats"]
    for cls in (GIN, GINPredictor):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "g", "categorical_node_feats",
                                                                   "categorical_edge_feats"]


def _layer_keys(prefix, bn=True):
    return ([prefix + k for k in ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "edge_embeddings.0.weight",
                                  "edge_embeddings.1.weight")] + ([prefix + "bn." + k for k in BN] if bn else []))


def test_state_dict_keys_order_and_shapes():
    layer = GINLayer([6, 3], 8)
    sd = layer.state_dict()
    assert list(sd) == _layer_keys("")
    assert [n for n, _ in layer.named_children()] == ["mlp", "edge_embeddings", "bn"]
    assert tuple(sd["mlp.0.weight"].shape) == (16, 8) and tuple(sd["mlp.2.weight"].shape) == (8, 16)
    assert tuple(sd["edge_embeddings.0.weight"].shape) == (6, 8) and tuple(sd["edge_embeddings.1.weight"].shape) == (3, 8)
    assert isinstance(layer.mlp[1], nn.ReLU) and layer.activation is None
    for w, (fi, fo) in ((sd["edge_embeddings.0.weight"], (6, 8)), (sd["edge_embeddings.1.weight"], (3, 8))):
        bound = (6.0 / (fi + fo)) ** 0.5  # xavier-uniform
        assert 0.5 * bound < float(w.abs().max()) <= bound
    nobn = GINLayer([6, 3], 8, batch_norm=False)
    assert list(nobn.state_dict()) == _layer_keys("", bn=False) and nobn.bn is None
    GINLayerRef([6, 3], 8).load_state_dict(sd, strict=True)
    GINLayerRef([6, 3], 8, batch_norm=False).load_state_dict(nobn.state_dict(), strict=True)

    gin = GIN([120, 3], [6, 3], num_layers=2, emb_dim=8)
    want = ["node_embeddings.0.weight", "node_embeddings.1.weight"] + _layer_keys("gnn_layers.0.") + _layer_keys("gnn_layers.1.")
    assert list(gin.state_dict()) == want
    assert tuple(gin.state_dict()["node_embeddings.0.weight"].shape) == (120, 8)
    bound = (6.0 / (120 + 8)) ** 0.5
    assert 0.5 * bound < float(gin.node_embeddings[0].weight.detach().abs().max()) <= bound
    GINRef([120, 3], [6, 3], 2, 8).load_state_dict(gin.state_dict(), strict=True)

    for jk, width in (("last", 8), ("sum", 8), ("concat", 24)):
        p = GINPredictor([120, 3], [6, 3], num_layers=2, emb_dim=8, JK=jk, n_tasks=5)
        assert list(p.state_dict()) == ["gnn." + k for k in want] + ["predict.weight", "predict.bias"]
        assert tuple(p.state_dict()["predict.weight"].shape) == (5, width)
        GINPredictorRef([120, 3], [6, 3], 2, 8, jk, "mean", 5).load_state_dict(p.state_dict(), strict=True)


def test_defaults_and_exports():
    for name in ("GINLayer", "GIN", "GINPredictor"):
        assert name in mvml_gat.__all__ and hasattr(mvml_gat, name)
    g = GIN([120, 3], [6, 3])
    assert len(g.gnn_layers) == 5 and g.JK == "last" and g.dropout.p == 0.5 and g.num_layers == 5
    assert [l.activation is F.relu for l in g.gnn_layers] == [True] * 4 + [False] and g.gnn_layers[4].activation is None
    assert all(isinstance(l.bn, nn.BatchNorm1d) and l.mlp[0].in_features == 300 and l.mlp[0].out_features == 600
               for l in g.gnn_layers)
    p = GINPredictor([120, 3], [6, 3])
    assert p.readout == "mean" and p.predict.in_features == 300 and p.predict.out_features == 1
    assert GINPredictor([120, 3], [6, 3], JK="concat").predict.in_features == 1800
    w = g.node_embeddings[0].weight.detach().clone()
    torch.manual_seed(1)
    g.reset_parameters()
    assert not torch.equal(g.node_embeddings[0].weight.detach(), w)


def test_refusals_at_construction():
    for emb in (0, 6, 1028, -4, 302):
        for make in (lambda: GINLayer([6, 3], emb), lambda: GIN([120, 3], [6, 3], emb_dim=emb),
                     lambda: GINPredictor([120, 3], [6, 3], emb_dim=emb)):
            with pytest.raises(ValueError, match="emb_dim"):
                make()
    GIN([120, 3], [6, 3], num_layers=2, emb_dim=1024)
    with pytest.raises(ValueError, match="2048"):
        GIN([120, 3], [6, 3], num_layers=5, emb_dim=344, JK="concat")  # 6 * 344 = 2064
    GIN([120, 3], [6, 3], num_layers=3, emb_dim=512, JK="concat")  # 2048: the widest
    for n in (1, 0):
        with pytest.raises(ValueError, match="greater than 1"):
            GIN([120, 3], [6, 3], num_layers=n)
        with pytest.raises(ValueError, match="greater than 1"):
            GINPredictor([120, 3], [6, 3], num_layers=n)
    for p in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="dropout"):
            GIN([120, 3], [6, 3], dropout=p)
    with pytest.raises(ValueError, match="node embedding tables"):
        GIN([2] * 5, [6, 3])
    with pytest.raises(ValueError, match="node embedding tables"):
        GIN([], [6, 3])
    with pytest.raises(ValueError, match="128 rows per node"):
        GIN([129], [6, 3])
    with pytest.raises(ValueError, match="edge embedding tables"):
        GINLayer([2] * 5, 8)
    with pytest.raises(ValueError, match="256 rows over the edge"):
        GINLayer([200, 57], 8)
    GINLayer([200, 56], 8), GINLayer([256], 8), GIN([128] * 4, [64] * 4, num_layers=2, emb_dim=8)
    with pytest.raises(ValueError, match="at least one row"):
        GINLayer([6, 0], 8)
    with pytest.raises(NotImplementedError, match="max"):
        GIN([120, 3], [6, 3], JK="max")
    with pytest.raises(ValueError, match="JK"):
        GIN([120, 3], [6, 3], JK="mean")
    for r in ("attention", "set2set"):
        with pytest.raises(NotImplementedError, match=r):
            GINPredictor([120, 3], [6, 3], readout=r)
    with pytest.raises(ValueError, match="readout"):
        GINPredictor([120, 3], [6, 3], readout="median")
    with pytest.raises(ValueError, match="activation"):
        GINLayer([6, 3], 8, activation=F.elu)
    GINLayer([6, 3], 8, activation=nn.ReLU()), GINLayer([6, 3], 8, activation=torch.relu)


def test_refusals_in_forward_and_no_cpu_fallback():
    layer, gin, pred = GINLayer([6, 3], 8), GIN([5, 3], [6, 3], 2, 8), GINPredictor([5, 3], [6, 3], 2, 8)
    x = torch.zeros(3, 8)
    nc, ec = [torch.zeros(3, dtype=torch.long)] * 2, [torch.zeros(7, dtype=torch.long)] * 2
    with pytest.raises(TypeError, match="BatchedMolGraph"):
        layer(None, x, ec)
    with pytest.raises(TypeError, match="BatchedMolGraph"):
        gin(None, nc, ec)
    g = mvml_gat.batch([mvml_gat.bigraph_from_bonds(3, [[0, 1], [1, 2]])])
    for call in (lambda: layer(g, x, ec), lambda: gin(g, nc, ec), lambda: pred(g, nc, ec)):
        with pytest.raises(RuntimeError, match="GPU"):  # no CPU fallback
            call()


# ---- edge data through the batching layer ---------------------------------------------------------
def test_edata_is_concatenated_in_edge_order():
    a = mvml_gat.bigraph_from_bonds(3, [[0, 1], [1, 2]])  # 4 bond edges + 3 self-loops
    b = mvml_gat.MolGraph(2, [0, 1], [1, 0], ndata={"h": torch.ones(2, 4)},
                          edata={"bond_type": torch.tensor([7, 8]), "bond_direction_type": torch.tensor([1, 2])})
    a.edata = {"bond_type": torch.arange(7), "bond_direction_type": torch.zeros(7, dtype=torch.long), "only_a": torch.ones(7)}
    a.ndata = {"h": torch.zeros(3, 4)}
    bg = mvml_gat.batch([a, b])
    assert sorted(bg.edata) == ["bond_direction_type", "bond_type"]  # the keys every graph has
    assert bg.edata["bond_type"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert bg.edata["bond_direction_type"].tolist() == [0] * 7 + [1, 2]
    assert bg.ndata["h"].shape == (5, 4) and bg.num_edges() == 9
    # defaults leave today's behaviour alone
    assert mvml_gat.MolGraph(2, [0], [1]).edata == {} and mvml_gat.batch([mvml_gat.graph(([0], [1]))]).edata == {}
    assert list(inspect.signature(mvml_gat.MolGraph.__init__).parameters)[-1] == "edata"
    assert list(inspect.signature(mvml_gat.from_arrays).parameters)[-1] == "edata"
    assert list(inspect.signature(mvml_gat.BatchedMolGraph.__init__).parameters)[-1] == "edata"
    fa = mvml_gat.from_arrays([3, 2], [7, 2], bg.src_local, bg.dst_local, edata={"bond_type": np.arange(9)})
    assert fa.edata["bond_type"].tolist() == list(range(9)) and fa.ndata == {}
    assert mvml_gat.from_arrays([3, 2], [7, 2], bg.src_local, bg.dst_local).edata == {}
    assert bg.to("cpu").edata["bond_type"].tolist() == list(range(9))


# ---- the reference's known answers: a 3-atom path 0 - 1 - 2 with self-loops -------------------
SRC = [0, 1, 1, 2, 0, 1, 2]
DST = [1, 0, 2, 1, 0, 1, 2]
X3 = torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=torch.float64)
# two edge tables: bond type (2 rows) and direction (2 rows); the categories per edge id
T0 = torch.tensor([[0.5, 0.25], [-1.0, -2.0]], dtype=torch.float64)
T1 = torch.tensor([[0.0, 0.0], [1000.0, 2000.0]], dtype=torch.float64)
C0 = torch.tensor([0, 0, 1, 1, 0, 0, 0])
C1 = torch.tensor([0, 0, 0, 0, 1, 0, 0])


def test_reference_u_add_e_sum_by_hand():
    x0, x1, x2 = X3
    out = gin_agg_ref(SRC, DST, X3, [T0, T1], [C0, C1])
    # in-edges: 0: 1->0 (e1), 0->0 (e4); 1: 0->1 (e0), 2->1 (e3), 1->1 (e5); 2: 1->2 (e2), 2->2 (e6)
    want = torch.stack([(x1 + T0[0]) + (x0 + T0[0] + T1[1]), (x0 + T0[0]) + (x2 + T0[1]) + (x1 + T0[0]),
                        (x1 + T0[1]) + (x2 + T0[0])])
    assert torch.allclose(out, want, rtol=1e-14, atol=0)
    assert out.tolist() == [[1012.0, 2022.5], [111.0, 220.5], [109.5, 218.25]]
    # a destination without in-edges sums to 0; no edges at all: zeros
    lone = gin_agg_ref([0], [1], X3, [T0], [torch.tensor([0])])
    assert lone.tolist() == [[0.0, 0.0], [1.5, 2.25], [0.0, 0.0]]
    assert float(gin_agg_ref([], [], X3, [T0], [torch.zeros(0, dtype=torch.long)]).abs().max()) == 0.0
    assert embed_sum_ref([T0, T1], [torch.tensor([1, 0]), torch.tensor([1, 1])]).tolist() == [[999.0, 1998.0],
                                                                                              [1000.5, 2000.25]]


def test_reference_pools_by_hand_with_an_empty_molecule():
    X = torch.tensor([[1.0, 9.0], [3.0, 9.0], [2.0, -1.0], [5.0, 5.0]], dtype=torch.float64)
    offs = [0, 3, 3, 4]  # molecules of 3, 0 and 1 atoms
    s, _ = segment_pool_ref(offs, X, "sum")
    m, _ = segment_pool_ref(offs, X, "mean")
    mx, own = segment_pool_ref(offs, X, "max")
    assert s.tolist() == [[6.0, 17.0], [0.0, 0.0], [5.0, 5.0]]
    assert m.tolist() == [[2.0, 17.0 / 3], [0.0, 0.0], [5.0, 5.0]]
    assert mx.tolist() == [[3.0, 9.0], [0.0, 0.0], [5.0, 5.0]]
    assert own.tolist() == [[1, 0], [-1, -1], [3, 3]] and first_owner(offs, X).tolist() == own.tolist()  # the tie at 9: atom 0
    Xg = X.clone().requires_grad_()
    segment_pool_ref(offs, Xg, "max")[0].sum().backward()
    assert Xg.grad.tolist() == [[0.0, 1.0], [1.0, 0.0], [0.0, 0.0], [1.0, 1.0]]
    Xg = X.clone().requires_grad_()
    segment_pool_ref(offs, Xg, "max", torch.tensor([[1, 1], [-1, -1], [3, 3]]))[0].sum().backward()
    assert Xg.grad.tolist() == [[0.0, 0.0], [1.0, 1.0], [0.0, 0.0], [1.0, 1.0]]  # an argmax from outside moves the gradient
    Xg = X.clone().requires_grad_()
    segment_pool_ref(offs, Xg, "mean")[0].sum().backward()
    assert torch.allclose(Xg.grad, torch.tensor([[1 / 3] * 2] * 3 + [[1.0, 1.0]], dtype=torch.float64))


def test_reference_edge_table_gradient_is_the_count_weighted_sum_of_g():
    tabs = [T0.clone().requires_grad_(), T1.clone().requires_grad_()]
    G = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], dtype=torch.float64)
    gin_agg_ref(SRC, DST, X3, tabs, [C0, C1]).backward(G)
    # row 0 of table 0: edges 0, 1, 4, 5, 6 with destinations 1, 0, 0, 1, 2; row 1: edges 2, 3 (2, 1)
    assert tabs[0].grad.tolist() == [[2 * 1.0 + 2 * 2.0 + 4.0, 20.0 + 40.0 + 40.0], [4.0 + 2.0, 40.0 + 20.0]]
    # table 1: row 1 is edge 4 alone (destination 0); row 0 every other edge
    assert tabs[1].grad.tolist() == [[1.0 + 3 * 2.0 + 2 * 4.0, 10.0 + 60.0 + 80.0], [1.0, 10.0]]


def test_reference_layer_and_jumping_knowledge():
    torch.manual_seed(0)
    gd = {"src": SRC, "dst": DST, "node_offsets": [0, 3]}
    nc, ec = [torch.tensor([0, 1, 2])], [C0, C1]
    outs = {}
    for jk in ("last", "concat", "sum"):
        torch.manual_seed(0)
        r = GINRef([3], [2, 2], 2, 4, jk).double().eval()
        outs[jk] = r(gd, nc, ec)
    assert outs["last"].shape == (3, 4) and outs["concat"].shape == (3, 12) and outs["sum"].shape == (3, 4)
    assert torch.equal(outs["concat"][:, 8:], outs["last"])
    assert torch.allclose(outs["sum"], outs["concat"][:, :4] + outs["concat"][:, 4:8] + outs["concat"][:, 8:], rtol=1e-14)
    torch.manual_seed(0)
    r = GINRef([3], [2, 2], 2, 4, "concat").double().eval()
    assert torch.equal(outs["concat"][:, :4], r.node_embeddings[0].weight.detach())  # h_0: the embedding rows
    layer = r.gnn_layers[0]
    assert layer.relu and not r.gnn_layers[1].relu
    h = gin_agg_ref(SRC, DST, outs["concat"][:, :4], [e.weight for e in layer.edge_embeddings], ec)
    want = F.relu(layer.bn(layer.mlp(h)))
    assert torch.allclose(outs["concat"][:, 4:8], want.detach(), rtol=1e-13, atol=1e-15)
    # masks stand in for the Dropout draws
    m = torch.tensor([[2.0] * 4, [0.0] * 4, [2.0] * 4], dtype=torch.float64)
    dropped = r(gd, nc, ec, None, None, [m, None])
    assert torch.equal(dropped[:, 4:8], outs["concat"][:, 4:8] * m) and not torch.equal(dropped[:, 8:], outs["last"])


def test_byte_counters():
    assert Fn.gin_agg_fwd_bytes(10, 30, 8, 9) == 4 * (2 * 80 + 11 + 60 + 72)
    assert Fn.embed_sum_fwd_bytes(10, 2, 8, 9) == 4 * (20 + 72 + 80)
    assert Fn.segment_pool_bytes(3, 10, 8, "sum") == 4 * (80 + 24) + 32
    assert Fn.segment_pool_bytes(3, 10, 8, "max") == 4 * (80 + 48) + 32


@pytest.mark.parametrize("kind", ["last", "concat", "sum", "wide", "pred_sum", "pred_mean", "pred_max"])
def test_weight_seeds_of_the_gpu_tests_are_well_conditioned_in_the_reference(kind):
    """tests/_gin_cases.py STACK_SEEDS / ADAM_SEEDS: float32 against float64 on the CPU, the float64
    reference given the float32 one's sides and argmax stays inside check_sides' cap (it raises
    outside), and over three Adam steps the float32 reference stays within 2.5e-6 of the float64
    one, so the GPU test's bar there is the 1e-5 floor."""
    from _gin_cases import ADAM_SEEDS, LAYERS, STACK_SEEDS, adam_e32, reference_flips
    assert reference_flips(kind, STACK_SEEDS[kind]) <= 2 * (2 * LAYERS + 1)
    if kind in ADAM_SEEDS:
        assert adam_e32(kind, ADAM_SEEDS[kind]) < 2.5e-6
