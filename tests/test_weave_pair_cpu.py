"""Weave's pair-update layers without a GPU: state_dict layout, exports, the constructors' refusals, the
refusals of mvml_weave_* (csrc/weave_pair.hip) before any launch, and a closed form of the reference."""
import ctypes

import pytest
import torch
import torch.nn as nn

import _weave_pair_ref as R
import mvml_gat
from mvml_gat import WeaveGNN, WeaveLayer, WeavePredictor, _lib

INVALID = 1
P = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before a launch
ENTRIES = ("mvml_weave_image_bytes", "mvml_weave_split_w", "mvml_weave_edge_fwd", "mvml_weave_edge_bwd",
           "mvml_weave_e2n_workspace_size", "mvml_weave_e2n_fwd", "mvml_weave_e2n_bwd", "mvml_weave_permute_rows")


def test_state_dict_and_exports():
    want = {}
    for i, (dn, de) in enumerate([(27, 12), (50, 50)]):
        shapes = {"node_to_node": (50, dn), "edge_to_node": (50, de), "update_node": (50, 100), "left_node_to_edge": (50, dn),
                  "right_node_to_edge": (50, dn), "edge_to_edge": (50, de), "update_edge": (50, 100)}
        assert tuple(shapes) == R.LINEARS
        for name, s in shapes.items():
            want[f"gnn.gnn_layers.{i}.{name}.weight"], want[f"gnn.gnn_layers.{i}.{name}.bias"] = s, s[:1]
    want.update({"node_to_graph.0.weight": (128, 50), "node_to_graph.0.bias": (128,), "node_to_graph.2.weight": (128,),
                 "node_to_graph.2.bias": (128,), "node_to_graph.2.running_mean": (128,), "node_to_graph.2.running_var": (128,),
                 "node_to_graph.2.num_batches_tracked": (), "readout.to_out.weight": (128, 11 * 128),
                 "readout.to_out.bias": (128,), "predict.weight": (1, 128), "predict.bias": (1,)})
    want.update({f"readout.{n}.{k}": () for n in ("means", "stds") for k in range(11)})
    assert {k: tuple(v.shape) for k, v in WeavePredictor(27, 12).state_dict().items()} == want
    for name in ("WeaveLayer", "WeaveGNN", "WeavePredictor"):
        assert name in mvml_gat.__all__ and hasattr(mvml_gat, name)
    for name in ENTRIES:
        assert name in _lib.parse_header() and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("make, match", [
    (lambda: WeaveLayer(8, 4, activation=torch.tanh), "ReLU"), (lambda: WeaveGNN(8, 4, activation=nn.Tanh()), "ReLU"),
    (lambda: WeavePredictor(8, 4, gnn_activation=torch.sigmoid), "ReLU"),
    *[(lambda k=k, w=w: WeaveLayer(8, 4, **{k: w}), k) for k in mvml_gat.functional.WEAVE_WIDTHS for w in (0, 129)],
    (lambda: WeaveGNN(8, 4, hidden_feats=129), r"\[1, 128\]"), (lambda: WeaveLayer(8, 0), r"edge_in_feats must be in \[1, 32\]"),
    (lambda: WeaveLayer(8, 33), r"edge_in_feats must be in \[1, 32\]"), (lambda: WeaveGNN(8, 33), r"\[1, 32\]"),
    (lambda: WeavePredictor(8, 4, graph_feats=126), "multiple of 4"), (lambda: WeavePredictor(8, 4, graph_feats=1028), "multiple of 4"),
    (lambda: WeavePredictor(8, 4, readout_activation=nn.ReLU()), "Tanh")])
def test_constructor_refusals(make, match):
    with pytest.raises(ValueError, match=match):
        make()


@pytest.mark.parametrize("kw", [dict(De=0), dict(De=129), dict(Hee=0), dict(Hen=129), dict(Hne=0), dict(Heo=129), dict(E=-1),
                                dict(E=2 ** 31), dict(lde=10), dict(lde=4), dict(ldo=6), dict(null="image"), dict(null="e")])
def test_entry_points_refuse_before_any_launch(kw):
    L = _lib.lib()
    De, Hee, Hen, Hne, Heo = (kw.get(k, 8) for k in ("De", "Hee", "Hen", "Hne", "Heo"))
    N, E, lde, ldo = 5, kw.get("E", 7), kw.get("lde", 8), kw.get("ldo", 8)
    img = None if kw.get("null") == "image" else P
    e = None if kw.get("null") == "e" else P
    calls = {
        "weave_edge_fwd": lambda: L.mvml_weave_edge_fwd(N, E, P, P, e, lde, De, P, 16, 8, Hne, Hee, Hen, Heo, img, P, P, P, ldo, P,
                                                        16, None),
        "weave_edge_bwd": lambda: L.mvml_weave_edge_bwd(N, E, P, P, P, ldo, e, lde, P, 16, P, 16, 8, De, Hne, Hee, Hen, Heo, img,
                                                        P, ldo, P, 16, P, 8, None),
        "weave_e2n_fwd": lambda: L.mvml_weave_e2n_fwd(N, E, P, P, e, lde, De, Hee, Hen, Hne, Heo, img, P, P, ldo, P, 1 << 20, None),
        "weave_e2n_bwd": lambda: L.mvml_weave_e2n_bwd(N, E, P, e, lde, De, Hee, Hen, Hne, Heo, img, P, P, 8, P, ldo, None)}
    if "lde" not in kw and "ldo" not in kw and "E" not in kw:
        calls["weave_split_w"] = lambda: L.mvml_weave_split_w(De, Hee, Hen, Hne, Heo, P, e, P, img, None)
    for who, fn in calls.items():  # every refusal names its own entry point
        assert fn() == INVALID and L.mvml_last_error().startswith(who.encode() + b":"), (who, L.mvml_last_error())
    if {"De", "Hee", "Hen", "Hne", "Heo"} & set(kw):
        assert L.mvml_weave_image_bytes(De, Hee, Hen, Hne, Heo) == 0
    assert L.mvml_weave_image_bytes(12, 50, 50, 50, 50) % 16 == 0 < L.mvml_weave_image_bytes(1, 1, 1, 1, 1)
    assert L.mvml_weave_permute_rows(-1, 4, P, P, 4, P, 4, 1, None) == L.mvml_weave_permute_rows(3, 4, P, P, 2, P, 4, 1, None) == INVALID


def test_reference_closed_form():
    """Zero edge_to_node weights with bias b > 0, node_to_node zero, update_node the identity on the edge
    half: x'[v] = S[v] = indeg(v) * b."""
    src, dst = torch.tensor([0, 1, 2, 2, 3]), torch.tensor([1, 1, 1, 0, 0])  # atom 3 and atom 2 have no in-edge
    H, b = 3, 0.25
    sd = {f"{n}.{p}": torch.zeros(s, dtype=torch.float64) for n in R.LINEARS
          for p, s in (("weight", (H, 2 * H if n.startswith("update") else 2)), ("bias", (H,)))}
    sd["edge_to_node.bias"] += b
    sd["update_node.weight"][:, H:] = torch.eye(H, dtype=torch.float64)
    x, e = torch.randn(4, 2, dtype=torch.float64), torch.randn(5, 2, dtype=torch.float64)
    xn = R.layer(sd, "", src, dst, x, e, node_only=True)
    assert torch.equal(xn, torch.tensor([2., 3., 0., 0.], dtype=torch.float64)[:, None].expand(4, H) * b)
