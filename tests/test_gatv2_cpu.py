"""GATv2 without a GPU: known answers of the float64 reference (tests/_gatv2_ref.py), the
parameter layout and refusals of GATv2Conv / GATv2Layer / GATv2, and the conv= / graph_conv= /
--graph_conv switch, whose default builds exactly today's modules and keys."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gatv2_ref import gatv2_agg_ref
from _util import batch_of_sizes
from mvml_gat import GATv2, GATv2Conv, GATv2Layer, GNNModule, train
from mvml_gat.mvp import MVP
from oracle.graph_ref import batch_ref


def _edges(sizes, seed=3):
    sb = batch_of_sizes(sizes, seed=seed)
    b = batch_ref(sb.num_nodes, sb.src_local, sb.dst_local, sb.num_edges)
    return torch.as_tensor(np.asarray(b["src"])).long(), torch.as_tensor(np.asarray(b["dst"])).long()


def _leaves(N, H, Fo, mode, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return (0.3 * rnd(N, H * Fo), 0.3 * rnd(N, H * Fo), 0.3 * rnd(N, Fo if mode == 1 else H * Fo),
            3 * rnd(H * Fo) / Fo ** 0.5)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_zero_attention_vector_gives_uniform_attention(mode):
    src, dst = _edges([5, 1, 3])
    N, H, Fo = int(dst.max()) + 1, 2, 4
    ZL, ZR, R, _ = _leaves(N, H, Fo, mode)
    _, a = gatv2_agg_ref(src, dst, ZL, ZR, R, torch.zeros(H * Fo, dtype=torch.float64), H, Fo, mode)
    deg = torch.bincount(dst, minlength=N).double()
    want = (1.0 / deg[dst[torch.argsort(dst, stable=True)]]).unsqueeze(1).expand(-1, H)
    assert torch.allclose(a, want, rtol=0, atol=1e-15)


def test_one_atom_molecule_is_its_own_row_plus_residual():
    src, dst = _edges([1])
    assert src.tolist() == [0] and dst.tolist() == [0]
    H, Fo = 2, 4
    ZL, ZR, R, av = _leaves(1, H, Fo, 2, seed=5)
    out, a = gatv2_agg_ref(src, dst, ZL, ZR, R, av, H, Fo, 2)
    assert torch.equal(a, torch.ones(1, H, dtype=torch.float64))
    assert torch.allclose(out, ZL + R, rtol=0, atol=1e-15)
    out1, _ = gatv2_agg_ref(src, dst, ZL, ZR, R[:, :Fo], av, H, Fo, 1)
    assert torch.allclose(out1, ZL.view(1, H, Fo).mean(1) + R[:, :Fo], rtol=0, atol=1e-15)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_gradcheck(mode):
    src, dst = _edges([5, 1, 3])
    N, H, Fo = int(dst.max()) + 1, 2, 4
    leaves = [t.requires_grad_() for t in _leaves(N, H, Fo, mode, seed=7)]
    fn = lambda ZL, ZR, R, av: gatv2_agg_ref(src, dst, ZL, ZR, R, av, H, Fo, mode)[0]
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", ["proj", "identity", "none"])
def test_conv_keys_and_shapes(kind, bias, share):
    H, Fo = 4, 20
    fin = H * Fo if kind == "identity" else 74
    conv = GATv2Conv(fin, Fo, H, residual=kind != "none", bias=bias, share_weights=share)
    want = {"fc_src.weight": (H * Fo, fin), "fc_dst.weight": (H * Fo, fin), "attn": (1, H, Fo)}
    if bias:
        want.update({"fc_src.bias": (H * Fo,), "fc_dst.bias": (H * Fo,)})
    if kind == "proj":
        want["res_fc.weight"] = (H * Fo, fin)
        if bias:
            want["res_fc.bias"] = (H * Fo,)
    sd = conv.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert (conv.fc_dst is conv.fc_src) == share
    if share:
        assert sd["fc_dst.weight"].data_ptr() == sd["fc_src.weight"].data_ptr()
    assert isinstance(conv.res_fc, torch.nn.Identity) == (kind == "identity")
    if kind == "none":
        assert conv.res_fc is None
    assert not hasattr(conv, "attn_l") and "bias" not in sd
    if bias:
        assert all(float(sd[k].abs().max()) == 0.0 for k in sd if k.endswith(".bias"))


def test_gatv2_stack_keys_and_defaults():
    net = GATv2(74, [64, 64])
    # (a module's own parameters come before its children's: attn first, as in dgl's module)
    conv_keys = ["attn", "fc_src.weight", "fc_src.bias", "fc_dst.weight", "fc_dst.bias"]
    want = [f"gnn_layers.0.gatv2_conv.{k}" for k in conv_keys + ["res_fc.weight", "res_fc.bias"]]
    want += [f"gnn_layers.1.gatv2_conv.{k}" for k in conv_keys]  # 256 -> 4 x 64: the identity residual
    assert list(net.state_dict()) == want
    l0, l1 = net.gnn_layers
    assert (l0.agg_mode, l1.agg_mode) == ("flatten", "mean")
    assert l0.gatv2_conv.activation is F.elu and l1.gatv2_conv.activation is None
    assert l0.gatv2_conv._num_heads == 4 and l0.gatv2_conv.negative_slope == 0.2
    assert not l0.gatv2_conv.share_weights
    assert tuple(l1.gatv2_conv.fc_src.weight.shape) == (256, 256)
    # width 256 -> 4 x 64: in_feats == H F gives the identity residual
    assert isinstance(GATv2(74, [64, 64], agg_modes=["flatten", "flatten"]).gnn_layers[1].gatv2_conv.res_fc,
                      torch.nn.Identity)
    assert isinstance(GATv2Layer(74, 16, 2).gatv2_conv, GATv2Conv)


@pytest.mark.parametrize("kw,exc", [(dict(feat_drop=0.1), NotImplementedError),
                                    (dict(attn_drop=0.5), NotImplementedError)])
def test_conv_refuses_dropout(kw, exc):
    with pytest.raises(exc, match="feat_drop/attn_drop"):
        GATv2Conv(74, 16, 4, **kw)


@pytest.mark.parametrize("H,Fo", [(3, 8), (4, 6), (4, 516), (8, 260), (4, 0)])
def test_conv_refuses_shapes_outside_the_kernels_range(H, Fo):
    with pytest.raises(ValueError, match="num_heads must be 1, 2, 4 or 8"):
        GATv2Conv(74, Fo, H)


def test_gnnmodule_default_conv_is_todays_gat():
    a, b = GNNModule(74, [64, 64], 0.5), GNNModule(74, [64, 64], 0.5, conv="gat")
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
    assert any(k.startswith("conv.gnn_layers.0.gat_conv.attn_l") for k in a.state_dict())
    v2 = GNNModule(74, [64, 64], 0.5, conv="gatv2")
    assert isinstance(v2.conv, GATv2)
    rest = lambda m: [k for k in m.state_dict() if not k.startswith("conv.")]
    assert rest(v2) == rest(a)
    assert "conv.gnn_layers.1.gatv2_conv.attn" in v2.state_dict()
    with pytest.raises(ValueError, match="conv must be one of"):
        GNNModule(74, [64, 64], 0.5, conv="gatv3")
    with pytest.raises(NotImplementedError, match="bf16"):
        GNNModule(74, [64, 64], 0.5, conv="gatv2", proj_dtype=torch.bfloat16)


def test_mvp_graph_conv_switch():
    m = MVP(11, 74, [16, 32], num_heads=12, graph_conv="gatv2")
    assert isinstance(m.gnn.conv, GATv2)
    assert list(MVP(11, 74, [16, 32], num_heads=12).state_dict()) == \
        list(MVP(11, 74, [16, 32], num_heads=12, graph_conv="gat").state_dict())
    with pytest.raises(ValueError):
        MVP(11, 74, [16, 32], num_heads=12, graph_conv="other")


def test_train_parses_graph_conv():
    base = ["--data", "d.csv", "--index", "i.txt"]
    assert train.parse(base).graph_conv == "gat"
    assert "graph_conv" not in vars(train.parse(base))  # a reference command line: config.py's flags only
    assert train.parse(base + ["--graph_conv", "gatv2"]).graph_conv == "gatv2"
    with pytest.raises(SystemExit):
        train.parse(base + ["--graph_conv", "gcn"])
