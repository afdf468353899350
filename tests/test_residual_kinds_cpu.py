"""GAT layers with DGL's three residual kinds (projected / identity / none) and an optional bias,
on the CPU: construction, the state_dict key sets (dgl 0.9.1 GATConv: res_fc is a bias-free
Linear when in_feats != heads * out_feats, nn.Identity() when they are equal, a None buffer with
residual=False; bias a None buffer with bias=False) and what is still refused."""
import pytest
import torch

import mvml_gat
from mvml_gat import functional as Fn
from mvml_gat.nn import GAT, GATConv, GATLayer, GNNModule


def _kinds(model):
    return [layer.gat_conv.res_kind for layer in model.gnn_layers]


def test_default_widths_construct():
    m = GAT(74, [64, 64])  # model.py:20-21's hidden_feats; layer 2: 256 == 4 * 64
    assert _kinds(m) == [Fn.RES_PROJ, Fn.RES_IDENTITY]


def test_repeated_widths_construct():
    m = GAT(74, [192, 192, 384])  # layer 2: 768 == 4 * 192
    assert _kinds(m) == [Fn.RES_PROJ, Fn.RES_IDENTITY, Fn.RES_PROJ]


def test_no_residual_constructs():
    m = GAT(74, [48, 48], residuals=[False, False])
    assert _kinds(m) == [Fn.RES_NONE, Fn.RES_NONE]
    assert all(layer.gat_conv.res_fc is None for layer in m.gnn_layers)


def test_no_bias_constructs():
    m = GAT(74, [48, 48], biases=[False, False])
    assert all(layer.gat_conv.bias is None for layer in m.gnn_layers)
    assert _kinds(m) == [Fn.RES_PROJ, Fn.RES_IDENTITY]


def test_mvp_defaults_construct():
    """MVP with the model's own defaults (hidden_feats = [64, 64]: an identity layer 2).  The one
    argument given besides num_classes is the fusion head count: MVP's signature default of 4 is
    refused by the fusion head itself, whatever the GAT does (MVFusion takes 12 only, as the
    reference's nn.Conv2d(12, 12) does, model.py:28; tests/test_fusion_widths_cpu.py pins that
    refusal), so the defaults construct with num_heads = 12, which is what main.py passes."""
    from mvml_gat.mvp import MVP
    assert mvml_gat.MVP is MVP and "MVP" in mvml_gat.__all__
    m = MVP(11, num_heads=12)
    assert m.gnn.conv.hidden_feats == [64, 64]
    assert _kinds(m.gnn.conv) == [Fn.RES_PROJ, Fn.RES_IDENTITY]
    # with the signature's head count the fusion head refuses, no longer the GAT
    with pytest.raises(ValueError, match="fusion head"):
        MVP(11)


def _dgl_keys(prefix, residual_projects, bias):
    """dgl 0.9.1 GATConv's state_dict keys (registration order aside)."""
    keys = {"fc.weight", "attn_l", "attn_r"}
    if residual_projects:
        keys.add("res_fc.weight")
    if bias:
        keys.add("bias")
    return {prefix + k for k in keys}


@pytest.mark.parametrize("in_feats,residual,bias,projects", [
    (74, True, True, True),      # projected
    (192, True, True, False),    # identity: nn.Identity() has no parameters
    (74, False, True, False),    # none: register_buffer('res_fc', None)
    (192, False, True, False),   # (equal widths do not bring a residual back)
    (74, True, False, True),     # bias=False: register_buffer('bias', None)
    (192, True, False, False),
    (74, False, False, False),
])
def test_state_dict_keys_equal_dgl(in_feats, residual, bias, projects):
    conv = GATConv(in_feats, 48, 4, residual=residual, bias=bias)
    want = _dgl_keys("", projects, bias)
    sd = conv.state_dict()
    assert set(sd) == want
    assert {n for n, _ in conv.named_parameters()} == want
    # a dict with exactly those keys loads strictly
    gen = torch.Generator().manual_seed(0)
    new = {k: torch.randn(v.shape, generator=gen) for k, v in sd.items()}
    other = GATConv(in_feats, 48, 4, residual=residual, bias=bias)
    res = other.load_state_dict(new, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in other.state_dict().items():
        assert torch.equal(v, new[k])
    # a res_fc.* or bias key that the kind does not have is refused
    if not projects:
        with pytest.raises(RuntimeError):
            other.load_state_dict({**new, "res_fc.weight": torch.zeros(192, in_feats)}, strict=True)
    if not bias:
        with pytest.raises(RuntimeError):
            other.load_state_dict({**new, "bias": torch.zeros(192)}, strict=True)
    other.reset_parameters()  # skips what is absent


def test_stack_state_dict_keys():
    m = GAT(74, [64, 64], biases=[True, False])
    want = _dgl_keys("gnn_layers.0.gat_conv.", True, True) | _dgl_keys("gnn_layers.1.gat_conv.", False, False)
    assert set(m.state_dict()) == want
    m.reset_parameters()


def test_folded_bias_rule_projecting_only():
    """later DGL's res_fc.bias (no bias key) loads into bias for a projecting residual only."""
    conv = GATConv(74, 48, 4, residual=True)
    sd = conv.state_dict()
    sd["res_fc.bias"] = sd.pop("bias") + 1.0
    conv.load_state_dict(sd, strict=True)
    assert torch.equal(conv.bias, sd["res_fc.bias"])
    ident = GATConv(192, 48, 4, residual=True)
    sd = ident.state_dict()
    sd["res_fc.bias"] = sd.pop("bias")
    with pytest.raises(RuntimeError):
        ident.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("kw", [{"feat_drop": 0.1}, {"attn_drop": 0.1}])
def test_dropouts_still_refused(kw):
    with pytest.raises(NotImplementedError, match="feat_drop/attn_drop"):
        GATConv(74, 48, 4, residual=True, **kw)
    with pytest.raises(NotImplementedError, match="feat_drop/attn_drop"):
        GATLayer(192, 48, 4, **kw)
    lists = {k + "s": [v, 0.0] for k, v in kw.items()}
    with pytest.raises(NotImplementedError, match="feat_drop/attn_drop"):
        GAT(74, [64, 64], **lists)


def test_bf16_projection_with_identity_layer_refused():
    with pytest.raises(NotImplementedError, match="bf16"):
        GNNModule(74, [64, 64], 0.5, 6, 3, proj_dtype=torch.bfloat16)
    m = GNNModule(74, [64, 64], 0.5, 6, 3)
    with pytest.raises(NotImplementedError, match="bf16"):
        m.set_projection_dtype(torch.bfloat16)
    assert all(layer.gat_conv.proj_dtype is None for layer in m.conv.gnn_layers)
    m.set_projection_dtype(torch.float32)
    GNNModule(74, [192, 384], 0.5, 6, 3, proj_dtype=torch.bfloat16)  # projected layers: as before


def test_shape_range_still_checked():
    with pytest.raises(ValueError):
        GATConv(12, 4, 3, residual=True)  # in_feats == 3 * 4, but 3 heads are out of range
