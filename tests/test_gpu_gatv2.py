"""GATv2Conv / GATv2Layer / GATv2 and the conv="gatv2" switch on the GPU against the float64
reference (tests/_gatv2_ref.py; parity with dgl / dgllife is unpinned).

The LeakyReLU side of every (edge, head, f) is the product's own: DEBUG_CAPTURE["zlr_fwd"] holds
each layer's fp32 (ZL, ZR), and branch = ZL[src] + ZR[dst] > 0 is evaluated in fp32 on the host
(the kernels' one IEEE add).  The float64 reference projects with its own rounding, so its own
side may differ where p is within rounding of 0: wherever it does, |p64| <= 1e-5 max |p64| is
asserted, and at most 8 such entries per layer.  With the seeds used here the float32 CPU
reference disagrees with the float64 one on 0 entries in every layer case (counted on the CPU).

Bar: conftest.rel_err <= max(1e-5, 4 e32) per quantity, e32 the same reference in float32 against
its float64 run; every case prints its worst err / budget.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gatv2_ref import conv_params, gatv2_layer_ref, gatv2_ref
from _util import batch_of_sizes, graph_dict, randomize_
from conftest import rel_err
from mvml_gat import GATv2Conv, GATv2Layer, GNNModule, batch, bigraph_from_bonds
from mvml_gat import functional as Fn
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
MIXED = [25, 1, 40, 7, 23, 3, 64, 2, 5]

# name: (in_feats, H, F, residual)
LAYERS = {"projecting": (74, 4, 20, True), "identity": (80, 4, 20, True), "none-tile-gemm": (132, 2, 24, False)}
FORMS = {"flatten-elu": ("flatten", F.elu), "mean": ("mean", None), "flatten": ("flatten", None)}


def _capture(fn):
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        out = fn()
    finally:
        Fn.DEBUG_CAPTURE = None
    return out, cap


def _branch(gd, zlr, H, Fo):
    src = torch.as_tensor(np.asarray(gd["src"])).long()
    dst = torch.as_tensor(np.asarray(gd["dst"])).long()
    zl, zr = zlr[0].cpu(), zlr[1].cpu()
    return ((zl[src] + zr[dst]) > 0).view(-1, H, Fo)


def _kink_cap(p64, branch, what):
    """Entries where the float64 reference's own side differs from the product's: each within
    rounding of 0, and few."""
    diff = (p64.detach() > 0) != branch
    n = int(diff.sum())
    if n:
        assert float(p64.detach()[diff].abs().max()) <= 1e-5 * float(p64.detach().abs().max()), what
    assert n <= 8, (what, n)
    return n


def _compare(got, ref64, ref32, what):
    worst = (0.0, None)
    for k in got:
        e = rel_err(got[k], ref64[k])
        budget = max(TOL, 4 * rel_err(ref32[k], ref64[k]))
        worst = max(worst, (e / budget, k))
        assert e <= budget, (what, k, e, budget)
    print(f"{what}: worst err/budget {worst[1]}: {worst[0]:.3f}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("share", [False, True], ids=["two-fc", "shared"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_layer_against_float64(name, bias, share, form):
    Fin, H, Fo, residual = LAYERS[name]
    mode, act = FORMS[form]
    sb = batch_of_sizes(MIXED, seed=1)
    gd = graph_dict(sb)
    n = int(sb.num_nodes.sum())
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(5)
    layer = GATv2Layer(Fin, Fo, H, residual=residual, activation=act, bias=bias, share_weights=share, agg_mode=mode)
    randomize_(layer, 5)
    conv = layer.gatv2_conv
    names = [k for k, _ in conv.named_parameters()]
    X = torch.randn(n, Fin, generator=gen, dtype=torch.float64)
    p64, p32 = conv_params(conv, torch.float64), conv_params(conv, torch.float32)
    layer = layer.to(DEV)
    gdev = sb.to_graph().to(DEV)
    Xp = X.float().to(DEV).requires_grad_()
    out_p, cap = _capture(lambda: layer(gdev, Xp))
    br = _branch(gd, cap["zlr_fwd"][0], H, Fo)
    gout = torch.randn(out_p.shape, generator=gen, dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    refs = []
    what = f"GATV2 LAYER {name} bias={bias} shared={share} {form}"
    for p, dt in ((p64, torch.float64), (p32, torch.float32)):
        Xr = X.to(dt).clone().requires_grad_()
        out_r, _, pe = gatv2_layer_ref(gd["src"], gd["dst"], Xr, p, H, Fo, mode, act, branch=br, return_attention=True)
        if dt == torch.float64:
            flips = _kink_cap(pe, br, what)
        out_r.backward(gout.to(dt))
        refs.append({"forward": out_r.detach(), "dX": Xr.grad, **{k: p[k].grad for k in names}})
    got = {"forward": out_p.detach(), "dX": Xp.grad, **{k: q.grad for k, q in conv.named_parameters()}}
    assert all(v is not None for v in got.values())
    _compare(got, refs[0], refs[1], f"{what} (kink-side entries {flips})")


def test_get_attention_is_in_edge_order():
    H, Fo = 4, 20
    sb = batch_of_sizes(MIXED, seed=1)
    gd = graph_dict(sb)
    n = int(sb.num_nodes.sum())
    torch.manual_seed(2)
    conv = GATv2Conv(74, Fo, H, residual=True)
    randomize_(conv, 2)
    X = torch.randn(n, 74, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    p64, p32 = conv_params(conv, torch.float64), conv_params(conv, torch.float32)
    conv = conv.to(DEV)
    gdev = sb.to_graph().to(DEV)
    (rst, att), cap = _capture(lambda: conv(gdev, X.float().to(DEV), get_attention=True))
    assert rst.shape == (n, H, Fo) and att.shape == (gdev.num_edges(), H, 1) and not att.requires_grad
    br = _branch(gd, cap["zlr_fwd"][0], H, Fo)
    o64, a64, _ = gatv2_layer_ref(gd["src"], gd["dst"], X, p64, H, Fo, "flatten", None, branch=br, return_attention=True)
    o32, a32, _ = gatv2_layer_ref(gd["src"], gd["dst"], X.float(), p32, H, Fo, "flatten", None, branch=br,
                                  return_attention=True)
    _compare({"attention": att.squeeze(-1), "rst": rst.detach().flatten(1)}, {"attention": a64, "rst": o64},
             {"attention": a32, "rst": o32}, "GATV2 get_attention")


def test_gnnmodule_gatv2_against_float64():
    """GNNModule(74, [20, 260], 0.0, conv="gatv2"): layer 1 is 4 x 20 flatten + ELU with a projected
    residual, layer 2 is 80 -> 4 x 260 head mean (H F = 1040: the 8-slot instances); molecules of
    1 .. 130 atoms, GraphNorm groups of 3."""
    from oracle.gnn_ref import graphnorm_ref, relu_branch, set2set_ref
    hidden = [20, 260]
    sb = batch_of_sizes([1, 2, 63, 64, 65, 130, 7], seed=4)
    gd = graph_dict(sb, group_size=3)
    torch.manual_seed(3)
    model = GNNModule(74, hidden, 0.0, conv="gatv2")
    randomize_(model, 3)
    X = torch.as_tensor(sb.feats, dtype=torch.float64)

    def ref_params(dt):
        p = {}
        layers = [conv_params(l.gatv2_conv, dt) for l in model.conv.gnn_layers]
        for i, (lp, l) in enumerate(zip(layers, model.conv.gnn_layers)):
            for k, _ in l.gatv2_conv.named_parameters():
                p[f"conv.gnn_layers.{i}.gatv2_conv.{k}"] = lp[k]
        lstm = torch.nn.LSTM(2 * hidden[-1], hidden[-1], model.readout.n_layers).to(dt)
        lstm.load_state_dict({k: v.detach().cpu().to(dt) for k, v in model.readout.lstm.state_dict().items()})
        for k, v in lstm.named_parameters():
            p["readout.lstm." + k] = v
        for k in ("norm.weight", "norm.bias", "norm.mean_scale", "fc.0.weight", "fc.0.bias"):
            p[k] = dict(model.named_parameters())[k].detach().cpu().to(dt).clone().requires_grad_()
        return p, layers, lstm

    refp = {dt: ref_params(dt) for dt in (torch.float64, torch.float32)}
    assert sorted(refp[torch.float64][0]) == sorted(k for k, _ in model.named_parameters())
    model = model.to(DEV).train()
    gdev = sb.to_graph().to(DEV).set_group_size(3)
    out_p, cap = _capture(lambda: model(gdev, X.float().to(DEV)))
    brs = [_branch(gd, z, 4, f) for z, f in zip(cap["zlr_fwd"], hidden)]
    fcb = (cap["relu_out"][-1] > 0).cpu()
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    refs = []
    for dt in (torch.float64, torch.float32):
        p, layers, lstm = refp[dt]
        node = gatv2_ref(gd["src"], gd["dst"], X.to(dt), layers, hidden, branches=brs)
        gx = set2set_ref(gd["node_offsets"], node, lstm, model.readout.n_iters)
        y = graphnorm_ref(gx, p["norm.weight"], p["norm.bias"], p["norm.mean_scale"], model.norm.eps,
                          gd["group_offsets"])
        out_r = relu_branch(y @ p["fc.0.weight"].t() + p["fc.0.bias"], fcb)
        out_r.backward(gout.to(dt))
        refs.append({"forward": out_r.detach(), **{k: v.grad for k, v in p.items()}})
    got = {"forward": out_p.detach(), **{k: v.grad for k, v in model.named_parameters()}}
    assert all(v is not None for v in got.values())
    _compare(got, refs[0], refs[1], "GATV2 GNNModule [20, 260]")


def _mvp_two_steps(seed):
    from mvml_gat import FlatAdam
    from mvml_gat.mvp import MVP, train_step
    from test_gpu_mvp import _kegg_batch
    bg, _, _, smiles, fp, y = _kegg_batch()
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    model = MVP(11, 74, [64, 128], num_heads=12, graph_conv="gatv2", device=DEV).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    g = bg.to(DEV)
    batch_ = ({"smiles": smiles["smiles"].to(DEV), "seq_len": smiles["seq_len"]}, g, g.ndata["h"].to(DEV),
              fp.float().to(DEV), y.float().to(DEV))
    losses = [float(train_step(model, opt, batch_).item()) for _ in range(2)]
    return losses, [p.detach().clone() for p in model.parameters()]


def test_mvp_gatv2_trains_and_repeats_bitwise():
    la, pa = _mvp_two_steps(1)
    lb, pb = _mvp_two_steps(1)
    print(f"GATV2 MVP [64, 128]: losses {la}")
    assert all(np.isfinite(l) for l in la) and la[1] <= la[0] + 1e-3
    assert la == lb
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(pa, pb))


def test_zero_in_degree_raises_unless_allowed():
    g = batch([bigraph_from_bonds(4, [(0, 1), (1, 2)], add_self_loop=False)]).to(DEV)
    X = torch.randn(4, 74, generator=torch.Generator().manual_seed(0)).to(DEV)
    torch.manual_seed(0)
    with pytest.raises(RuntimeError, match="0-in-degree nodes"):
        GATv2Conv(74, 20, 4).to(DEV)(g, X)
    conv = GATv2Conv(74, 20, 4, residual=True, allow_zero_in_degree=True).to(DEV)
    rst = conv(g, X)
    res = conv.res_fc(X).view(4, 4, 20)
    assert torch.isfinite(rst).all()
    assert rel_err(rst[3], res[3]) <= TOL  # no in-edges: the residual alone
