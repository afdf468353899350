"""GAT layers with an identity residual, no residual or no bias through mvml_gat.nn, forward and
every gradient against float64 (oracle.gnn_ref.gat_layer_ref / gat_ref / GNNModuleRef as they are:
res_fc.weight = the H F x H F identity — exact in float64 — or zeros for no residual, bias = zeros
for no bias).

Bar: 1e-5 norm-wise, or 4 x the error of the same oracle run in fp32 on the CPU where that is
larger (tests/test_gpu_parity_configs.py's); the oracle is evaluated on the product's side of
every LeakyReLU kink (that file's _capture / _branches).  Parameters that do not exist get no
gradient: they are not parameters of the module at all.

Batches: the mixed small molecules of the shape tests, and the hub batch [150, 90], which counts
as a large batch (functional._large_batch), so it runs the flat_src / mean_src / fused-softmax
policy where the small one runs the molecule-window backward and the split softmax."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import batch_of_sizes, graph_dict, randomize_
from conftest import rel_err
from mvml_gat import functional as Fn
from mvml_gat.nn import GAT, GATLayer, GNNModule
from oracle import gnn_ref
from test_gpu_parity_configs import _branches, _capture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

BATCHES = {"small": lambda: batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1),
           "hubs": lambda: batch_of_sizes([150, 90], seed=7, hubs=True)}


def _ref_params(conv, in_feats, dtype):
    """gat_layer_ref's parameter dict for a mvml_gat GATConv of any residual kind, as leaves."""
    HF = conv._num_heads * conv._out_feats
    if conv.res_kind == Fn.RES_PROJ:
        res = conv.res_fc.weight.detach().cpu().to(dtype)
    elif conv.res_kind == Fn.RES_IDENTITY:
        assert in_feats == HF
        res = torch.eye(HF, dtype=dtype)
    else:
        res = torch.zeros((HF, in_feats), dtype=dtype)
    bias = conv.bias.detach().cpu().to(dtype) if conv.bias is not None else torch.zeros(HF, dtype=dtype)
    p = {"fc.weight": conv.fc.weight.detach().cpu().to(dtype), "res_fc.weight": res,
         "attn_l": conv.attn_l.detach().cpu().to(dtype), "attn_r": conv.attn_r.detach().cpu().to(dtype),
         "bias": bias}
    return {k: v.clone().requires_grad_() for k, v in p.items()}


def _existing(conv):
    names = ["fc.weight", "attn_l", "attn_r"]
    if conv.res_kind == Fn.RES_PROJ:
        names.append("res_fc.weight")
    if conv.bias is not None:
        names.append("bias")
    assert sorted(n for n, _ in conv.named_parameters()) == sorted(names)
    return names


def _compare(got, ref64, ref32, what):
    worst = (0.0, None)
    for k in got:
        e = rel_err(got[k], ref64[k])
        budget = TOL if k == "forward" else max(TOL, 4 * rel_err(ref32[k], ref64[k]))
        worst = max(worst, (e / budget, k))
        assert e < budget, (what, k, e, budget)
    print(f"{what}: worst err/budget {worst[1]}: {worst[0]:.3f}")


LAYERS = {
    # name: (in_feats, H, F, agg_mode, residual, bias)
    "identity-flatten-elu": (192, 4, 48, "flatten", True, True),
    "identity-mean": (256, 4, 64, "mean", True, True),
    "none-bias-flatten-elu": (74, 4, 48, "flatten", False, True),
    "none-bias-mean": (80, 4, 64, "mean", False, True),
    "projected-nobias-flatten-elu": (74, 4, 48, "flatten", True, False),
    "projected-nobias-mean": (80, 4, 64, "mean", True, False),
    "none-nobias-flatten-elu": (74, 4, 48, "flatten", False, False),
    "none-nobias-mean": (80, 4, 64, "mean", False, False),
    "identity-nobias-flatten-elu": (192, 4, 48, "flatten", True, False),
}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("name", list(LAYERS))
def test_single_layer(name, batch):
    Fin, H, Fo, mode, residual, bias = LAYERS[name]
    sb = BATCHES[batch]()
    gd = graph_dict(sb)
    n = int(sb.num_nodes.sum())
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(5)
    act = F.elu if mode == "flatten" else None
    layer = GATLayer(Fin, Fo, H, residual=residual, agg_mode=mode, activation=act, bias=bias)
    randomize_(layer, 5)
    conv = layer.gat_conv
    names = _existing(conv)
    X = torch.randn(n, Fin, generator=gen, dtype=torch.float64)
    p64, p32 = _ref_params(conv, Fin, torch.float64), _ref_params(conv, Fin, torch.float32)
    layer = layer.to(DEV)
    gdev = sb.to_graph().to(DEV)
    Xp = X.float().to(DEV).requires_grad_()
    out_p, elrs = _capture(lambda: layer(gdev, Xp))
    br = _branches(gd, elrs, H)
    gout = torch.randn(out_p.shape, generator=gen, dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    refs = []
    for p, dt in ((p64, torch.float64), (p32, torch.float32)):
        Xr = X.detach().to(dt).clone().requires_grad_()
        out_r = gnn_ref.gat_layer_ref(gd["src"], gd["dst"], Xr, p, H, Fo, mode, act, branch=br[0])
        out_r.backward(gout.to(dt))
        refs.append({"forward": out_r.detach(), "dX": Xr.grad, **{k: p[k].grad for k in names}})
    c = layer.gat_conv
    got = {"forward": out_p, "dX": Xp.grad, **{k: dict(c.named_parameters())[k].grad for k in names}}
    _compare(got, refs[0], refs[1], f"LAYER {name} {batch}")


def _stack_run(model, gdev, X):
    Xp = X.float().to(DEV).requires_grad_()
    out, elrs = _capture(lambda: model(gdev, Xp))
    return Xp, out, elrs


def _stack_grads(model, Xp, out):
    got = {"forward": out.detach(), "dX": Xp.grad}
    for i, layer in enumerate(model.gnn_layers):
        for k, p in layer.gat_conv.named_parameters():
            got[f"{i}.{k}"] = p.grad
    return got


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("hidden", [(64, 64), (48, 48, 24)], ids=["64-64", "48-48-24"])
def test_stack_with_identity_layer_elu_link_on_and_off(hidden, batch, monkeypatch):
    """GAT(74, [64, 64]): layer 2 is an identity head-mean layer; GAT(74, [48, 48, 24]): layer 2 is
    an identity flatten + ELU layer behind a flatten + ELU layer (it must not claim layer 1's ELU
    link) and in front of a projected layer (which may claim layer 2's).  With the link forced on
    and off: both within the bar of float64 and of each other; the link's consistency check
    (GATLayerFunction.backward) must not raise."""
    hidden = list(hidden)
    sb = BATCHES[batch]()
    gd = graph_dict(sb)
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(9)
    model = GAT(74, hidden)
    randomize_(model, 9)
    kinds = [l.gat_conv.res_kind for l in model.gnn_layers]
    assert kinds[1] == Fn.RES_IDENTITY and kinds[0] == Fn.RES_PROJ
    widths = [74] + [4 * h for h in hidden[:-1]]
    lp64 = [_ref_params(l.gat_conv, w, torch.float64) for l, w in zip(model.gnn_layers, widths)]
    lp32 = [_ref_params(l.gat_conv, w, torch.float32) for l, w in zip(model.gnn_layers, widths)]
    X = torch.as_tensor(sb.feats, dtype=torch.float64)
    model = model.to(DEV)
    gdev = sb.to_graph().to(DEV)
    gout = None
    results = {}
    for policy in ("on", "off"):
        monkeypatch.setattr(Fn, "ELU_LINK_POLICY", policy)
        model.zero_grad(set_to_none=True)
        Xp, out, elrs = _stack_run(model, gdev, X)
        if gout is None:
            gout = torch.randn(out.shape, generator=gen, dtype=torch.float64)
        out.backward(gout.float().to(DEV))
        torch.cuda.synchronize()
        results[policy] = (_stack_grads(model, Xp, out), elrs)
    for policy, (got, elrs) in results.items():
        br = _branches(gd, elrs)
        refs = []
        for lp, dt in ((lp64, torch.float64), (lp32, torch.float32)):
            for p in lp:
                for v in p.values():
                    v.grad = None
            Xr = X.detach().to(dt).clone().requires_grad_()
            out_r = gnn_ref.gat_ref(gd["src"], gd["dst"], Xr, lp, hidden, branches=br)
            out_r.backward(gout.to(dt))
            ref = {"forward": out_r.detach(), "dX": Xr.grad}
            for i, (layer, p) in enumerate(zip(model.gnn_layers, lp)):
                for k in _existing(layer.gat_conv):
                    ref[f"{i}.{k}"] = p[k].grad.clone()
            refs.append(ref)
        assert set(got) == set(refs[0])
        _compare(got, refs[0], refs[1], f"STACK {hidden} {batch} link={policy}")
        if policy == "off":
            on = results["on"][0]
            for k in got:
                budget = TOL if k == "forward" else max(TOL, 4 * rel_err(refs[1][k], refs[0][k]))
                assert rel_err(on[k], got[k]) < budget, ("link on vs off", k)


def test_identity_stack_backward_is_deterministic():
    """Two forward + backward passes of the identity stack: every gradient bitwise equal."""
    sb = BATCHES["small"]()
    torch.manual_seed(2)
    model = GAT(74, [64, 64]).to(DEV)
    gdev = sb.to_graph().to(DEV)
    X = torch.as_tensor(sb.feats, dtype=torch.float64)
    gout = torch.randn((int(sb.num_nodes.sum()), 64), generator=torch.Generator().manual_seed(1)).to(DEV)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        Xp, out, _ = _stack_run(model, gdev, X)
        out.backward(gout)
        torch.cuda.synchronize()
        runs.append({k: v.clone() for k, v in _stack_grads(model, Xp, out).items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), k


def test_gnn_module_default_widths():
    """GNNModule(74, [64, 64]) against GNNModuleRef with its layer-2 res_fc.weight set to the
    identity; 192 molecules in 64-molecule GraphNorm groups.  Bar of
    test_gpu_parity_configs.test_gnn_module_other_widths: 1e-5, or 4 x e32 where larger (the Set2Set
    LSTM bias gradients, which cancel under GraphNorm's mean-free upstream gradient)."""
    from mvml_gat import synth
    from oracle.gnn_ref import GNNModuleRef
    hidden = [64, 64]
    sb = synth.config3(192, seed=11)
    torch.manual_seed(4)
    prod = GNNModule(74, hidden, 0.5, 6, 3)
    randomize_(prod, 4)
    prod.eval()
    res_key = "conv.gnn_layers.1.gat_conv.res_fc.weight"
    assert res_key not in prod.state_dict()
    refs = []
    for dt in (torch.float64, torch.float32):
        ref = GNNModuleRef(74, hidden, 0.5, 6, 3).eval()
        sd = {k: v.clone() for k, v in prod.state_dict().items()}
        sd[res_key] = torch.eye(256)
        ref.load_state_dict(sd, strict=True)
        refs.append(ref.to(dt))
    gd = graph_dict(sb, group_size=64)
    X = torch.as_tensor(sb.feats, dtype=torch.float64)
    prod = prod.to(DEV)
    g = sb.to_graph(group_size=64).to(DEV)
    out_p, elrs = _capture(lambda: prod(g, g.ndata["h"]))
    br = _branches(gd, elrs)
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    torch.cuda.synchronize()
    outs = []
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        o = ref(gd, X.to(dt), branches=br)
        o.backward(gout.to(dt))
        outs.append(o.detach())
    p64, p32 = dict(refs[0].named_parameters()), dict(refs[1].named_parameters())
    got = {"forward": out_p}
    r64, r32 = {"forward": outs[0]}, {"forward": outs[1]}
    for n, p in prod.named_parameters():
        got[n], r64[n], r32[n] = p.grad, p64[n].grad, p32[n].grad
    assert res_key not in got
    _compare(got, r64, r32, "GNNModule [64, 64]")


def test_mvp_defaults_train_step():
    """One train_step of MVP with the model's defaults (in_feats 64, hidden_feats [64, 64]: an
    identity layer 2; num_heads = 12, the one count the fusion head takes — see
    tests/test_residual_kinds_cpu.py) on 64 molecules with FlatAdam: it runs, the loss is finite,
    and every parameter's gradient is finite, or absent exactly where the reference leaves it None
    (the unused LayerNorms)."""
    from mvml_gat import MVP, FlatAdam
    from mvml_gat.mvp import train_step
    from oracle.fusion_ref import MVPRef, bce_logits_ref
    from test_gpu_mvp import _kegg_batch
    bg, gd, x, smiles, fp, y = _kegg_batch()
    x64 = x[:, :64].contiguous()  # the defaults' in_feats
    torch.manual_seed(0)
    model = MVP(11, num_heads=12)
    ref = MVPRef(11, 64, (64, 64), 6, 3, 64, 128, 2, 128, 12, 0.2).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["gnn.conv.gnn_layers.1.gat_conv.res_fc.weight"] = torch.eye(256)
    ref.load_state_dict(sd, strict=True)
    bce_logits_ref(ref({"smiles": smiles["smiles"], "seq_len": smiles["seq_len"]}, gd, x64.float(), fp.float()),
                   y.float()).backward()
    none_in_ref = {n for n, p in ref.named_parameters() if p.grad is None}
    model = model.to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    g = bg.to(DEV)
    batch = ({"smiles": smiles["smiles"].to(DEV), "seq_len": smiles["seq_len"]}, g, x64.float().to(DEV),
             fp.float().to(DEV), y.float().to(DEV))
    loss = train_step(model, opt, batch)
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and loss.item() > 0
    for n, p in model.named_parameters():
        if n in none_in_ref:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert bool(torch.isfinite(p).all()), n
