"""GraphConv / GCNLayer / GCN / GCNPredictor on the GPU against the float64 reference
(tests/_gcn_ref.py; parity with dgl / dgllife is unpinned), weight-tied through
load_state_dict(strict=True), on the 170-atom `mixed` batch of tests/test_gpu_agg_shapes.py
(molecules of 25, 1, 40, 7, 23, 3, 64, 2 and 5 atoms).

Bar (the project's rule, as tests/test_gpu_predictor.py): conftest.rel_err <= max(1e-5, 4 e32) per
quantity, e32 the same reference in float32 against its float64 run.

ReLU sides are taken from the product (Fn.DEBUG_CAPTURE: "gcn_out" for GraphConv's ReLU, "relu_out"
for the residual branch's and predict.1's, "readout_argmax" for the max's ties) and given to both
references, under the condition that the float64 reference disagrees with at most 2 elements per
tensor, each with a pre-activation within 1e-6 of that tensor's largest (check_sides).  The
reference alone stays inside this: float32 against float64 on this batch, four norms x widths
[74, 64, 64], [74, 128, 20], [76, 260, 516] x two seeds, gives 0 flips and a worst e32 of 7e-7.

Two notes on what the bar means here.  A bias directly in front of a BatchNorm with no ReLU between
(activation None) has a gradient that is zero in exact arithmetic: its float64 value, its e32 and
the product's error are all rounding noise, and the bar holds trivially.  And Adam turns a
gradient element of any size into a step of about lr, so ONE element whose gradient is mostly
cancellation moves by a different amount in every arithmetic: after three steps the float32
reference itself is 7e-5 (GCN) / 1e-5 (predictor) from its float64 run at weight seed 3, against
4e-7 .. 1e-6 at most seeds.  The Adam test therefore takes weight seeds at which the reference's
own three-step e32 is below 2.5e-6, so that its bar is the 1e-5 floor: ADAM_SEEDS, decided from
the reference alone (tests/_gcn_cases.py adam_e32; tests/test_gcn_cpu.py recomputes it without a GPU).
Every other test here, the stack's forward and all its gradients included, runs at weight seed 3."""
import pytest
import torch
import torch.nn.functional as F

import numpy as np

from _gcn_cases import ADAM_SEEDS, adam_labels as _adam_labels, features as _features, mixed_batch
from _gcn_cases import perturb_bn as _perturb_bn, stack
from _gcn_ref import GCNLayerRef
from _util import graph_dict, randomize_
from conftest import rel_err
from mvml_gat import FlatAdam, GCNLayer, bce_with_logits
from mvml_gat import functional as Fn
from mvml_gat._lib import call, ptr, stream_ptr
from test_gpu_agg_shapes import GRAPHS
from test_gpu_gcn_agg import _no_loops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
NORMS = ["none", "both", "right", "left"]
# 74 -> 64: the product first (74 % 4 != 0, and 74 > 64); 64 -> 64 and 76 -> 260: the sum first
# (sub-wave / one-row aggregation); 260 -> 516: the sum first at two column slots per lane
WIDTHS = [(74, 64), (64, 64), (76, 260), (260, 516)]
BN_BUFFERS = ("running_mean", "running_var")


def _stack(kind, seed=3):
    return stack(kind, seed, DEV)


@pytest.fixture(scope="module")
def mols():
    sb = GRAPHS["mixed"]()
    assert np.array_equal(sb.src_local, mixed_batch().src_local)  # _gcn_cases restates its arguments
    return sb, graph_dict(sb), sb.to_graph().to(DEV)


def _capture(fn):
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        out = fn()
    finally:
        Fn.DEBUG_CAPTURE = None
    return out, cap


def _sides(cap, n_layers, residual=True, predict=False):
    """The product's ReLU sides in the reference's layout.  "relu_out" holds the residual
    branches' outputs in layer order, then predict.1's."""
    conv = [(t > 0).cpu() for t in cap.get("gcn_out", [])]
    relu = [(t > 0).cpu() for t in cap.get("relu_out", [])]
    assert len(conv) == n_layers and len(relu) == (n_layers if residual else 0) + int(predict)
    return {"conv": conv, "res": relu[:n_layers] if residual else [None] * n_layers,
            "predict": relu[-1] if predict else None}


def check_sides(record, sides):
    """The float64 reference's own sides differ from the given ones in at most 2 elements per
    tensor, each with a pre-activation within 1e-6 of the tensor's largest."""
    pairs = list(zip(record.get("conv", []), sides["conv"])) + list(zip(record.get("res", []), sides["res"]))
    if sides.get("predict") is not None:
        pairs.append((record["predict"], sides["predict"]))
    for pre, side in pairs:
        if side is None:
            continue
        flips = (pre > 0) != side
        assert int(flips.sum()) <= 2, int(flips.sum())
        if flips.any():
            assert float(pre[flips].abs().max()) <= 1e-6 * float(pre.abs().max())


def _compare(what, got, r64, r32):
    worst = (0.0, None, 0.0, 0.0)
    assert sorted(got) == sorted(r64)
    for k in got:
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (what, k)
        e, budget = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        worst = max(worst, (e / budget, k, e, budget))
        assert e <= budget, (what, k, e, budget)
    print(f"gcn {what}: worst err/budget {worst[1]}: {worst[2]:.2e} / {worst[3]:.2e} = {worst[0]:.3f}")


def _layer_pair(fin, fout, norm, relu=True, residual=True, batchnorm=True, dropout=0.0, seed=3, allow_zero=False):
    torch.manual_seed(seed)
    m = GCNLayer(fin, fout, norm, F.relu if relu else None, residual, batchnorm, dropout, allow_zero)
    randomize_(m, seed)
    _perturb_bn(m, seed)
    refs = []
    for dt in (torch.float64, torch.float32):
        r = GCNLayerRef(fin, fout, norm, relu, residual, batchnorm)
        r.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
        refs.append(r.to(dt))
    return m.to(DEV), refs


def _layer_case(gd, g, X, model, refs, relu, residual, batchnorm, what, mask=None):
    """Training-mode forward + every gradient, then eval mode, against both references."""
    model.train()
    Xp = X.to(DEV).requires_grad_()
    out_p, cap = _capture(lambda: model(g, Xp))
    sides = _sides(cap, 1, residual) if relu else {"conv": [None], "res": [None]}
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    sd = model.state_dict()
    bufs = ["bn_layer." + b for b in BN_BUFFERS] if batchnorm else []
    got = {"out": out_p.detach(), "dX": Xp.grad, **{k: p.grad for k, p in model.named_parameters()},
           **{k: sd[k] for k in bufs}}
    res = []
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        ref.train()
        Xr = X.to(dt).clone().requires_grad_()
        rec = {}
        out_r = ref(gd, Xr, sides["conv"][0], sides["res"][0], rec, None if mask is None else mask.to(dt))
        if dt == torch.float64:
            check_sides(rec, sides)
        out_r.backward(gout.to(dt))
        res.append({"out": out_r.detach(), "dX": Xr.grad, **{k: p.grad for k, p in ref.named_parameters()},
                    **{k: ref.state_dict()[k].clone() for k in bufs}})
    _compare(what + " train", got, res[0], res[1])
    if batchnorm:
        assert int(sd["bn_layer.num_batches_tracked"]) == 1 == int(refs[0].state_dict()["bn_layer.num_batches_tracked"])
    if mask is not None:
        return
    model.eval()
    stats = {k: model.state_dict()[k].clone() for k in bufs}
    with torch.no_grad():
        out_e, cap = _capture(lambda: model(g, Xp))
        sides = _sides(cap, 1, residual) if relu else {"conv": [None], "res": [None]}
        ev = [ref.eval()(gd, X.to(dt), sides["conv"][0], sides["res"][0])
              for ref, dt in zip(refs, (torch.float64, torch.float32))]
    for k in bufs:
        assert torch.equal(model.state_dict()[k], stats[k]), "eval mode changed a running statistic"
    if batchnorm:
        assert int(model.state_dict()["bn_layer.num_batches_tracked"]) == 1
        assert rel_err(out_e, out_p) > 1e-3  # the running statistics' output, not the batch's
    _compare(what + " eval", {"out": out_e}, {"out": ev[0]}, {"out": ev[1]})


@pytest.mark.parametrize("fin,fout", WIDTHS, ids=[f"{a}to{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("norm", NORMS)
def test_layer_against_float64(mols, norm, fin, fout):
    sb, gd, g = mols
    model, refs = _layer_pair(fin, fout, norm)
    _layer_case(gd, g, _features(sb, fin), model, refs, True, True, True, f"layer {norm} {fin}->{fout}")


@pytest.mark.parametrize("fin,fout", [(74, 64), (76, 260)], ids=["74to64", "76to260"])
@pytest.mark.parametrize("relu,residual,batchnorm", [(True, False, True), (True, True, False), (True, False, False),
                                                     (False, True, True), (False, False, False)])
def test_layer_variants_against_float64(mols, relu, residual, batchnorm, fin, fout):
    sb, gd, g = mols
    model, refs = _layer_pair(fin, fout, "both", relu, residual, batchnorm)
    _layer_case(gd, g, _features(sb, fin), model, refs, relu, residual, batchnorm,
                f"layer relu={relu} res={residual} bn={batchnorm} {fin}->{fout}")


def test_layer_dropout_parity_with_the_regenerated_mask(mols, monkeypatch):
    sb, gd, g = mols
    p, seed, fin, fout = 0.25, 123456789, 74, 64
    model, refs = _layer_pair(fin, fout, "both", dropout=p)
    monkeypatch.setattr(Fn, "dropout_seed", lambda: seed)
    ones = torch.ones((g.num_nodes(), fout), device=DEV)
    mask = torch.empty_like(ones)
    call("mvml_dropout_fwd", ones.numel(), ptr(ones), ptr(mask), p, seed, stream_ptr())
    mask = mask.cpu()
    kept = mask != 0
    assert 0.6 < float(kept.float().mean()) < 0.9 and torch.equal(mask[kept], torch.full_like(mask[kept], 1 / (1 - p)))
    _layer_case(gd, g, _features(sb, fin), model, refs, True, True, True, "layer dropout 0.25", mask=mask.double())


def test_layer_dropout_repeats_under_manual_seed_differs_from_p0_and_is_off_in_eval(mols):
    sb, gd, g = mols
    X = _features(sb, 74).to(DEV)
    base, _ = _layer_pair(74, 64, "both")
    drop, _ = _layer_pair(74, 64, "both", dropout=0.5)
    gout = torch.randn((g.num_nodes(), 64), generator=torch.Generator().manual_seed(6)).to(DEV)
    outs = []
    drop.train()
    for seed in (21, 21, 22):
        torch.manual_seed(seed)
        Xp = X.clone().requires_grad_()
        z = drop(g, Xp)
        z.backward(gout)
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(Xp.grad).all())
        outs.append((z.detach(), Xp.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])
    with torch.no_grad():
        assert rel_err(outs[0][0], base.train()(g, X)) > 1e-3
        a, _ = _layer_pair(74, 64, "both")
        b, _ = _layer_pair(74, 64, "both", dropout=0.5)
        assert torch.equal(a.eval()(g, X), b.eval()(g, X))


def test_zero_in_degree_is_refused_unless_allowed():
    bg = _no_loops()
    src, dst = bg.edges()
    gd = {"src": src.long().numpy(), "dst": dst.long().numpy()}
    g = bg.to(DEV)
    X = torch.randn((g.num_nodes(), 8), generator=torch.Generator().manual_seed(1))
    strict, _ = _layer_pair(8, 12, "both")
    with pytest.raises(RuntimeError, match="0-in-degree"):
        strict(g, X.to(DEV))
    model, refs = _layer_pair(8, 12, "both", allow_zero=True)
    _layer_case(gd, g, X, model, refs, True, True, True, "layer zero in-degree allowed")


# ---- the stack and the predictor ----------------------------------------------------------------
def _ref_forward(kind, ref, gd, X, sides, cap, rec=None):
    if kind == "gcn":
        return ref(gd, X, sides, rec)
    return ref(gd, X, sides, rec, argmax=cap["readout_argmax"][0].cpu().long())


@pytest.mark.parametrize("kind", ["gcn", "predictor"])
def test_stack_against_float64(mols, kind):
    sb, gd, g = mols
    model, refs = _stack(kind)
    model.train()
    X = _features(sb, 74)
    Xp = g.ndata["h"].detach().requires_grad_()  # the batch's resident (zero-padded) atom features
    out_p, cap = _capture(lambda: model(g, Xp))
    assert out_p.shape == ((g.num_nodes(), 64) if kind == "gcn" else (len(sb.num_nodes), 11))
    sides = _sides(cap, 2, True, kind == "predictor")
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    sd = model.state_dict()
    bufs = [k for k in sd if k.endswith(BN_BUFFERS)]
    got = {"out": out_p.detach(), "dX": Xp.grad, **{k: p.grad for k, p in model.named_parameters()},
           **{k: sd[k] for k in bufs}}
    res = []
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        ref.train()
        Xr = X.to(dt).clone().requires_grad_()
        rec = {}
        out_r = _ref_forward(kind, ref, gd, Xr, sides, cap, rec)
        if dt == torch.float64:
            check_sides(rec, sides)
        out_r.backward(gout.to(dt))
        res.append({"out": out_r.detach(), "dX": Xr.grad, **{k: p.grad for k, p in ref.named_parameters()},
                    **{k: ref.state_dict()[k].clone() for k in bufs}})
    _compare(f"{kind} train", got, res[0], res[1])
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 1 == int(refs[0].state_dict()[k])


@pytest.mark.parametrize("kind", ["gcn", "predictor"])
def test_three_adam_steps_against_float64(mols, kind):
    sb, gd, g = mols
    model, refs = _stack(kind, ADAM_SEEDS[kind])
    model.train()
    X = _features(sb, 74)
    Xd = g.ndata["h"]
    y = _adam_labels(kind, sb)
    yd = y.to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    opts = [torch.optim.Adam(r.parameters(), lr=1e-3, weight_decay=1e-4) for r in refs]
    for _ in range(3):
        opt.zero_grad()
        z, cap = _capture(lambda: model(g, Xd))
        bce_with_logits(z, yd).backward()
        opt.step()
        sides = _sides(cap, 2, True, kind == "predictor")
        for ref, o, dt in zip(refs, opts, (torch.float64, torch.float32)):
            ref.train()
            o.zero_grad()
            rec = {}
            zr = _ref_forward(kind, ref, gd, X.to(dt), sides, cap, rec)
            if dt == torch.float64:
                check_sides(rec, sides)
            F.binary_cross_entropy_with_logits(zr, y.to(dt)).backward()
            o.step()
    sd, s64, s32 = model.state_dict(), refs[0].state_dict(), refs[1].state_dict()
    keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == 3 == int(s64[k])
    _compare(f"{kind} 3 Adam steps", {k: sd[k] for k in keys}, {k: s64[k] for k in keys}, {k: s32[k] for k in keys})


@pytest.mark.parametrize("kind", ["gcn", "predictor"])
def test_checkpoint_round_trip_is_bitwise(mols, kind):
    sb, gd, g = mols
    Xd = g.ndata["h"]
    model, _ = _stack(kind)
    model.train()
    with torch.no_grad():
        model(g, Xd)  # moves the running statistics and the counters
        ckpt = {k: v.cpu().clone() for k, v in model.state_dict().items()}
        fresh, _ = _stack(kind, seed=99)
        fresh.load_state_dict(ckpt, strict=True)
        fresh.eval()
        assert all(int(v) == 1 for k, v in fresh.state_dict().items() if k.endswith("num_batches_tracked"))
        assert torch.equal(fresh(g, Xd), model.eval()(g, Xd))


@pytest.mark.parametrize("kind", ["gcn", "predictor"])
def test_no_framework_arithmetic_in_forward_or_backward(mols, kind):
    """Every layer's input feeds the conv and the residual branch; their input gradients must meet
    in the HIP kernels (Fn.GCNConvResidualFunction), not in an add of the autograd engine: no aten
    arithmetic operator runs in a training-mode forward + backward with the input's gradient on."""
    from torch.profiler import ProfilerActivity, profile
    sb, gd, g = mols
    model, _ = _stack(kind)
    model.train()
    Xp = _features(sb, 74).to(DEV).requires_grad_()
    gout = torch.randn((g.num_nodes(), 64) if kind == "gcn" else (len(sb.num_nodes), 11), device=DEV)
    model(g, Xp).backward(gout)  # warm-up: the degree factors are cached
    model.zero_grad(set_to_none=True)
    Xp.grad = None
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        model(g, Xp).backward(gout)
        torch.cuda.synchronize()
    ops = {e.name for e in prof.events() if e.name.startswith("aten::")}
    banned = ("add", "sub", "mul", "div", "sum", "mean", "mm", "matmul", "linear", "relu", "threshold", "where",
              "batch_norm", "native_batch_norm", "dropout", "index", "scatter", "sigmoid", "max", "neg", "sqrt")
    bad = sorted(o for o in ops if o[6:].rstrip("_").split(".")[0] in banned or o[6:].startswith(("addmm", "index_")))
    print(f"aten operators in one {kind} step: {sorted(ops)}")
    assert not bad, bad
    assert Xp.grad is not None and bool(torch.isfinite(Xp.grad).all())
