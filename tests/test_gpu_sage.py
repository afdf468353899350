"""SAGEConv / GraphSAGE / GraphSAGEPredictor on the GPU against the float64 reference
(tests/_sage_ref.py; parity with dgl / dgllife is unpinned), weight-tied through
load_state_dict(strict=True), on the 170-atom `mixed` batch of tests/test_gpu_agg_shapes.py.

Bar (the project's rule, as tests/test_gpu_gcn.py): conftest.rel_err <= max(1e-5, 4 e32) per
quantity, e32 the same reference in float32 against its float64 run.

ReLU sides and the neighbour maximum's arg are taken from the product (Fn.DEBUG_CAPTURE: "sage_out"
for a layer's ReLU, "sage_pool" for fc_pool's, "sage_arg" for the maximum's owner slots, "relu_out"
for predict.1's, "readout_argmax" for the readout's) and given to both references, under
_sage_cases.check_sides' cap: the float64 reference's own sides and argmax differ in at most 2
elements per tensor, each a near-tie.  The weight seeds are chosen from the reference alone
(tests/_sage_cases.py STACK_SEEDS / ADAM_SEEDS; tests/test_sage_cpu.py recomputes the conditions)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gcn_cases import features as _features, mixed_batch
from _sage_cases import ADAM_SEEDS, KINDS, STACK_SEEDS, adam_labels, check_sides, out_shape, stack
from _sage_ref import SAGEConvRef
from _util import graph_dict, randomize_
from conftest import rel_err
from mvml_gat import FlatAdam, SAGEConv, bce_with_logits
from mvml_gat import functional as Fn
from mvml_gat._lib import call, ptr, stream_ptr
from test_gpu_agg_shapes import GRAPHS
from test_gpu_gcn_agg import _no_loops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
AGGREGATORS = ["mean", "gcn", "pool"]
# 74 -> 64: zero-padded, the product first (mean, gcn) / a 76-wide pooled middle; 64 -> 64: the
# aggregation first, sub-wave kernels; 20 -> 64: the aggregation first on 20 columns; 132 -> 24: the
# product first (132 > 24) and the sum on 24 columns, pool's maximum on the one-row kernel at 132
WIDTHS = [(74, 64), (64, 64), (20, 64), (132, 24)]
BN_BUFFERS = ("running_mean", "running_var")


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


def _sides(cap, aggrs, fins, relus, predict=False):
    """The product's ReLU sides and owner slots in the reference's layout (the pooled middle is
    zero-padded to a multiple of 4 columns in the product: its first in_feats columns)."""
    outs, pools, args = list(cap.get("sage_out", [])), list(cap.get("sage_pool", [])), list(cap.get("sage_arg", []))
    assert len(outs) == sum(relus) and len(pools) == len(args) == aggrs.count("pool")
    assert len(cap.get("relu_out", [])) == int(predict)
    sides = {"out": [], "pool": [], "arg": [], "predict": (cap["relu_out"][0] > 0).cpu() if predict else None}
    for a, fin, relu in zip(aggrs, fins, relus):
        sides["out"].append((outs.pop(0) > 0).cpu() if relu else None)
        sides["pool"].append((pools.pop(0)[:, :fin] > 0).cpu() if a == "pool" else None)
        sides["arg"].append(args.pop(0)[:, :fin].cpu().long() if a == "pool" else None)
    return sides


def _compare(what, got, r64, r32):
    worst = (0.0, None, 0.0, 0.0)
    assert sorted(got) == sorted(r64)
    for k in got:
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (what, k)
        e, budget = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        worst = max(worst, (e / budget, k, e, budget))
        assert e <= budget, (what, k, e, budget)
    print(f"sage {what}: worst err/budget {worst[1]}: {worst[2]:.2e} / {worst[3]:.2e} = {worst[0]:.3f}")


def _conv_pair(fin, fout, aggr, relu=True, bias=True, feat_drop=0.0, seed=3):
    torch.manual_seed(seed)
    m = SAGEConv(fin, fout, aggr, feat_drop, bias, activation=F.relu if relu else None)
    randomize_(m, seed)
    refs = []
    for dt in (torch.float64, torch.float32):
        r = SAGEConvRef(fin, fout, aggr, relu, bias)
        r.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
        refs.append(r.to(dt))
    return m.to(DEV), refs


def _conv_case(gd, g, X, model, refs, aggr, relu, what, mask=None):
    """Training-mode forward + every gradient against both references."""
    model.train()
    fin = X.shape[1]
    Xp = X.to(DEV).requires_grad_()
    out_p, cap = _capture(lambda: model(g, Xp))
    sides = _sides(cap, [aggr], [fin], [relu])
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    got = {"out": out_p.detach(), "dX": Xp.grad, **{k: p.grad for k, p in model.named_parameters()}}
    res = []
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        ref.train()
        Xr = X.to(dt).clone().requires_grad_()
        rec = {}
        out_r = ref(gd, Xr, sides["out"][0], sides["pool"][0], sides["arg"][0], rec, None if mask is None else mask.to(dt))
        if dt == torch.float64:
            check_sides(rec, sides)
        out_r.backward(gout.to(dt))
        res.append({"out": out_r.detach(), "dX": Xr.grad, **{k: p.grad for k, p in ref.named_parameters()}})
    _compare(what, got, res[0], res[1])
    return out_p.detach()


@pytest.mark.parametrize("relu,bias", [(True, True), (False, False), (True, False), (False, True)],
                         ids=["relu-bias", "none-nobias", "relu-nobias", "none-bias"])
@pytest.mark.parametrize("fin,fout", WIDTHS, ids=[f"{a}to{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("aggr", AGGREGATORS)
def test_conv_against_float64(mols, aggr, fin, fout, relu, bias):
    sb, gd, g = mols
    model, refs = _conv_pair(fin, fout, aggr, relu, bias)
    _conv_case(gd, g, _features(sb, fin), model, refs, aggr, relu, f"conv {aggr} {fin}->{fout} relu={relu} bias={bias}")


@pytest.mark.parametrize("aggr", AGGREGATORS)
def test_conv_feat_drop_parity_with_the_regenerated_mask(mols, monkeypatch, aggr):
    sb, gd, g = mols
    p, seed, fin, fout = 0.25, 123456789, 74, 64
    model, refs = _conv_pair(fin, fout, aggr, feat_drop=p)
    monkeypatch.setattr(Fn, "dropout_seed", lambda: seed)
    ones = torch.ones((g.num_nodes(), fin), device=DEV)
    mask = torch.empty_like(ones)
    call("mvml_dropout_fwd", ones.numel(), ptr(ones), ptr(mask), p, seed, stream_ptr())
    mask = mask.cpu()
    kept = mask != 0
    assert 0.6 < float(kept.float().mean()) < 0.9 and torch.equal(mask[kept], torch.full_like(mask[kept], 1 / (1 - p)))
    _conv_case(gd, g, _features(sb, fin), model, refs, aggr, True, f"conv {aggr} feat_drop 0.25", mask=mask.double())


@pytest.mark.parametrize("aggr", AGGREGATORS)
def test_conv_feat_drop_repeats_under_manual_seed_differs_from_p0_and_is_off_in_eval(mols, aggr):
    sb, gd, g = mols
    X = _features(sb, 74).to(DEV)
    base, _ = _conv_pair(74, 64, aggr)
    drop, _ = _conv_pair(74, 64, aggr, feat_drop=0.5)
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
        assert torch.equal(base.eval()(g, X), drop.eval()(g, X))


@pytest.mark.parametrize("aggr", AGGREGATORS)
def test_batch_without_self_loops_runs_with_zero_neighbour_rows(aggr):
    bg = _no_loops()
    src, dst = bg.edges()
    gd = {"src": src.long().numpy(), "dst": dst.long().numpy()}
    g = bg.to(DEV)
    assert g.has_zero_in_degree  # not refused: DGL's SAGEConv has no such check
    X = torch.randn((g.num_nodes(), 8), generator=torch.Generator().manual_seed(1))
    model, refs = _conv_pair(8, 12, aggr)
    _conv_case(gd, g, X, model, refs, aggr, True, f"conv {aggr} zero in-degree")
    # h_neigh of an atom without in-edges is 0 (mean, pool): with fc_self = 0 and no bias, its row is 0
    empty = torch.bincount(dst.long().cpu(), minlength=g.num_nodes()) == 0
    assert int(empty.sum()) >= 4
    if aggr != "gcn":
        model, _ = _conv_pair(8, 12, aggr, relu=False, bias=False)
        with torch.no_grad():
            model.fc_self.weight.zero_()
            out = model(g, X.to(DEV)).cpu()
        assert float(out[empty].abs().max()) == 0.0 and float(out[~empty].abs().max()) > 0.0


# ---- the stack and the predictor ----------------------------------------------------------------
def _stack_sides(cap, kind):
    k = KINDS[kind]
    return _sides(cap, k["aggr"], [74, k["hidden"][0]], [True, True], kind == "predictor")


def _ref_forward(kind, ref, gd, X, sides, cap, rec=None):
    if kind == "sage":
        return ref(gd, X, sides, rec)
    return ref(gd, X, sides, rec, argmax=cap["readout_argmax"][0].cpu().long())


@pytest.mark.parametrize("kind", ["sage", "predictor"])
def test_stack_against_float64(mols, kind):
    sb, gd, g = mols
    model, refs = stack(kind, STACK_SEEDS[kind], DEV)
    model.train()
    X = _features(sb, 74)
    Xp = g.ndata["h"].detach().requires_grad_()  # the batch's resident (zero-padded) atom features
    out_p, cap = _capture(lambda: model(g, Xp))
    assert out_p.shape == out_shape(kind, sb)
    sides = _stack_sides(cap, kind)
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


@pytest.mark.parametrize("kind", ["sage", "predictor"])
def test_three_adam_steps_against_float64(mols, kind):
    sb, gd, g = mols
    model, refs = stack(kind, ADAM_SEEDS[kind], DEV)
    model.train()
    X = _features(sb, 74)
    Xd = g.ndata["h"]
    y = adam_labels(kind, sb)
    yd = y.to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    opts = [torch.optim.Adam(r.parameters(), lr=1e-3, weight_decay=1e-4) for r in refs]
    for _ in range(3):
        opt.zero_grad()
        z, cap = _capture(lambda: model(g, Xd))
        bce_with_logits(z, yd).backward()
        opt.step()
        sides = _stack_sides(cap, kind)
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


@pytest.mark.parametrize("kind", ["sage", "predictor"])
def test_checkpoint_round_trip_is_bitwise(mols, kind):
    sb, gd, g = mols
    Xd = g.ndata["h"]
    model, _ = stack(kind, 3, DEV)
    model.train()
    with torch.no_grad():
        model(g, Xd)  # moves the predictor's running statistics and counter
        ckpt = {k: v.cpu().clone() for k, v in model.state_dict().items()}
        fresh, _ = stack(kind, 99, DEV)
        fresh.load_state_dict(ckpt, strict=True)
        fresh.eval()
        assert all(torch.equal(v.cpu(), ckpt[k]) for k, v in fresh.state_dict().items())
        assert torch.equal(fresh(g, Xd), model.eval()(g, Xd))


@pytest.mark.parametrize("kind", ["sage", "predictor"])
def test_no_framework_arithmetic_in_forward_or_backward(mols, kind):
    """Every SAGEConv's input feeds fc_self and the neighbour branch (and fc_pool); their input
    gradients must meet in the HIP kernels (Fn.SAGEConvFunction), not in an add of the autograd
    engine: no aten arithmetic operator runs in a training-mode forward + backward with the input's
    gradient on."""
    from torch.profiler import ProfilerActivity, profile
    sb, gd, g = mols
    model, _ = stack(kind, 3, DEV)
    model.train()
    Xp = _features(sb, 74).to(DEV).requires_grad_()
    gout = torch.randn(out_shape(kind, sb), device=DEV)
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
