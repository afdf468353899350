"""GINLayer / GIN / GINPredictor on the GPU against the float64 reference (tests/_gin_ref.py; parity
with dgllife is unpinned), weight-tied through load_state_dict(strict=True), on the 170-atom `mixed`
batch of tests/test_gpu_agg_shapes.py with seeded categorical atom and bond features
(tests/_gin_cases.py).

Bar (the project's rule, as tests/test_gpu_sage.py): conftest.rel_err <= max(1e-5, 4 e32) per
quantity, e32 the same reference in float32 against its float64 run.

ReLU sides and the max readout's argmax are taken from the product (Fn.DEBUG_CAPTURE: "gin_hidden"
for the MLP's ReLU, "gin_out" for a layer's own, "pool_argmax" for the readout's) and given to both
references, under _gin_cases.check_sides' cap: the float64 reference's own sides and argmax differ
in at most 2 elements per tensor, each a near-tie.  The weight seeds are chosen from the reference
alone (tests/_gin_cases.py STACK_SEEDS / ADAM_SEEDS; tests/test_gin_cpu.py recomputes the
conditions).

mlp[2]'s bias feeds BatchNorm1d directly, so its gradient is identically zero and every arithmetic
returns rounding noise for it: under the bar above that entry compares noise with noise (rel_err of
order 1e8 on both sides, printed as the worst key of most cases; measured 0.11 - 0.25 of its
budget).  Its consequence for Adam is in tests/_gin_cases.py (ADAM)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gcn_cases import mixed_batch, perturb_bn
from _gin_cases import (ADAM, ADAM_SEEDS, EDGE_TABLES, KINDS, LAYERS, STACK_SEEDS, adam_labels, categories,
                        check_sides, is_predictor, out_shape, stack)
from _gin_ref import GINLayerRef
from _util import graph_dict, randomize_
from conftest import rel_err
from mvml_gat import FlatAdam, GINLayer, bce_with_logits
from mvml_gat import functional as Fn
from mvml_gat._lib import call, ptr, stream_ptr
from test_gpu_agg_shapes import GRAPHS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
BN_BUFFERS = ("running_mean", "running_var")


@pytest.fixture(scope="module")
def mols():
    sb = GRAPHS["mixed"]()
    assert np.array_equal(sb.src_local, mixed_batch().src_local)  # _gcn_cases restates its arguments
    nc, ec = categories(sb)
    dev = lambda cs: [c.to(torch.int32).to(DEV) for c in cs]
    return sb, graph_dict(sb), sb.to_graph().to(DEV), (nc, ec), (dev(nc), dev(ec))


def _capture(fn):
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        out = fn()
    finally:
        Fn.DEBUG_CAPTURE = None
    return out, cap


def _sides(cap, relus, argmax=False):
    """The product's ReLU sides and argmax in the reference's layout."""
    hid, outs = list(cap.get("gin_hidden", [])), list(cap.get("gin_out", []))
    assert len(hid) == len(relus) and len(outs) == sum(relus) and len(cap.get("pool_argmax", [])) == int(argmax)
    return {"hidden": [(h > 0).cpu() for h in hid], "out": [(outs.pop(0) > 0).cpu() if r else None for r in relus],
            "argmax": cap["pool_argmax"][0].cpu().long() if argmax else None}


def _compare(what, got, r64, r32):
    worst = (0.0, None, 0.0, 0.0)
    assert sorted(got) == sorted(r64)
    for k in got:
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (what, k)
        e, budget = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        worst = max(worst, (e / budget, k, e, budget))
        assert e <= budget, (what, k, e, budget)
    print(f"gin {what}: worst err/budget {worst[1]}: {worst[2]:.2e} / {worst[3]:.2e} = {worst[0]:.3f}")


# ---- one layer --------------------------------------------------------------------------------
def _layer_pair(D, relu, bn, seed=3):
    torch.manual_seed(seed)
    m = GINLayer(EDGE_TABLES, D, batch_norm=bn, activation=F.relu if relu else None)
    randomize_(m, seed)
    perturb_bn(m, seed)
    refs = []
    for dt in (torch.float64, torch.float32):
        r = GINLayerRef(EDGE_TABLES, D, bn, relu)
        r.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
        refs.append(r.to(dt))
    return m.to(DEV), refs


@pytest.mark.parametrize("D", [64, 300])
@pytest.mark.parametrize("relu,bn", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["relu-bn", "relu-nobn", "none-bn", "none-nobn"])
def test_layer_against_float64(mols, relu, bn, D):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, refs = _layer_pair(D, relu, bn)
    model.train()
    X = torch.randn((g.num_nodes(), D), generator=torch.Generator().manual_seed(1))
    Xp = X.to(DEV).requires_grad_()
    out_p, cap = _capture(lambda: model(g, Xp, ecd))
    sides = _sides(cap, [relu])
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
        out_r = ref(gd, Xr, ec, sides["hidden"][0], sides["out"][0], rec)
        if dt == torch.float64:
            check_sides(rec, sides)
        out_r.backward(gout.to(dt))
        res.append({"out": out_r.detach(), "dX": Xr.grad, **{k: p.grad for k, p in ref.named_parameters()},
                    **{k: ref.state_dict()[k].clone() for k in bufs}})
    _compare(f"layer D={D} relu={relu} bn={bn}", got, res[0], res[1])


def test_edge_table_gradient_is_the_count_weighted_sum_of_g(mols):
    """With the MLP's first Linear the identity on the first D of 2D units (and the ReLU open), no
    BatchNorm and the second Linear picking those units back, d out / d h is the identity, so an
    edge table's gradient row r is sum over edges with category r of g[dst]."""
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    D = 8
    model = GINLayer(EDGE_TABLES, D, batch_norm=False).to(DEV)
    with torch.no_grad():
        model.mlp[0].weight.zero_(), model.mlp[0].bias.fill_(1000.0), model.mlp[2].weight.zero_(), model.mlp[2].bias.zero_()
        model.mlp[0].weight[:D] = torch.eye(D)
        model.mlp[2].weight[:, :D] = torch.eye(D)
    X = torch.zeros((g.num_nodes(), D), device=DEV)
    gout = torch.randn((g.num_nodes(), D), generator=torch.Generator().manual_seed(2))
    model(g, X, ecd).backward(gout.to(DEV))
    dst = torch.as_tensor(gd["dst"]).long()
    for t, n in enumerate(EDGE_TABLES):
        want = torch.zeros((n, D), dtype=torch.float64).index_add(0, ec[t], gout.double()[dst])
        assert rel_err(model.edge_embeddings[t].weight.grad, want) <= TOL, t


# ---- the stack and the predictor ----------------------------------------------------------------
def _relus():
    return [True] * (LAYERS - 1) + [False]


def _run_product(model, g, ncd, ecd, kind):
    out, cap = _capture(lambda: model(g, ncd, ecd))
    return out, cap, _sides(cap, _relus(), is_predictor(kind) and KINDS[kind]["readout"] == "max")


@pytest.mark.parametrize("kind", list(KINDS))
def test_stack_against_float64(mols, kind):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, refs = stack(kind, STACK_SEEDS[kind], DEV)
    model.train()
    out_p, cap, sides = _run_product(model, g, ncd, ecd, kind)
    assert out_p.shape == out_shape(kind, sb)
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    sd = model.state_dict()
    bufs = [k for k in sd if k.endswith(BN_BUFFERS)]
    got = {"out": out_p.detach(), **{k: p.grad for k, p in model.named_parameters()}, **{k: sd[k] for k in bufs}}
    res = []
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        ref.train()
        rec = {}
        out_r = ref(gd, nc, ec, sides, rec)
        if dt == torch.float64:
            check_sides(rec, sides)
        out_r.backward(gout.to(dt))
        res.append({"out": out_r.detach(), **{k: p.grad for k, p in ref.named_parameters()},
                    **{k: ref.state_dict()[k].clone() for k in bufs}})
    _compare(f"{kind} train", got, res[0], res[1])


@pytest.mark.parametrize("kind", ["last", "pred_mean"])
def test_dropout_parity_with_the_regenerated_mask(mols, monkeypatch, kind):
    """Every layer's Dropout draws with the patched seed; the mask is a function of (seed, element
    index) alone, so one regenerated [N, D] mask serves the references at every layer."""
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    p, seed, D = 0.25, 123456789, KINDS[kind]["emb"]
    model, refs = stack(kind, STACK_SEEDS[kind], DEV, dropout=p)
    model.train()
    monkeypatch.setattr(Fn, "dropout_seed", lambda: seed)
    ones = torch.ones((g.num_nodes(), D), device=DEV)
    mask = torch.empty_like(ones)
    call("mvml_dropout_fwd", ones.numel(), ptr(ones), ptr(mask), p, seed, stream_ptr())
    mask = mask.cpu()
    kept = mask != 0
    assert 0.6 < float(kept.float().mean()) < 0.9 and torch.equal(mask[kept], torch.full_like(mask[kept], 1 / (1 - p)))
    out_p, cap, sides = _run_product(model, g, ncd, ecd, kind)
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    got = {"out": out_p.detach(), **{k: q.grad for k, q in model.named_parameters()}}
    res = []
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        ref.train()
        rec = {}
        out_r = ref(gd, nc, ec, sides, rec, [mask.to(dt)] * LAYERS)
        if dt == torch.float64:
            check_sides(rec, sides)
        out_r.backward(gout.to(dt))
        res.append({"out": out_r.detach(), **{k: q.grad for k, q in ref.named_parameters()}})
    _compare(f"{kind} dropout 0.25", got, res[0], res[1])


def test_dropout_repeats_under_manual_seed_and_eval_mode_uses_the_running_statistics(mols):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    base, refs = stack("pred_mean", 3, DEV)
    drop, _ = stack("pred_mean", 3, DEV, dropout=0.5)
    outs = []
    drop.train()
    for seed in (21, 21, 22):
        torch.manual_seed(seed)
        with torch.no_grad():
            before = {k: v.clone() for k, v in drop.state_dict().items()}
            outs.append(drop(g, ncd, ecd))
            drop.load_state_dict(before)  # (the running statistics moved)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    with torch.no_grad():
        base.load_state_dict(drop.state_dict())
        z = drop.eval()(g, ncd, ecd)
        assert torch.equal(z, base.eval()(g, ncd, ecd))  # no dropout in eval mode
        assert rel_err(outs[0], base.train()(g, ncd, ecd)) > 1e-3
        # eval mode normalises with the running statistics: the references in eval mode
        r64, r32 = refs
        z64, z32 = r64.eval()(gd, nc, ec), r32.eval()(gd, nc, ec)
        assert rel_err(z, z64) <= max(TOL, 4 * rel_err(z32, z64))
        assert rel_err(z, r64.train()(gd, nc, ec)) > 1e-3


@pytest.mark.parametrize("kind", list(ADAM_SEEDS))
def test_three_adam_steps_against_float64(mols, kind):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, refs = stack(kind, ADAM_SEEDS[kind], DEV)
    model.train()
    y = adam_labels(kind, sb)
    yd = y.to(DEV)
    opt = FlatAdam(model.parameters(), **ADAM)
    opts = [torch.optim.Adam(r.parameters(), **ADAM) for r in refs]
    for _ in range(3):
        opt.zero_grad()
        z, cap, sides = _run_product(model, g, ncd, ecd, kind)
        bce_with_logits(z, yd).backward()
        opt.step()
        for ref, o, dt in zip(refs, opts, (torch.float64, torch.float32)):
            ref.train()
            o.zero_grad()
            rec = {}
            zr = ref(gd, nc, ec, sides, rec)
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


@pytest.mark.parametrize("kind", ["concat", "pred_max"])
def test_checkpoint_round_trip_is_bitwise(mols, kind):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, _ = stack(kind, 3, DEV)
    model.train()
    with torch.no_grad():
        model(g, ncd, ecd)  # moves the running statistics and counters
        ckpt = {k: v.cpu().clone() for k, v in model.state_dict().items()}
        fresh, _ = stack(kind, 99, DEV)
        fresh.load_state_dict(ckpt, strict=True)
        fresh.eval()
        assert all(torch.equal(v.cpu(), ckpt[k]) for k, v in fresh.state_dict().items())
        assert torch.equal(fresh(g, ncd, ecd), model.eval()(g, ncd, ecd))


def test_two_runs_are_bitwise_equal_and_the_codes_are_cached_on_the_batch(mols):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, _ = stack("pred_max", 3, DEV)
    model.train()
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        z = model(g, ncd, ecd)
        z.sum().backward()
        runs.append((z.detach().clone(), [p.grad.clone() for p in model.parameters()]))
        model.load_state_dict(state)
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    cache = g._dev["gin_codes"]
    assert len(cache) == 1  # one entry for these feature tensors and table sizes, made once
    g.recollate()
    assert "gin_codes" not in g._dev  # dropped with the indices it was made from
    with torch.no_grad():
        assert torch.equal(model(g, ncd, ecd), runs[0][0]) and len(g._dev["gin_codes"]) == 1


def test_out_of_range_edge_categories_raise(mols):
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, _ = stack("last", 3, DEV)
    bad = [ecd[0].clone(), ecd[1].clone()]
    bad[1][3] = EDGE_TABLES[1]
    with pytest.raises(IndexError, match="outside"):
        model(g, ncd, bad)
    with pytest.raises(ValueError, match="edge tables"):
        model(g, ncd, ecd[:1])


@pytest.mark.parametrize("kind", ["pred_mean", "pred_max", "sum"])
def test_no_framework_arithmetic_in_forward_or_backward(mols, kind):
    """With JK 'concat' / 'sum' every h_l feeds the next layer and the jumping knowledge; their two
    gradients must meet in a HIP kernel (Fn.ForkFunction), not in an add of the autograd engine: no
    aten arithmetic operator runs in a training-mode forward + backward."""
    from torch.profiler import ProfilerActivity, profile
    sb, gd, g, (nc, ec), (ncd, ecd) = mols
    model, _ = stack(kind, 3, DEV, dropout=0.25)
    model.train()
    gout = torch.randn(out_shape(kind, sb), device=DEV)
    model(g, ncd, ecd).backward(gout)  # warm-up: the slot codes are cached
    model.zero_grad(set_to_none=True)
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        model(g, ncd, ecd).backward(gout)
        torch.cuda.synchronize()
    ops = {e.name for e in prof.events() if e.name.startswith("aten::")}
    banned = ("add", "sub", "mul", "div", "sum", "mean", "mm", "matmul", "linear", "relu", "threshold", "where",
              "batch_norm", "native_batch_norm", "dropout", "index", "scatter", "sigmoid", "max", "neg", "sqrt",
              "embedding", "embedding_dense_backward", "cat", "index_select", "gather")
    bad = sorted(o for o in ops if o[6:].rstrip("_").split(".")[0] in banned or o[6:].startswith(("addmm", "index_")))
    print(f"aten operators in one {kind} step: {sorted(ops)}")
    assert not bad, bad
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
