"""GATPredictor / GATv2Predictor on the GPU against the float64 reference composition
(tests/_predictor_ref.py; parity with dgllife is unpinned), weight-tied through
load_state_dict(strict=True).

Molecules of 1, 2, 63, 64, 65, 130 and 7 atoms.  Kinks are evaluated on the product's own side in
both references: the LeakyReLU side of every edge (GAT: el + er of DEBUG_CAPTURE["elr_fwd"];
GATv2: ZL[src] + ZR[dst] of ["zlr_fwd"], per element), the ReLU side of predict.1's output
(["relu_out"]) and the atom that owns each column's max (["readout_argmax"]).

Bar (the project's rule): conftest.rel_err <= max(1e-5, 4 e32) per quantity, e32 the same
reference in float32 against its float64 run.  Every case prints its worst err / budget.

Weights.  Two quantities of the float64 reference say how far fp32 arithmetic of ANY kind can be
trusted on a model, and seven molecules behind a ReLU make both vary by orders of magnitude with
the weights (conditioning() below; test_predictor_cpu.py recomputes the choice without a GPU):
  * the gate bias of the readout (atom_weighting.0.bias) is ONE number whose gradient sums
    c_n = gate (1 - gate) <g_s, x_n> over all 332 atoms, and behind a BatchNorm (whose input
    gradient is orthogonal to the batch mean) the terms largely cancel: sum |c_n| / |sum c_n| is
    21 / 280 / 4 / 21 for the four models at weight seed 3 and ranges 6 .. 2037 over seeds 3 .. 10;
  * BatchNorm divides by the batch deviation of each column of predict.1's ReLU output, and a
    column that is live in one or two of the seven molecules can have a deviation of 1e-3 of the
    largest activation: A = max |h| / min_c std_c (live columns) is 150 .. 8000.  The products
    feeding it carry 2^-22 of their row's largest value (split-fp16), xhat then A 2^-22.
e32 is one float32 sample per quantity and can come out far below either effect by luck.  Each
model therefore takes the FIRST weight seed >= 3 at which the float64 reference has ratio <= 32
and A <= 1024, decided from the reference alone: SEEDS."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _predictor_ref import PredictorRef
from _util import batch_of_sizes, graph_dict, randomize_
from conftest import rel_err
from mvml_gat import FlatAdam, GATPredictor, GATv2Predictor, bce_with_logits
from mvml_gat import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SIZES = [1, 2, 63, 64, 65, 130, 7]
HIDDEN, HEADS = [8, 12], [2, 4]
# name: (kind, agg_modes, predictor hidden feats, n_tasks)
MODELS = {"gat-mean": ("gat", None, 20, 3), "gat-flatten": ("gat", ["flatten", "flatten"], 20, 3),
          "gatv2-mean": ("gatv2", None, 20, 3), "gat-default-head": ("gat", None, 128, 1)}
SEEDS = {"gat-mean": 4, "gat-flatten": 7, "gatv2-mean": 8, "gat-default-head": 20}  # pick_seed(name)
BUFFERS = ("predict.predict.3.running_mean", "predict.predict.3.running_var")
NBT = "predict.predict.3.num_batches_tracked"


@pytest.fixture(scope="module")
def mols():
    sb = batch_of_sizes(SIZES, seed=9)
    return sb, graph_dict(sb), sb.to_graph().to(DEV), torch.as_tensor(sb.feats, dtype=torch.float32)


def _make(name, dropout=0.0, seed=None):
    kind, modes, hidden, n_tasks = MODELS[name]
    seed = SEEDS[name] if seed is None else seed
    torch.manual_seed(seed)
    if kind == "gat":
        m = GATPredictor(74, HIDDEN, HEADS, agg_modes=modes, predictor_hidden_feats=hidden, n_tasks=n_tasks,
                         predictor_dropout=dropout)
    else:
        m = GATv2Predictor(74, HIDDEN, HEADS, agg_modes=modes, predictor_out_feats=hidden, n_tasks=n_tasks,
                           predictor_dropout=dropout)
    randomize_(m, seed)
    gen = torch.Generator().manual_seed(seed)
    bn = m.predict.predict[3]
    with torch.no_grad():  # BatchNorm's weight and buffers off their initial 1 / 0 / 1
        bn.weight.add_(0.2 * torch.randn(bn.weight.shape, generator=gen))
        bn.running_mean.add_(0.1 * torch.randn(bn.weight.shape, generator=gen))
        bn.running_var.add_(0.3 * torch.rand(bn.weight.shape, generator=gen))
    return m


def conditioning(name, seed):
    """(sum |c_n| / |sum c_n| of the gate bias's gradient, max |h| / min live-column deviation of
    predict.1's ReLU output) of the float64 reference at these weights, on the CPU."""
    from _readout_ref import wsum_max_ref
    sb = batch_of_sizes(SIZES, seed=9)
    gd, X = graph_dict(sb), torch.as_tensor(sb.feats, dtype=torch.float64)
    ref = _refs(name, _make(name, seed=seed))[0].train()
    h = ref.node_feats(gd, X)
    lin = ref.readout.weight_and_sum.atom_weighting[0]
    ro, _ = wsum_max_ref(gd["node_offsets"], h, lin.weight, lin.bias)
    ro.retain_grad()
    gout = torch.randn((len(SIZES), MODELS[name][3]), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    ref.predict(ro).backward(gout)
    D = h.shape[1]
    h = h.detach()
    gate = torch.sigmoid(h @ lin.weight.detach().reshape(-1) + lin.bias.detach())
    gid = torch.repeat_interleave(torch.arange(len(SIZES)), torch.as_tensor(SIZES))
    c = gate * (1 - gate) * (ro.grad[:, :D][gid] * h).sum(1)
    act = torch.relu(ref.predict.predict[1](ro.detach())).detach()
    std = act.std(0, unbiased=False)
    return float(c.abs().sum() / c.sum().abs()), float(act.max() / std[(act > 0).any(0)].min())


def pick_seed(name, first=3):
    seed = first
    while True:
        ratio, amp = conditioning(name, seed)
        if ratio <= 32 and amp <= 1024:
            return seed
        seed += 1


def _refs(name, model):
    kind, modes, hidden, n_tasks = MODELS[name]
    out = []
    for dt in (torch.float64, torch.float32):
        r = PredictorRef(kind, 74, HIDDEN, HEADS, agg_modes=modes, predictor_hidden_feats=hidden, n_tasks=n_tasks)
        r.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
        out.append(r.to(dt))
    return out


def _forward(model, g, X):
    """The product's forward with its kink sides captured."""
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        out = model(g, X)
    finally:
        Fn.DEBUG_CAPTURE = None
    return out, cap


def _sides(name, gd, cap):
    src = torch.as_tensor(np.asarray(gd["src"])).long()
    dst = torch.as_tensor(np.asarray(gd["dst"])).long()
    if MODELS[name][0] == "gat":
        br = [(e.cpu()[:, :H][src] + e.cpu()[:, H:][dst]) > 0 for e, H in zip(cap["elr_fwd"], HEADS)]
    else:
        br = [((zl.cpu()[src] + zr.cpu()[dst]) > 0).view(-1, H, Fo)
              for (zl, zr), H, Fo in zip(cap["zlr_fwd"], HEADS, HIDDEN)]
    (relu,) = cap["relu_out"]
    (am,) = cap["readout_argmax"]
    return dict(branches=br, relu_side=(relu > 0).cpu(), argmax=am.cpu().long())


def _compare(what, got, r64, r32):
    worst = (0.0, None, 0.0, 0.0)
    for k in got:
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (what, k)
        e, budget = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        worst = max(worst, (e / budget, k, e, budget))
        assert e <= budget, (what, k, e, budget)
    print(f"predictor {what}: worst err/budget {worst[1]}: {worst[2]:.2e} / {worst[3]:.2e} = {worst[0]:.3f}")


@pytest.mark.parametrize("name", list(MODELS))
def test_training_and_eval_against_float64(mols, name):
    sb, gd, g, X = mols
    model = _make(name)
    ref64, ref32 = _refs(name, model)
    model = model.to(DEV).train()
    Xp = X.to(DEV).requires_grad_()
    out_p, cap = _forward(model, g, Xp)
    assert out_p.shape == (len(SIZES), MODELS[name][3])
    sides = _sides(name, gd, cap)
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    out_p.backward(gout.float().to(DEV))
    got = {"logits": out_p.detach(), "dX": Xp.grad, **{k: p.grad for k, p in model.named_parameters()},
           **{k: model.state_dict()[k] for k in BUFFERS}}
    res = []
    for ref, dt in ((ref64, torch.float64), (ref32, torch.float32)):
        ref.train()
        Xr = X.to(dt).clone().requires_grad_()
        out_r = ref(gd, Xr, **sides)
        out_r.backward(gout.to(dt))
        res.append({"logits": out_r.detach(), "dX": Xr.grad, **{k: p.grad for k, p in ref.named_parameters()},
                    **{k: ref.state_dict()[k].clone() for k in BUFFERS}})
    assert sorted(got) == sorted(res[0])
    assert int(model.state_dict()[NBT]) == 1
    _compare(f"{name} train", got, res[0], res[1])
    # a second training-mode forward, then eval mode: the running statistics are the ones in use
    with torch.no_grad():
        model(g, Xp)
        for ref, dt in ((ref64, torch.float64), (ref32, torch.float32)):
            ref(gd, X.to(dt), **sides)
    assert int(model.state_dict()[NBT]) == 2 == int(ref64.state_dict()[NBT])
    model.eval()
    stats = {k: model.state_dict()[k].clone() for k in BUFFERS}
    with torch.no_grad():
        out_e, cap = _forward(model, g, Xp)
        sides = _sides(name, gd, cap)
        ev = [ref.eval()(gd, X.to(dt), **sides) for ref, dt in ((ref64, torch.float64), (ref32, torch.float32))]
    assert int(model.state_dict()[NBT]) == 2
    for k in BUFFERS:
        assert torch.equal(model.state_dict()[k], stats[k]), "eval mode changed a running statistic"
    assert rel_err(out_e, out_p) > 1e-3  # not the batch statistics' output
    _compare(f"{name} eval", {"logits": out_e, **stats},
             {"logits": ev[0], **{k: ref64.state_dict()[k] for k in BUFFERS}},
             {"logits": ev[1], **{k: ref32.state_dict()[k] for k in BUFFERS}})


def test_predictor_dropout_runs_repeats_under_manual_seed_and_differs_from_p0(mols):
    sb, gd, g, X = mols
    base = _make("gat-mean").to(DEV).train()
    drop = _make("gat-mean", dropout=0.5).to(DEV).train()
    Xd = X.to(DEV)
    outs = []
    gout = torch.randn((len(SIZES), 3), generator=torch.Generator().manual_seed(6)).to(DEV)
    for seed in (21, 21, 22):
        torch.manual_seed(seed)
        Xp = Xd.clone().requires_grad_()
        z = drop(g, Xp)
        z.backward(gout)
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(Xp.grad).all())
        outs.append((z.detach(), Xp.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])
    with torch.no_grad():
        z0 = base(g, Xd)
        assert rel_err(outs[0][0], z0) > 1e-3
        # eval mode: no Dropout at all (fresh models: the same running statistics)
        a, b = (_make("gat-mean", dropout=p).to(DEV).eval() for p in (0.0, 0.5))
        assert torch.equal(a(g, Xd), b(g, Xd))


def test_three_adam_steps_against_float64(mols):
    sb, gd, g, X = mols
    name = "gat-mean"
    model = _make(name)
    ref64, ref32 = _refs(name, model)
    model = model.to(DEV).train()
    y = (torch.rand((len(SIZES), 3), generator=torch.Generator().manual_seed(8)) > 0.5).float()
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    opts = [torch.optim.Adam(r.parameters(), lr=1e-3, weight_decay=1e-4) for r in (ref64, ref32)]
    Xd, yd = X.to(DEV), y.to(DEV)
    for _ in range(3):
        opt.zero_grad()
        z, cap = _forward(model, g, Xd)
        bce_with_logits(z, yd).backward()
        opt.step()
        sides = _sides(name, gd, cap)
        for ref, o, dt in ((ref64, opts[0], torch.float64), (ref32, opts[1], torch.float32)):
            ref.train()
            o.zero_grad()
            F.binary_cross_entropy_with_logits(ref(gd, X.to(dt), **sides), y.to(dt)).backward()
            o.step()
    sd, s64, s32 = model.state_dict(), ref64.state_dict(), ref32.state_dict()
    assert int(sd[NBT]) == 3 == int(s64[NBT])
    keys = [k for k in sd if k != NBT]
    _compare("gat-mean 3 Adam steps", {k: sd[k] for k in keys}, s64, s32)


def test_checkpoint_round_trip_is_bitwise(mols):
    sb, gd, g, X = mols
    Xd = X.to(DEV)
    for name in ("gat-mean", "gatv2-mean"):
        model = _make(name).to(DEV).train()
        with torch.no_grad():
            model(g, Xd)  # moves the running statistics and the counter
            ckpt = {k: v.cpu().clone() for k, v in model.state_dict().items()}
            fresh = _make(name, seed=99)
            fresh.load_state_dict(ckpt, strict=True)
            fresh = fresh.to(DEV).eval()
            assert int(fresh.state_dict()[NBT]) == 1
            assert torch.equal(fresh(g, Xd), model.eval()(g, Xd))
