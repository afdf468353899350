"""The weighted-sum-and-max readout (csrc/readout.hip) on the GPU against float64
(tests/_readout_ref.py): at the C ABI on padded, sentinel-filled buffers, through the modules,
through the graph view and through MVP.

The kernels hold a molecule's D columns as NV = ceil(D / 256) float4 slots per lane: D = 4, 100,
260, 516, 772 are NV = 1 .. 4 with a partly masked last slot, 1024 the full widest one.  They keep
4 or 2 atom rows in flight (forward: 4 at NV <= 2; backward: 4 at NV = 1), so the molecule sizes sit
around those counts and around the wavefront's 64 lanes; a workgroup is four molecules, so 8 and 5 molecules are two
workgroups, the second partly and nearly empty.

Bars (the project's rule): max(1e-5, 4 x e32) norm-wise (conftest.rel_err), e32 the error of the
same reference evaluated in float32 on the CPU; the argmax must EQUAL the reference's at the C ABI
(comparisons of fp32 inputs are exact).  Each case prints its worst err / budget."""
import numpy as np
import pytest
import torch

from _readout_ref import gate_ref, wsum_max_ref
from _util import batch_of_sizes, graph_dict, randomize_
from conftest import rel_err
from mvml_gat import functional as Fn
from mvml_gat._lib import call, lib, ptr, stream_ptr
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SIZES_A = [1, 2, 63, 64, 65, 130, 7, 300]
SIZES_B = [0, 3, 0, 65, 0]
SIZE_LISTS = {"A": SIZES_A, "B": SIZES_B}
MODULE_SIZES = [1, 2, 63, 64, 65, 130, 7]
SENT = 7.0


def _offsets(sizes):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)


def _inputs(D, which, pattern):
    """Seeded fp32 inputs (CPU): X [N, D], W [1, D], b [1], g_out [B, 2 D]."""
    sizes = SIZE_LISTS[which]
    offs = _offsets(sizes)
    B, N = len(sizes), int(offs[-1])
    gen = torch.Generator().manual_seed(1000 * D + len(sizes))
    X = torch.randn((N, D), generator=gen)
    W = torch.randn((1, D), generator=gen) / D ** 0.5
    b = torch.randn((1,), generator=gen)
    g_out = torch.randn((B, 2 * D), generator=gen)
    if pattern == "neg":  # a zero-initialised max would show
        X = -X.abs() - 1
    elif pattern == "ties":  # atoms 2, 5 and 40 of the 65- and 130-atom molecules: one row, on top
        for g in (4, 5):
            n0 = int(offs[g])
            X[n0 + 5] = X[n0 + 2]
            X[n0 + 40] = X[n0 + 2]
            X[[n0 + 2, n0 + 5, n0 + 40]] += 10
    elif pattern == "saturated":  # |<W, x>| reaches 50: gates at 0 and 1 in fp32
        W = W * (50.0 / (X @ W.reshape(-1)).abs().max())
        b = torch.zeros(1)
    return sizes, offs, X, W, b, g_out


_REF = {}


def _reference(D, which, pattern):
    """float64 outputs and gradients, and the float32 reference's error e32 per quantity (made
    once per case, shared, never changed)."""
    key = (D, which, pattern)
    if key in _REF:
        return _REF[key]
    sizes, offs, X, W, b, g_out = _inputs(D, which, pattern)
    res = {}
    for dt in (torch.float64, torch.float32):
        Xr, Wr, br = (t.to(dt).clone().requires_grad_() for t in (X, W, b))
        out, am = wsum_max_ref(offs, Xr, Wr, br)
        out.backward(g_out.to(dt))
        res[dt] = dict(out=out.detach(), gate=gate_ref(Xr, Wr, br).detach(), gX=Xr.grad, dW=Wr.grad,
                       db=br.grad, argmax=am)
    r64, r32 = res[torch.float64], res[torch.float32]
    assert torch.equal(r64["argmax"], r32["argmax"])
    e32 = {k: rel_err(r32[k], r64[k]) for k in ("out", "gate", "gX", "dW", "db")}
    _REF[key] = (r64, e32)
    return _REF[key]


def _run_abi(D, which, pattern, check_guards=True):
    """Forward and backward through the C ABI on padded buffers; returns the unpadded results."""
    sizes, offs, X, W, b, g_out = _inputs(D, which, pattern)
    B, N = len(sizes), int(offs[-1])
    ldx, ldo, lda, ldgx, ldp = D + 4, 2 * D + 4, D + 4, D + 4, D + 8
    Xp = torch.full((N, ldx), float("nan"))
    Xp[:, :D] = X
    gp = torch.full((B, ldo), float("nan"))
    gp[:, :2 * D] = g_out
    d_offs, d_X, d_W, d_b, d_g = (t.to(DEV) for t in (offs, Xp, W.reshape(-1).contiguous(), b, gp))
    out = torch.full((B, ldo), SENT, device=DEV)
    gate = torch.full((N + 8,), SENT, device=DEV)
    argmax = torch.full((B, lda), -7, dtype=torch.int32, device=DEV)
    gX = torch.full((N + 1, ldgx), SENT, device=DEV)  # one guard row
    R = lib().mvml_wsum_max_bwd_part_rows(B)
    assert R == (B + 3) // 4
    part = torch.full((R + 1, ldp), SENT, device=DEV)
    st = stream_ptr()
    call("mvml_wsum_max_fwd", B, N, D, ptr(d_offs), ptr(d_X), ldx, ptr(d_W), ptr(d_b), ptr(out), ldo,
         ptr(gate), ptr(argmax), lda, st)
    call("mvml_wsum_max_bwd", B, N, D, ptr(d_offs), ptr(d_X), ldx, ptr(d_W), ptr(gate), ptr(argmax), lda,
         ptr(d_g), ldo, ptr(gX), ldgx, ptr(part), ldp, st)
    dW = torch.empty(D, device=DEV)
    db = torch.empty(1, device=DEV)
    Fn.colsum(part, R, D, ldp, dW)
    Fn.colsum(part, R, 1, ldp, db, offset=D)
    torch.cuda.synchronize()
    if check_guards:
        assert bool((out[:, 2 * D:] == SENT).all()), "out pad written"
        assert bool((gate[N:] == SENT).all()), "gate past the last atom written"
        assert bool((gate[:N] != SENT).all()), "a gate entry not written"
        assert bool((argmax[:, D:] == -7).all()), "argmax pad written"
        assert bool((gX[:N, D:] == SENT).all()) and bool((gX[N] == SENT).all()), "gX pad / guard row written"
        assert bool((part[:R, D + 1:] == SENT).all()) and bool((part[R] == SENT).all()), "partials pad written"
    return dict(out=out[:, :2 * D].clone(), gate=gate[:N].clone(), argmax=argmax[:, :D].clone(),
                gX=gX[:N, :D].clone(), dW=dW.reshape(1, D), db=db, part=part[:R].clone())


def _compare(tag, got, r64, e32):
    assert torch.equal(got["argmax"].cpu().long(), r64["argmax"]), "argmax differs from the reference"
    margins = {}
    for k in ("out", "gate", "gX", "dW", "db"):
        assert bool(torch.isfinite(got[k]).all()), k
        margins[k] = (rel_err(got[k], r64[k]), max(TOL, 4 * e32[k]))
    worst = max(margins, key=lambda k: margins[k][0] / margins[k][1])
    print(f"readout {tag}: worst err/budget {worst}: {margins[worst][0]:.2e} / {margins[worst][1]:.2e} = "
          f"{margins[worst][0] / margins[worst][1]:.3f}")
    for k, (e, budget) in margins.items():
        assert e < budget, (k, e, budget)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("D", [4, 100, 260, 516, 772, 1024])
def test_abi_against_float64(D, which):
    r64, e32 = _reference(D, which, "plain")
    got = _run_abi(D, which, "plain")
    _compare(f"D={D} sizes {which}", got, r64, e32)
    sizes = SIZE_LISTS[which]
    for g, n in enumerate(sizes):
        if n == 0:  # sum 0, max 0, argmax -1
            assert bool((got["out"][g] == 0).all()) and bool((got["argmax"][g] == -1).all())


@pytest.mark.parametrize("pattern", ["neg", "ties", "saturated"])
def test_abi_value_patterns(pattern):
    D = 260
    r64, e32 = _reference(D, "A", pattern)
    got = _run_abi(D, "A", pattern)
    _compare(f"D={D} {pattern}", got, r64, e32)
    sizes, offs, X, W, b, g_out = _inputs(D, "A", pattern)
    if pattern == "neg":
        assert bool((got["out"][:, D:] < 0).all())
    if pattern == "saturated":
        gt = got["gate"]
        assert float(gt.min()) < 1e-10 and float(gt.max()) > 0.999999  # both ends reached
    if pattern == "ties":
        for g in (4, 5):
            n0 = int(offs[g])
            assert bool((got["argmax"][g] == n0 + 2).all())
            gx = got["gX"]
            # the three rows are one x, one gate, one t: equal but for the g_m term, which atom 2
            # alone receives — one fp32 rounding of (a + g_m) away from exact
            assert torch.equal(gx[n0 + 5], gx[n0 + 40])
            gm = g_out[g, D:].to(DEV)
            assert rel_err(gx[n0 + 2] - gx[n0 + 5], gm) < 1e-6


def test_abi_bitwise_deterministic():
    D = 516
    a = _run_abi(D, "A", "plain", check_guards=False)
    b = _run_abi(D, "A", "plain", check_guards=False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_abi_no_molecules_no_atoms():
    st = stream_ptr()
    offs = torch.zeros(4, dtype=torch.int64, device=DEV)
    t = torch.full((16,), SENT, device=DEV)
    i = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    for B, N in ((0, 0), (3, 0)):
        call("mvml_wsum_max_fwd", B, N, 4, ptr(offs), ptr(t), 4, ptr(t), ptr(t), ptr(t), 8, ptr(t), ptr(i), 4, st)
        call("mvml_wsum_max_bwd", B, N, 4, ptr(offs), ptr(t), 4, ptr(t), ptr(t), ptr(i), 4, ptr(t), 8, ptr(t), 4,
             ptr(t), 8, st)
    torch.cuda.synchronize()
    assert bool((t == SENT).all()) and bool((i == -7).all())
    assert lib().mvml_wsum_max_bwd_part_rows(0) == 0
    from mvml_gat._lib import MvmlError
    for D in (6, 1028):
        with pytest.raises(MvmlError, match="multiple of 4"):
            call("mvml_wsum_max_fwd", 1, 1, D, ptr(offs), ptr(t), 1032, ptr(t), ptr(t), ptr(t), 2064, ptr(t),
                 ptr(i), 1032, st)


@pytest.fixture(scope="module")
def batch():
    sb = batch_of_sizes(MODULE_SIZES, seed=9)
    return sb, sb.to_graph(group_size=3).to(DEV)


@pytest.mark.parametrize("D", [4, 260, 1024])
def test_module_against_float64(batch, D):
    from mvml_gat import WeightAndSum, WeightedSumAndMax
    sb, g = batch
    offs = _offsets(MODULE_SIZES)
    N, B = int(offs[-1]), len(MODULE_SIZES)
    torch.manual_seed(D)
    mod = WeightedSumAndMax(D)
    lin = mod.weight_and_sum.atom_weighting[0]
    big = torch.randn(N, D + 8)
    gout = torch.randn(B, 2 * D)
    res = {}
    for dt in (torch.float64, torch.float32):
        Xr = big[:, 4:4 + D].to(dt).clone().requires_grad_()
        Wr, br = (p.detach().to(dt).clone().requires_grad_() for p in (lin.weight, lin.bias))
        out, _ = wsum_max_ref(offs, Xr, Wr, br)
        out.backward(gout.to(dt))
        res[dt] = dict(out=out.detach(), dX=Xr.grad, dW=Wr.grad, db=br.grad)
    r64, r32 = res[torch.float64], res[torch.float32]
    mod = mod.to(DEV)
    bigd = big.to(DEV).requires_grad_()
    Xp = bigd[:, 4:4 + D]  # a column slice: read in place through its row pitch
    assert not Xp.is_contiguous()
    out_p = mod(g, Xp)
    assert out_p.shape == (B, 2 * D)
    out_p.backward(gout.to(DEV))
    lin = mod.weight_and_sum.atom_weighting[0]
    got = dict(out=out_p, dX=bigd.grad[:, 4:4 + D], dW=lin.weight.grad, db=lin.bias.grad)
    assert float(bigd.grad[:, :4].abs().max()) == 0 and float(bigd.grad[:, 4 + D:].abs().max()) == 0
    margins = {k: (rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))) for k in got}
    worst = max(margins, key=lambda k: margins[k][0] / margins[k][1])
    print(f"WeightedSumAndMax D={D}: worst err/budget {worst}: {margins[worst][0] / margins[worst][1]:.3f}")
    for k, (e, budget) in margins.items():
        assert e < budget, (k, e, budget)
    # WeightAndSum alone: the sum half, the same bits
    ws = WeightAndSum(D).to(DEV)
    ws.load_state_dict(mod.weight_and_sum.state_dict())
    with torch.no_grad():
        s = ws(g, Xp)
    assert s.shape == (B, D) and torch.equal(s, out_p[:, :D])


def _view_ref(params, gd, X, offs, hidden, dt, branches, fc_branch, argmax):
    """GAT -> weighted-sum-and-max -> GraphNorm -> Linear + ReLU in dtype dt from the product's
    parameters (leaves), on the product's side of every kink."""
    p = {k: v.detach().cpu().to(dt).clone().requires_grad_() for k, v in params.items()}
    lp = [{k: p[f"conv.gnn_layers.{i}.gat_conv.{k}"] for k in ("fc.weight", "res_fc.weight", "attn_l",
                                                             "attn_r", "bias")} for i in range(len(hidden))]
    Xr = X.to(dt).clone().requires_grad_()
    node_x = gnn_ref.gat_ref(gd["src"], gd["dst"], Xr, lp, hidden, branches=branches)
    ro, _ = wsum_max_ref(offs, node_x, p["readout.weight_and_sum.atom_weighting.0.weight"],
                         p["readout.weight_and_sum.atom_weighting.0.bias"], argmax=argmax)
    y = gnn_ref.graphnorm_ref(ro, p["norm.weight"], p["norm.bias"], p["norm.mean_scale"], 1e-5,
                              gd["group_offsets"])
    y = gnn_ref.relu_branch(y @ p["fc.0.weight"].t() + p["fc.0.bias"], fc_branch)
    return y, Xr, p, node_x.detach()


def test_view_against_float64(batch):
    from mvml_gat import GNNModule
    from test_gpu_parity_configs import _branches
    sb, g = batch
    gd = graph_dict(sb, group_size=3)
    offs = _offsets(MODULE_SIZES)
    hidden = [20, 260]
    torch.manual_seed(6)
    prod = GNNModule(74, hidden, 0.0, readout="weighted_sum_max")
    randomize_(prod, 6)
    prod = prod.to(DEV)
    X = torch.as_tensor(sb.feats, dtype=torch.float32)
    Xp = X.to(DEV).requires_grad_()
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        out_p = prod(g, Xp)
    finally:
        Fn.DEBUG_CAPTURE = None
    assert out_p.shape == (len(MODULE_SIZES), 260)
    br = _branches(gd, [e.cpu() for e in cap["elr_fwd"]])
    fcb = (cap["relu_out"][-1] > 0).cpu()
    (am,) = cap["readout_argmax"]
    am = am.cpu().long()
    gout = torch.randn(out_p.shape, generator=torch.Generator().manual_seed(6))
    out_p.backward(gout.to(DEV))
    params = dict(prod.named_parameters())
    y64, X64, p64, node64 = _view_ref(params, gd, X, offs, hidden, torch.float64, br, fcb, am)
    y64.backward(gout.double())
    y32, X32, p32, _ = _view_ref(params, gd, X, offs, hidden, torch.float32, br, fcb, am)
    y32.backward(gout)
    # the max is a kink where atoms tie: EVERY atom the product chose holds the float64 segment
    # maximum to within 1e-6 of the feature scale
    scale = float(node64.abs().max())
    for gi in range(len(MODULE_SIZES)):
        seg = node64[int(offs[gi]):int(offs[gi + 1])]
        chosen = node64.gather(0, am[gi].unsqueeze(0))[0]
        assert bool((am[gi] >= offs[gi]).all()) and bool((am[gi] < offs[gi + 1]).all())
        assert float((seg.max(0).values - chosen).max()) <= 1e-6 * scale
    margins = {"out": (rel_err(out_p, y64), max(TOL, 4 * rel_err(y32, y64))),
               "dX": (rel_err(Xp.grad, X64.grad), max(TOL, 4 * rel_err(X32.grad, X64.grad)))}
    for n, p in params.items():
        margins[n] = (rel_err(p.grad, p64[n].grad), max(TOL, 4 * rel_err(p32[n].grad, p64[n].grad)))
    worst = max(margins, key=lambda k: margins[k][0] / margins[k][1])
    print(f"GNNModule weighted_sum_max: worst err/budget {worst}: {margins[worst][0]:.2e} / "
          f"{margins[worst][1]:.2e} = {margins[worst][0] / margins[worst][1]:.3f}")
    for k, (e, budget) in margins.items():
        assert e < budget, (k, e, budget)


def test_mvp_trains_with_the_readout():
    from mvml_gat import MVP, bce_with_logits
    from test_gpu_mvp import _kegg_batch
    bg, gd, x, smiles, fp, y = _kegg_batch(n=7)
    torch.manual_seed(7)
    # num_heads = 12: the only head count the fusion head takes
    mod = MVP(11, 74, [64, 128], num_heads=12, graph_readout="weighted_sum_max", device=DEV).to(DEV).train()
    g = bg.to(DEV)
    z = mod({"smiles": smiles["smiles"].to(DEV), "seq_len": smiles["seq_len"]}, g, g.ndata["h"].to(DEV),
            fp.float().to(DEV))
    assert z.shape == (7, 11) and bool(torch.isfinite(z).all())
    bce_with_logits(z, y.float().to(DEV)).backward()
    unused = ("norm_layer.", "rnn.norm_layer.")  # constructed, never called (model.py:39, 120)
    for n, p in mod.named_parameters():
        if p.grad is None:
            assert n.startswith(unused), n
            continue
        assert bool(torch.isfinite(p.grad).all()), n
    for n in ("gnn.readout.weight_and_sum.atom_weighting.0.weight", "gnn.readout.weight_and_sum.atom_weighting.0.bias"):
        assert float(dict(mod.named_parameters())[n].grad.abs().max()) > 0
