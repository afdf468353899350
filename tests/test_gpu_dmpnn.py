"""D-MPNN on the GPU against the float64 formulas of tests/_dmpnn_ref.py: the kernels of csrc/dmpnn.hip
through mvml_gat.functional, then DMPNNPredictor, weight-tied through its state_dict.

Batch: _afp_ref.molecules() twice (single atom, two-atom molecule, six-ring, the 70-edge hub with parallel
bonds, the ringed chain), then three hand cases: a self-loop, a doubled bond u->v, u->v, v->u, v->u, and a
one-way edge (its source has no in-edge, the edge no reverse).  Widths: 64 (four atoms per wave), 68 (the
first with one atom per wave), 300 (two 256-column chunks, the second partial); the init kernel also at
1024 with 12 (W_ieT in LDS) and 13 bond features (the first that leave it).

Bar (the project's rule, as tests/test_gpu_mpnn.py): conftest.rel_err (norm-wise) <= max(1e-5, 4 e32) per
quantity, e32 the same formulas in float32 on the CPU against their float64 run."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _afp_ref as A
import _dmpnn_ref as R
import mvml_gat
from conftest import rel_err
from mvml_gat import DMPNNGNN, DMPNNPredictor, bce_with_logits
from mvml_gat import functional as Fn
from mvml_gat._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
FA = 39
_bits = lambda x: x.contiguous().view(torch.int32)  # noqa: E731
HAND = ([1, 2, 2], [1, 4, 1], [0, 0, 0, 1, 1, 0], [0, 1, 1, 0, 0, 1])  # self-loop | doubled bond | one-way


def _check(what, got, r64, r32):
    for k in r64:
        e, b = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        print(f"dmpnn {what} {k}: {e:.2e} / {b:.2e}")
        assert bool(torch.isfinite(got[k]).all()) and e <= b, (what, k, e, b)


def _both(fn, leaves):
    """fn's outputs and the gradients of its leaves at float64 and float32: fn(leaves) -> (outs, loss)."""
    res = []
    for dt in (torch.float64, torch.float32):
        ls = {k: v.to(dt).clone().requires_grad_() for k, v in leaves.items()}
        outs, loss = fn(ls)
        loss.backward()
        res.append({**{k: v.detach() for k, v in outs.items()}, **{"g_" + k: v.grad for k, v in ls.items()}})
    return res


@functools.lru_cache(maxsize=None)
def _batch(only=None):
    """(device batch, src, dst, gid, rev, in_eid) of the whole batch, or of its molecule `only` alone."""
    nn_, ne, src, dst = A.molecules()
    nn_, ne, src, dst = 2 * nn_ + HAND[0], 2 * ne + HAND[1], 2 * src + HAND[2], 2 * dst + HAND[3]
    if only is not None:
        e0 = sum(ne[:only])
        nn_, ne, src, dst = nn_[only:only + 1], ne[only:only + 1], src[e0:e0 + ne[only]], dst[e0:e0 + ne[only]]
    g = mvml_gat.from_arrays(nn_, ne, src, dst).to(DEV)
    src, dst, gid = A.global_ids(nn_, ne, src, dst)
    return g, src, dst, gid, R.rev_map(src, dst), g.in_eid.long().cpu()


def _slots(g, t):
    """A per-edge tensor in edge-id order -> in-CSR slot order on the device, rows pitched, NaN in the pad."""
    buf = torch.full((t.shape[0], t.shape[1] + 4), float("nan"), device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)[g.in_eid.long()]
    return buf[:, :t.shape[1]]


def _edges(g, t):
    """A per-slot device tensor -> edge-id order."""
    return torch.empty_like(t).index_copy_(0, g.in_eid.long(), t)


def test_rev_slots_equal_the_reference_map():
    g, src, dst, _, rev, eid = _batch()
    rs = Fn.dmpnn_rev_slots(g).cpu().long()
    got = torch.empty_like(rs).index_copy_(0, eid, torch.where(rs >= 0, eid[rs.clamp(min=0)], rs))
    E = len(rev)
    assert got.tolist() == rev and rev[-6:] == [E - 6, E - 3, E - 2, E - 5, E - 4, -1]


@pytest.mark.parametrize("D,De,bias", [(64, 1, False), (64, 14, True), (68, 32, False), (68, 14, True), (300, 14, False),
                                       (300, 32, True), (300, 1, True), (1024, 12, True), (1024, 13, False)])
def test_init_against_float64(D, De, bias):
    g, src, dst, _, _, _ = _batch()
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator().manual_seed(10 * D + De)
    rnd = lambda *s: torch.randn(s, generator=gen)
    lv = dict(x=rnd(N, FA), Wa=rnd(D, FA) / FA ** 0.5, We=rnd(D, De) / De ** 0.5, **({"b": rnd(D)} if bias else {}))
    e, gi, gm = rnd(E, De), rnd(E, D), rnd(E, D)

    def fn(l):
        dt = l["x"].dtype
        inp, M0 = R.init(src, l["x"], e.to(dt), torch.cat([l["Wa"], l["We"]], 1), l.get("b"))
        return {"input": inp, "M0": M0}, (inp * gi.to(dt)).sum() + (M0 * gm.to(dt)).sum()
    r64, r32 = _both(fn, lv)
    xb = torch.full((N, FA + 5), float("nan"), device=DEV)
    xb[:, :FA] = lv["x"].to(DEV)
    x = xb[:, :FA].detach().requires_grad_()
    W = torch.cat([lv["Wa"], lv["We"]], 1).to(DEV).requires_grad_()
    b = lv["b"].to(DEV).requires_grad_() if bias else None
    inp, M0 = Fn.DMPNNInitFunction.apply(x, e.to(DEV), g, W, b)
    torch.autograd.backward([inp, M0], [_slots(g, gi), _slots(g, gm)])
    torch.cuda.synchronize()
    got = {"input": _edges(g, inp.detach()), "M0": _edges(g, M0.detach()), "g_x": x.grad, "g_Wa": W.grad[:, :FA],
           "g_We": W.grad[:, FA:], **({"g_b": b.grad} if bias else {})}
    assert torch.equal(M0.detach(), inp.detach().clamp(min=0))
    _check(f"init D={D} De={De}", got, r64, r32)


def _step_inputs(D, bias, seed):
    g = _batch()[0]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen)
    lv = dict(R=rnd(g.num_edges(), D), input=rnd(g.num_edges(), D), **({"b_h": rnd(D)} if bias else {}))
    return lv, rnd(g.num_edges(), D)


def _gpu_step(g, lv, gs):
    """mvml_dmpnn_update and its adjoint on pitched slot rows; every quantity back in edge-id order."""
    D = gs.shape[1]
    b = lv["b_h"].to(DEV) if "b_h" in lv else None
    out = Fn.dmpnn_update(g, _slots(g, lv["R"]), _slots(g, lv["input"]), b)
    dR, dpre = Fn.dmpnn_update_bwd(g, out, _slots(g, gs))
    gb = torch.empty(D, device=DEV)
    Fn.colsum(dpre, out.shape[0], D, D, gb)
    torch.cuda.synchronize()
    return {"out": _edges(g, out), "g_R": _edges(g, dR), "g_input": _edges(g, dpre), **({"g_b_h": gb} if b is not None else {})}


@pytest.mark.parametrize("D,bias", [(64, True), (68, False), (300, True), (300, False)])
def test_update_step_against_float64(D, bias):
    g, src, dst, _, rev, _ = _batch()
    N, E = g.num_nodes(), g.num_edges()
    lv, gs = _step_inputs(D, bias, D)

    def fn(l):
        out = R.update(src, dst, rev, N, l["input"], l["R"], l.get("b_h"))
        return {"out": out}, (out * gs.to(out.dtype)).sum()
    r64, r32 = _both(fn, lv)
    got = _gpu_step(g, lv, gs)
    _check(f"update D={D}", got, r64, r32)
    # the hub atoms' out-edges on their own (70 in-slot rows summed, in chunks)
    deg = torch.bincount(dst, minlength=N)
    hub = torch.isin(src, torch.nonzero(deg == 70).flatten())
    assert int(hub.sum()) == 140
    _check(f"update D={D} hub rows", {"out": got["out"][hub]}, {"out": r64["out"][hub]}, {"out": r32["out"][hub]})
    # the one-way edge: its source atom has no in-edge (Q = 0) and it has no reverse, so out = relu(input + b_h)
    assert rev[E - 1] == -1 and int(deg[src[E - 1]]) == 0
    want = (lv["input"][E - 1] + lv["b_h"] if bias else lv["input"][E - 1]).clamp(min=0)
    assert torch.equal(got["out"][E - 1].cpu(), want)


def test_step_bits_do_not_depend_on_the_run_or_the_batch():
    g = _batch()[0]
    lv, gs = _step_inputs(300, True, 7)
    once, again = _gpu_step(g, lv, gs), _gpu_step(g, lv, gs)
    for k in once:
        assert torch.equal(_bits(once[k]), _bits(again[k])), k
    nn_, ne, _, _ = A.molecules()
    ring, e0 = _batch(2)[0], sum(ne[:2])  # the first copy's six-ring alone: edges e0 .. e0 + 12
    alone = _gpu_step(ring, {k: (v[e0:e0 + 12] if v.dim() == 2 else v) for k, v in lv.items()}, gs[e0:e0 + 12])
    for k in ("out", "g_R", "g_input"):
        assert torch.equal(_bits(alone[k]), _bits(once[k][e0:e0 + 12])), k


@pytest.mark.parametrize("D,depth,bias,aggregation", [(64, 1, False, "mean"), (68, 3, True, "sum"), (300, 3, False, "mean")])
def test_predictor_step_against_float64(D, depth, bias, aggregation):
    g, src, dst, gid, rev, _ = _batch()
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    torch.manual_seed(D + depth)
    model = DMPNNPredictor(FA, 14, hidden_size=D, depth=depth, bias=bias, aggregation=aggregation, ffn_hidden_size=32, n_tasks=3)
    keys = {"gnn.W_i.weight", "gnn.W_h.weight", "gnn.W_o.weight", "gnn.W_o.bias"} | ({"gnn.W_i.bias", "gnn.W_h.bias"} if bias else set())
    assert set(model.state_dict()) == keys | {f"predict.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")}
    assert isinstance(model.gnn, DMPNNGNN) and model.gnn.W_i.weight.shape == (D, FA + 14) and model.gnn.W_o.weight.shape == (D, FA + D)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if depth == 1:  # no update step: W_h takes no part and gets no gradient
        sd = {k: v for k, v in sd.items() if "W_h" not in k}
    x, e, y = torch.randn(N, FA), torch.randn(E, 14), (torch.rand(B, 3) < 0.5).float()

    def fn(l):
        dt = l["predict.2.bias"].dtype
        z = R.predictor(l, src, dst, rev, gid, B, x.to(dt), e.to(dt), depth, aggregation)
        return {"logits": z}, F.binary_cross_entropy_with_logits(z, y.to(dt))
    r64, r32 = _both(fn, sd)
    model = model.to(DEV).train()
    z = model(g, x.to(DEV), e.to(DEV))
    bce_with_logits(z, y.to(DEV)).backward()
    got = {"logits": z.detach(), **{"g_" + k: p.grad for k, p in model.named_parameters() if p.grad is not None}}
    assert sorted(got) == sorted(r64)
    _check(f"predictor D={D} depth={depth}", got, r64, r32)


@pytest.mark.parametrize("kw,match", [(dict(dropout=0.1), "inside the depth loop"), (dict(hidden_size=302), "multiple of 4"),
                                      (dict(hidden_size=1028), "at most 1024"), (dict(edge_in_feats=0), "bond features"),
                                      (dict(edge_in_feats=33), "bond features"), (dict(depth=0), "depth")])
def test_modules_refuse_what_the_kernels_do_not_hold(kw, match):
    with pytest.raises(ValueError, match=match):
        DMPNNGNN(**{**dict(node_in_feats=FA, edge_in_feats=14), **kw})


@pytest.mark.parametrize("D,De", [(302, 14), (1028, 14), (300, 33), (300, 0)])
def test_entries_refuse_other_shapes_before_any_launch(D, De):
    g = _batch()[0]
    N, E = g.num_nodes(), g.num_edges()
    buf = torch.zeros((E, 1040), device=DEV)
    L, st, p = lib(), stream_ptr(), ptr(buf)
    csr = (ptr(g.in_rowptr), ptr(g.out_rowptr), ptr(g.out_inslot), ptr(Fn.dmpnn_rev_slots(g)))
    rcs = [L.mvml_dmpnn_init_fwd(N, E, ptr(g.in_src), p, 1040, D, p, De, p, None, p, 1040, p, 1040, st)]
    if D != 300:
        rcs += [L.mvml_dmpnn_update(N, E, *csr, p, 1040, p, 1040, None, D, p, 1040, st),
                L.mvml_dmpnn_update_bwd(N, E, *csr, p, 1040, p, 1040, D, p, 1040, p, 1040, st),
                L.mvml_dmpnn_atom_sum(N, E, csr[0], None, p, 1040, D, p, 1040, st),
                L.mvml_dmpnn_atom_sum_bwd(N, E, csr[0], p, 1040, D, p, 1040, st)]
    torch.cuda.synchronize()
    assert set(rcs) == {1} and lib().mvml_last_error() and float(buf.abs().max()) == 0.0
