"""AttentiveFP on the GPU against the float64 formulas of tests/_afp_ref.py: the context kernel pair
(csrc/afp_agg.hip), the GRU cell (csrc/gru.hip) and the attention pool (csrc/attn_pool.hip) through
the C ABI, then AttentiveFPPredictor, weight-tied through its state_dict.

Batch: _afp_ref.molecules(), 40 atoms: a single atom (no in-edge), a two-atom molecule, a six-ring,
a 12-atom molecule whose atom 0 has 70 in- and 70 out-edges (past the 64-entry id chunks of every
kernel and the 16-entry ones of the four-atoms-per-wave form) and a 19-atom chain with two rings.
Widths: 4; 64 and 68 (the last width of the four-atoms-per-wave forward and the first past it);
200; 1024 (four float4 slots per lane; with De = 32 past the LDS budget: the L2 path).

Bar (the project's rule, as tests/test_gpu_gin_agg.py and tests/test_gpu_gin.py): the norm-wise
relative error max|a - b| / max|b| (conftest.rel_err's) <= max(1e-5, 4 e32) per quantity, e32 the
same formulas in float32 on the CPU against their float64 run.  Norm-wise: no gradient entry is
masked out.  Quantities that need more than 1e-5 (measured error / bound; DESIGN.md, "AttentiveFP", has
the table): the context cases' g_t, a sum that vanishes where a row's LeakyReLU sides agree (G=4: 9.2e-3 /
2.2, G=68: 3.3e-4 / 0.67, G=200 De=10: 1.8e-5 / 2.5e-4, G=1024: 2.0e-5 / 1.4e-4 and 2.6e3 / 3.9e5);
context G=64 g_w2e 1.4e-5 / 3.6e-5; context G=1024 De=32 g_P 2.3e-5 / 4.0e-5, g_W1e 1.4e-5 / 4.3e-5,
g_b1 1.2e-5 / 3.7e-5, g_w2e 1.6e-5 / 4.7e-5; the predictor's compute_logits.0.bias gradient, vanishing
likewise (4.6e8 / 2.9e9, 9.4e8 / 1.8e10, 2.4e7 / 3.8e8 of a 1e-20 reference); L=3 T=2 G=200
gnn_layers.1.project_edge.1.bias 1.3e-5 / 6.4e-5."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _afp_ref as R
import mvml_gat
from conftest import rel_err
from mvml_gat import AttentiveFPPredictor, bce_with_logits
from mvml_gat._lib import lib, ptr, stream_ptr, ws_ptr_size

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
KEYS = """gnn.init_context.project_node.0 gnn.init_context.project_edge1.0 gnn.init_context.project_edge2.1
gnn.init_context.attentive_gru.edge_transform.1 gnn.init_context.attentive_gru.gru
gnn.gnn_layers.{i}.project_edge.1 gnn.gnn_layers.{i}.attentive_gru.project_node.1 gnn.gnn_layers.{i}.attentive_gru.gru
gnn.gnn_layers.{i}.bn_layer readout.readouts.{t}.compute_logits.0 readout.readouts.{t}.project_nodes.1
readout.readouts.{t}.gru predict.1""".split()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(what, got, r64, r32):
    for k in r64:
        e, b = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        print(f"afp {what} {k}: {e:.2e} / {b:.2e}")
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
    """(device batch, src, dst, gid, atom range, edge range) of the whole batch or of molecule `only`."""
    nn_, ne, src, dst = R.molecules()
    a0, e0 = sum(nn_[:only or 0]), sum(ne[:only or 0])
    if only is not None:
        src, dst = src[e0:e0 + ne[only]], dst[e0:e0 + ne[only]]
        nn_, ne = nn_[only:only + 1], ne[only:only + 1]
    g = mvml_gat.from_arrays(nn_, ne, src, dst).to(DEV)
    return (g, *R.global_ids(nn_, ne, src, dst), (a0, a0 + sum(nn_)), (e0, e0 + sum(ne)))


# ---- the context kernel pair ----------------------------------------------------------------------
def _context_inputs(G, De, seed):
    g, src, dst, _, _, _ = _batch()
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen)
    # logits of spread > 80 inside the hub's row at every width from 64: w2e . he1 has a standard deviation of about 64
    # (G = 4 is exempt: four terms do not reach it; that case is about the single column slot)
    return dict(P=rnd(N, G), t=rnd(N), W1e=rnd(G, De) / De ** 0.5, b1=rnd(G), w2e=rnd(G) * 64 / G ** 0.5), rnd(E, De), rnd(N, G)


def _context_gpu(g, lv, e, gs, backward=True):
    N, E, (G, De) = g.num_nodes(), g.num_edges(), lv["W1e"].shape
    d = {k: v.to(DEV) for k, v in lv.items()}
    P = torch.full((N, G + 8), float("nan"), device=DEV)  # a row pitch past G
    P[:, :G] = d["P"]
    W1eT, ed, st = d["W1e"].t().contiguous(), e.to(DEV), stream_ptr()
    rows = torch.empty((E, (De + 3) // 4 * 4), device=DEV)
    s, attn = torch.empty((N, G), device=DEV), torch.empty(E, device=DEV)
    assert lib().mvml_afp_edge_rows(E, De, ptr(g.in_eid), ptr(ed), De, ptr(rows), st) == 0
    assert torch.equal(rows[:, :De], ed[g.in_eid.long()]) and float(rows[:, De:].abs().sum()) == 0.0
    rc = lib().mvml_afp_context_fwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(P), G + 8, G, ptr(rows), De, ptr(W1eT),
                                    ptr(d["b1"]), ptr(d["w2e"]), ptr(d["t"]), ptr(s), G, ptr(attn), st)
    assert rc == 0, lib().mvml_last_error()
    out = {"s": s, "a": torch.empty(E, device=DEV).index_copy_(0, g.in_eid.long(), attn)}  # edge-id order
    if backward:
        gP, g_t = torch.empty((N, G), device=DEV), torch.empty(N, device=DEV)
        g_w2e, g_w1b = torch.empty(G, device=DEV), torch.empty((De + 1, G), device=DEV)
        wp, wn = ws_ptr_size(lib().mvml_afp_context_bwd_workspace_size(N, E, G, De), DEV)
        gsd = gs.to(DEV)
        rc = lib().mvml_afp_context_bwd(N, E, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
                                        ptr(g.out_inslot), ptr(P), G + 8, G, ptr(rows), De, ptr(W1eT), ptr(d["b1"]),
                                        ptr(d["w2e"]), ptr(d["t"]), ptr(s), G, ptr(attn), ptr(gsd), G, ptr(gP), G, ptr(g_t),
                                        ptr(g_w2e), ptr(g_w1b), wp, wn, st)
        assert rc == 0, lib().mvml_last_error()
        out.update(g_P=gP, g_t=g_t, g_w2e=g_w2e, g_W1e=g_w1b[:De].t(), g_b1=g_w1b[De])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("G,De", [(4, 1), (64, 10), (68, 10), (200, 1), (200, 10), (200, 32), (1024, 10), (1024, 32)])
def test_context_kernels_against_float64(G, De):
    g, src, dst, _, _, _ = _batch()
    N = g.num_nodes()
    lv, e, gs = _context_inputs(G, De, 10 * G + De)

    def fn(l):
        s, a = R.context_sum(src, dst, N, l["P"], e.to(l["P"].dtype), l["W1e"], l["b1"], l["w2e"], l["t"])
        return {"s": s, "a": a}, (s * gs.to(s.dtype)).sum()
    r64, r32 = _both(fn, lv)
    lg = F.leaky_relu(lv["t"][dst].double() + F.leaky_relu(lv["P"][src].double() + e.double() @ lv["W1e"].double().T
                                                            + lv["b1"].double()) @ lv["w2e"].double())
    hub = dst == int(torch.bincount(dst).argmax())
    assert G == 4 or float(lg[hub].max() - lg[hub].min()) > 80  # the online softmax rescales there
    got = _context_gpu(g, lv, e, gs)
    assert float(got["s"][0].abs().max()) == 0.0  # the single atom: no in-edge, a zero row
    _check(f"context G={G} De={De}", got, r64, r32)


def test_context_bits_do_not_depend_on_the_batch_or_the_run():
    g, _, _, _, _, _ = _batch()
    lv, e, gs = _context_inputs(200, 10, 7)
    whole, again = _context_gpu(g, lv, e, gs), _context_gpu(g, lv, e, gs)
    for k in whole:
        assert torch.equal(_bits(whole[k]), _bits(again[k])), k
    one, _, _, _, (a0, a1), (e0, e1) = _batch(3)  # the hub molecule alone
    alone = _context_gpu(one, {**lv, "P": lv["P"][a0:a1], "t": lv["t"][a0:a1]}, e[e0:e1], gs[a0:a1], backward=False)
    assert torch.equal(_bits(alone["s"]), _bits(whole["s"][a0:a1])) and torch.equal(_bits(alone["a"]), _bits(whole["a"][e0:e1]))


@pytest.mark.parametrize("G,De", [(1028, 10), (6, 10), (200, 33), (200, 0)])
def test_context_refuses_other_shapes_before_any_launch(G, De):
    g, _, _, _, _, _ = _batch()
    buf = torch.zeros((g.num_nodes(), 1040), device=DEV)
    rc = lib().mvml_afp_context_fwd(g.num_nodes(), ptr(g.in_rowptr), ptr(g.in_src), ptr(buf), 1040, G, ptr(buf), De, ptr(buf),
                                    ptr(buf), ptr(buf), ptr(buf), ptr(buf), 1040, ptr(buf), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 1 and lib().mvml_last_error() and float(buf.abs().max()) == 0.0


# ---- the GRU cell ---------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("M", [1, 67])
@pytest.mark.parametrize("D", [4, 200, 1024])
def test_gru_cell_against_float64(D, M, relu):
    gen = torch.Generator().manual_seed(D + M)
    rnd = lambda *s: torch.randn(s, generator=gen)
    lv = dict(gi=rnd(M, 3 * D), gh=rnd(M, 3 * D), h=rnd(M, D))
    bih, bhh, go = rnd(3 * D), rnd(3 * D), rnd(M, D)

    def fn(l):
        dt = l["h"].dtype
        out = R.gru_gates(l["gi"], l["gh"], bih.to(dt), bhh.to(dt), l["h"])
        out = F.relu(out) if relu else out
        return {"out": out}, (out * go.to(dt)).sum()
    r64, r32 = _both(fn, lv)
    d = {k: v.to(DEV) for k, v in lv.items()}
    out, save = torch.empty((M, D), device=DEV), torch.empty((M, 4 * D), device=DEV)
    st = stream_ptr()
    bi, bh = bih.to(DEV), bhh.to(DEV)
    rc = lib().mvml_gru_cell_fwd(M, D, ptr(d["gi"]), ptr(d["gh"]), ptr(bi), ptr(bh), ptr(d["h"]), D, relu,
                                 ptr(out), D, ptr(save), st)
    assert rc == 0, lib().mvml_last_error()
    g_gi, g_gh, g_h, god = torch.empty((M, 3 * D), device=DEV), torch.empty((M, 3 * D), device=DEV), torch.empty((M, D), device=DEV), go.to(DEV)
    rc = lib().mvml_gru_cell_bwd(M, D, ptr(save), ptr(d["h"]), D, ptr(out), D, ptr(god), D, relu, ptr(g_gi), ptr(g_gh),
                                 ptr(g_h), D, st)
    torch.cuda.synchronize()
    assert rc == 0, lib().mvml_last_error()
    if relu:  # outputs exactly on the ReLU's zero side, where the reference has them
        assert bool((out == 0).any()) and torch.equal((out == 0).cpu(), r64["out"] == 0)
    _check(f"gru D={D} M={M} relu={relu}", {"out": out, "g_gi": g_gi, "g_gh": g_gh, "g_h": g_h}, r64, r32)


# ---- the attention pool ---------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("D", [4, 200, 1024])
def test_attn_pool_against_float64(D, acc):
    sizes = [1, 2, 65, 300]
    B, N = len(sizes), sum(sizes)
    gid = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    offs = torch.tensor([0] + sizes).cumsum(0).to(DEV)
    gen = torch.Generator().manual_seed(D)
    rnd = lambda *s: torch.randn(s, generator=gen)
    lv = dict(X=rnd(N, D), wn=rnd(D) * 4 / D ** 0.5, u=rnd(B))
    gr, base = rnd(B, D), rnd(N, D)

    def fn(l):
        r, a = R.attn_pool(gid, B, l["X"], l["wn"], l["u"])
        return {"r": r, "a": a}, (r * gr.to(r.dtype)).sum()
    r64, r32 = _both(fn, lv)
    for r in (r64, r32):
        r["g_X"] = r["g_X"] + acc * base.to(r["g_X"].dtype)
    d = {k: v.to(DEV) for k, v in lv.items()}
    r, a, st = torch.empty((B, D), device=DEV), torch.empty(N, device=DEV), stream_ptr()
    rc = lib().mvml_attn_pool_fwd(B, N, D, ptr(offs), ptr(d["X"]), D, ptr(d["wn"]), ptr(d["u"]), 0.01, ptr(r), D, ptr(a), st)
    assert rc == 0, lib().mvml_last_error()
    gX, g_u, g_wn, grd = base.to(DEV).clone(), torch.empty(B, device=DEV), torch.empty(D, device=DEV), gr.to(DEV)
    wp, wn = ws_ptr_size(lib().mvml_attn_pool_bwd_workspace_size(B, N, D), DEV)
    rc = lib().mvml_attn_pool_bwd(B, N, D, ptr(offs), ptr(d["X"]), D, ptr(d["wn"]), ptr(d["u"]), 0.01, ptr(r), D, ptr(a),
                                  ptr(grd), D, acc, ptr(gX), D, ptr(g_u), ptr(g_wn), wp, wn, st)
    torch.cuda.synchronize()
    assert rc == 0, lib().mvml_last_error()
    _check(f"attn_pool D={D} acc={acc}", {"r": r, "a": a, "g_X": gX, "g_u": g_u, "g_wn": g_wn}, r64, r32)


# ---- the whole model ------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [16, 200])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("L", [1, 3])
def test_predictor_step_against_float64(L, T, G):
    g, src, dst, gid, _, _ = _batch()
    N, E, B, Fn_, De = g.num_nodes(), g.num_edges(), g.batch_size, 39, 10
    torch.manual_seed(100 * L + 10 * T + G)
    model = AttentiveFPPredictor(Fn_, De, num_layers=L, num_timesteps=T, graph_feat_size=G, n_tasks=3)
    want = set()
    for k in KEYS:
        want |= {k.format(i=i, t=t) for i in range(L - 1 if "{i}" in k else 1) for t in range(T)}
    assert {k.rsplit(".", 1)[0] for k in model.state_dict()} == want
    sd = {k: v.detach().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    x, e, y = torch.randn(N, Fn_), torch.randn(E, De), (torch.rand(B, 3) < 0.5).float()

    def fn(l):
        dt = l["predict.1.bias"].dtype
        z = R.predictor(l, src, dst, gid, B, x.to(dt), e.to(dt), L, T)
        return {"logits": z}, F.binary_cross_entropy_with_logits(z, y.to(dt))
    r64, r32 = _both(fn, sd)
    drop = [k for k in r64 if k.startswith("g_") and ("running_" in k or r64[k] is None)]  # BatchNorm's buffers
    for r in (r64, r32):
        for k in drop:
            del r[k]
    model = model.to(DEV).train()
    z = model(g, x.to(DEV), e.to(DEV))
    bce_with_logits(z, y.to(DEV)).backward()
    got = {"logits": z.detach(), **{"g_" + k: p.grad for k, p in model.named_parameters()}}
    assert sorted(got) == sorted(r64)
    # (a logit Linear's bias shifts the logits of a softmax alike, so where the LeakyReLU sides agree its
    # gradient is rounding noise on both sides: noise against noise under the same bar, as test_gpu_gin.py's)
    _check(f"predictor L={L} T={T} G={G}", got, r64, r32)


def test_a_batch_without_any_bond():
    """Three one-atom molecules: E = 0, empty edge arrays; every context row is zero before the GRU."""
    g = mvml_gat.from_arrays([1, 1, 1], [0, 0, 0], [], []).to(DEV)
    none, gid = torch.zeros(0, dtype=torch.long), torch.arange(3)
    torch.manual_seed(5)
    model = AttentiveFPPredictor(39, 10, num_layers=2, num_timesteps=1, graph_feat_size=16, n_tasks=2)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point and "running_" not in k}
    x, e, y = torch.randn(3, 39), torch.zeros(0, 10), torch.tensor([[0., 1.], [1., 1.], [0., 0.]])

    def fn(l):
        dt = l["predict.1.bias"].dtype
        z = R.predictor(l, none, none, gid, 3, x.to(dt), e.to(dt), 2, 1)
        return {"logits": z}, F.binary_cross_entropy_with_logits(z, y.to(dt))
    r64, r32 = _both(fn, sd)
    model = model.to(DEV).train()
    z = model(g, x.to(DEV), e.to(DEV))
    bce_with_logits(z, y.to(DEV)).backward()
    _check("no bonds", {"logits": z.detach(), **{"g_" + k: p.grad for k, p in model.named_parameters()}}, r64, r32)


def test_predictor_refuses_what_the_kernels_do_not_hold():
    with pytest.raises(ValueError, match="dropout"):
        AttentiveFPPredictor(39, 10, dropout=0.1)
    with pytest.raises(ValueError, match="graph_feat_size"):
        AttentiveFPPredictor(39, 10, graph_feat_size=1028)
    with pytest.raises(ValueError, match="bond features"):
        AttentiveFPPredictor(39, 33)
