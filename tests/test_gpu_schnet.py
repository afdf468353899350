"""SchNet on the GPU against the float64 formulas of tests/_schnet_ref.py (the [E, K] expansion
materialised): the fused filter, aggregation, dW_1 and ssp kernels (csrc/schnet.hip) through the autograd
functions and the C ABI, then SchNetPredictor, weight-tied through its state_dict.

Batch: _afp_ref.molecules() twice, as tests/test_gpu_mpnn.py: 80 atoms and 428 edges, four 128-slot
tiles with the last one partial; per copy a single atom without in-edge (its aggregated row is exactly
0) and the 70-edge hub, whose second copy's rows cross a tile boundary (asserted).  Distances uniform in
[0, 1.1 cutoff] (some past every centre), one exactly 0 and one exactly on a centre.

Bar (the project's rule): the norm-wise conftest.rel_err <= max(1e-5, 4 e32) per quantity, e32 the same
formulas in float32 on the CPU against their float64 run; no entry is masked."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import _afp_ref as A
import _schnet_ref as R
import mvml_gat
from conftest import rel_err
from mvml_gat import SchNetGNN, SchNetPredictor
from mvml_gat import functional as Fn
from mvml_gat._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
TILE = 128  # csrc/schnet.hip kSnTile
KEYS = ({"gnn.embed.weight", "gnn.rbf.centers"} | {f"readout.{m}_project.{p}" for m in ("in", "out") for p in ("weight", "bias")})
LAYER = [f"{m}.{p}" for m in ("conv.project_edge.0", "conv.project_edge.2", "conv.project_node", "conv.project_out.0",
                              "project_out") for p in ("weight", "bias")]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(what, got, r64, r32):
    for k in r64:
        e, b = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        print(f"schnet {what} {k}: {e:.2e} / {b:.2e}")
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
    """(device batch, src, dst, gid, atom range, edge range) of the doubled batch or of molecule `only`."""
    nn_, ne, src, dst = A.molecules()
    nn_, ne, src, dst = 2 * nn_, 2 * ne, 2 * src, 2 * dst
    a0, e0 = sum(nn_[:only or 0]), sum(ne[:only or 0])
    if only is not None:
        src, dst = src[e0:e0 + ne[only]], dst[e0:e0 + ne[only]]
        nn_, ne = nn_[only:only + 1], ne[only:only + 1]
    g = mvml_gat.from_arrays(nn_, ne, src, dst).to(DEV)
    return (g, *A.global_ids(nn_, ne, src, dst), (a0, a0 + sum(nn_)), (e0, e0 + sum(ne)))


def _dists(E, centers, cutoff, gen):
    d = torch.rand(E, generator=gen) * 1.1 * cutoff
    if E:
        d[0], d[1] = 0.0, centers[len(centers) // 2]
    return d


def _inputs(Fw, H, cutoff, gap, seed):
    g = _batch()[0]
    N, E = g.num_nodes(), g.num_edges()
    rbf = mvml_gat.RBFExpansion(high=cutoff, gap=gap)
    K = rbf.centers.numel()
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen)
    lv = dict(hv=rnd(N, H), W1=rnd(H, K), b1=rnd(H), W2=rnd(H, H) / H ** 0.5, b2=rnd(H), Wo=rnd(Fw, H) / H ** 0.5, bo=rnd(Fw))
    return lv, _dists(E, rbf.centers, cutoff, gen), rnd(N, Fw), rbf


def _reference(lv, d, gs, rbf):
    _, src, dst, _, _, _ = _batch()

    def fn(l):
        dt = l["hv"].dtype
        he = R.filter(d.to(dt), rbf.centers.to(dt), rbf.gamma, l["W1"], l["b1"], l["W2"], l["b2"])
        a = R.cfconv(src, dst, l["hv"].shape[0], l["hv"], he)
        y = R.ssp(F.linear(a, l["Wo"], l["bo"]))
        return {"he": he, "a": a, "y": y}, (y * gs.to(dt)).sum()
    return _both(fn, lv)


def _gpu(g, lv, d, gs, rbf):
    """One CFConv after project_node through the autograd functions, hv on rows with a pitch past H; he in
    edge-id order.  Also returns what a second dW_1 call needs."""
    H = lv["hv"].shape[1]
    p = {k: v.to(DEV).requires_grad_() for k, v in lv.items() if k != "hv"}
    hb = torch.full((g.num_nodes(), H + 8), float("nan"), device=DEV)
    hb[:, :H] = lv["hv"].to(DEV)
    hv = hb[:, :H].detach().requires_grad_()
    link, dd, cen = Fn.CFConvLink(), d.to(DEV), rbf.centers.to(DEV)
    he = Fn.SchNetFilterFunction.apply(dd, cen, rbf.gamma, p["W1"], p["b1"], p["W2"], p["b2"], g, link)
    a = Fn.CFConvAggFunction.apply(hv, he, g, link)
    a.retain_grad()
    y = Fn.LinearSSPFunction.apply(a, p["Wo"], p["bo"])
    y.backward(gs.to(DEV), retain_graph=True)
    torch.cuda.synchronize()
    he_e = torch.empty_like(he).index_copy_(0, g.in_eid.long(), he.detach())
    got = {"he": he_e, "a": a.detach(), "y": y.detach(), "g_hv": hv.grad, **{"g_" + k: v.grad for k, v in p.items()}}
    return got, (he, a, hv.detach())


@pytest.mark.parametrize("Fw,H,cutoff,gap,K", [(16, 16, 0.1, 0.1, 1), (20, 48, 33.0, 1.0, 33), (64, 64, 30.0, 0.1, 300),
                                               (128, 128, 64.0, 0.125, 512)])
def test_kernels_against_float64(Fw, H, cutoff, gap, K):
    g = _batch()[0]
    N, E = g.num_nodes(), g.num_edges()
    rp = g.in_rowptr.cpu()
    hubs = [v for v in range(N) if int(rp[v + 1] - rp[v]) == 70]
    assert E > 3 * TILE and E % TILE and any(int(rp[v]) // TILE != int(rp[v + 1] - 1) // TILE for v in hubs)
    lv, d, gs, rbf = _inputs(Fw, H, cutoff, gap, 100 * Fw + H)
    assert rbf.centers.numel() == K and math.isclose(rbf.gamma, 1 / gap)
    assert float(d.max()) > cutoff and float(d[0]) == 0.0 and float(d[1]) == float(rbf.centers[K // 2])
    r64, r32 = _reference(lv, d, gs, rbf)
    got, (he, a, hv) = _gpu(g, lv, d, gs, rbf)
    assert int(rp[1]) == 0 and float(got["a"][0].abs().max()) == 0.0  # the single atom: no in-edge, exactly 0
    _check(f"F={Fw} H={H} K={K}", got, r64, r32)
    # dW_1 once more with the accumulate flag, onto a pre-filled buffer
    fn = he.grad_fn
    s1, _ = fn.saved_tensors
    _, dslot, ldd, cen, gamma, image, _, _, _ = fn.state
    dpre2, dpre1 = torch.empty_like(s1), torch.empty_like(s1)
    call("mvml_schnet_filter_bwd", E, ptr(g.in_src), ptr(Fn.nnconv_slot_dst(g)), ptr(a.grad), H, ptr(hv), hv.stride(0), ptr(s1), H,
         ptr(he), H, H, K, ptr(image), ptr(dpre2), H, ptr(dpre1), H, stream_ptr())
    base = torch.randn((H, K), generator=torch.Generator().manual_seed(1))
    acc = Fn.schnet_dw1(dslot, ldd, cen, gamma, dpre1, E, H, K, base.to(DEV), accumulate=True)
    torch.cuda.synchronize()
    _check(f"accumulate H={H} K={K}", {"g_W1": acc}, *({"g_W1": r["g_W1"] + base.to(r["g_W1"].dtype)} for r in (r64, r32)))


def test_bits_do_not_depend_on_the_batch_or_the_run():
    g = _batch()[0]
    lv, d, gs, rbf = _inputs(64, 64, 30.0, 0.1, 7)
    (once, (he, a, _)), (again, _) = _gpu(g, lv, d, gs, rbf), _gpu(g, lv, d, gs, rbf)
    for k in once:
        assert torch.equal(_bits(once[k]), _bits(again[k])), k
    one, _, _, _, (a0, a1), (e0, e1) = _batch(8)  # the second copy's hub molecule alone
    cen, link = rbf.centers.to(DEV), Fn.CFConvLink()
    w = [lv[k].to(DEV) for k in ("W1", "b1", "W2", "b2")]
    he1 = Fn.SchNetFilterFunction.apply(d[e0:e1].to(DEV), cen, rbf.gamma, *w, one, link)
    a1_ = Fn.CFConvAggFunction.apply(lv["hv"][a0:a1].to(DEV), he1, one, link)
    rp = g.in_rowptr.cpu()
    assert torch.equal(_bits(he1), _bits(he.detach()[int(rp[a0]):int(rp[a1])]))
    assert torch.equal(_bits(a1_), _bits(a.detach()[a0:a1]))


@pytest.mark.parametrize("H,K", [(20, 300), (144, 300), (64, 513), (64, 0)])
def test_refuses_other_shapes_before_any_launch(H, K):
    g = _batch()[0]
    buf = torch.zeros((g.num_edges(), 512), device=DEV)
    L, st, N, E, b = lib(), stream_ptr(), g.num_nodes(), g.num_edges(), ptr(buf)
    rcs = [L.mvml_schnet_split_w(H, K, b, b, b, st),
           L.mvml_schnet_filter_fwd(E, b, 1, b, K, 10.0, H, b, b, b, b, 512, b, 512, st),
           L.mvml_schnet_filter_bwd(E, ptr(g.in_src), ptr(g.in_src), b, 512, b, 512, b, 512, b, 512, H, K, b, b, 512, b, 512,
                                    st),
           L.mvml_schnet_dw1(E, b, 1, b, K, 10.0, b, 512, H, 0, b, b, buf.numel() * 4, st)]
    if H % 16 or H > 128:  # (the aggregation takes no K)
        rcs.append(L.mvml_cfconv_agg(N, E, ptr(g.in_rowptr), None, ptr(g.in_src), b, 512, b, 512, H, b, 512, st))
    torch.cuda.synchronize()
    assert set(rcs) == {1} and lib().mvml_last_error() and float(buf.abs().max()) == 0.0
    assert L.mvml_schnet_image_bytes(H, K) == 0


def _predictor_case(model, g, src, dst, gid, what):
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cen = sd.pop("gnn.rbf.centers")
    gen = torch.Generator().manual_seed(3)
    types = torch.randint(0, sd["gnn.embed.weight"].shape[0], (N,), generator=gen)
    d, y = _dists(E, cen, float(cen[-1]) if len(cen) > 1 else 0.1, gen), torch.randn((B, 3), generator=gen)

    def fn(l):
        dt = l["readout.out_project.bias"].dtype
        z = R.predictor({**l, "gnn.rbf.centers": cen}, src, dst, gid, B, types, d.to(dt), model.gnn.rbf.gamma)
        return {"logits": z}, F.mse_loss(z, y.to(dt))
    r64, r32 = _both(fn, sd)
    model = model.to(DEV).train()
    z = model(g, types.to(DEV, torch.int32), d.to(DEV).view(-1, 1))
    F.mse_loss(z, y.to(DEV)).backward()
    assert model.gnn.rbf.centers.grad is None and not model.gnn.rbf.centers.requires_grad
    got = {"logits": z.detach(), **{"g_" + k: p.grad for k, p in model.named_parameters()}}
    assert sorted(got) == sorted(r64)
    _check(what, got, r64, r32)


@pytest.mark.parametrize("kw", [dict(node_feats=16, hidden_feats=[16], cutoff=4.0, gap=0.5),
                                dict(node_feats=64, hidden_feats=[64, 64, 64], cutoff=30.0, gap=0.1)])
def test_predictor_step_against_float64(kw):
    g, src, dst, gid, _, _ = _batch()
    torch.manual_seed(kw["node_feats"])
    model = SchNetPredictor(n_tasks=3, **kw)
    L = len(kw["hidden_feats"])
    assert set(model.state_dict()) == KEYS | {f"gnn.gnn_layers.{i}.{k}" for i in range(L) for k in LAYER}
    _predictor_case(model, g, src, dst, gid, f"predictor {kw['node_feats']} x {L}")


def test_a_batch_without_any_bond():
    """Three one-atom molecules: E = 0, empty edge arrays; every aggregated row is zero."""
    g = mvml_gat.from_arrays([1, 1, 1], [0, 0, 0], [], []).to(DEV)
    none = torch.zeros(0, dtype=torch.long)
    a = Fn.cfconv_agg(g, torch.randn((3, 16), device=DEV), torch.empty((0, 16), device=DEV))
    assert float(a.abs().max()) == 0.0
    torch.manual_seed(5)
    model = SchNetPredictor(node_feats=16, hidden_feats=[16, 16], n_tasks=3, cutoff=4.0, gap=0.5)
    _predictor_case(model, g, none, none, torch.arange(3), "no bonds")


def test_constructors_refuse_what_the_kernels_do_not_hold():
    with pytest.raises(ValueError, match="hidden_feats"):
        SchNetGNN(hidden_feats=[20])
    with pytest.raises(ValueError, match="cutoff / gap"):
        SchNetPredictor(cutoff=513.0, gap=1.0)
    with pytest.raises(ValueError, match="gap"):
        SchNetGNN(gap=0.0)
