"""MPNN on the GPU against the float64 formulas of tests/_mpnn_ref.py (the per-edge matrices
materialised): the NNConv kernels (csrc/nnconv.hip) through Fn.NNConvFunction and the C ABI, then
MPNNPredictor, weight-tied through its state_dict.

Batch: _afp_ref.molecules() twice, 80 atoms and 428 edges: four 128-slot edge tiles, the last one
partial (44 slots).  Per copy a single atom (no in-edge: its NNConv row is exactly bias), a two-atom
molecule, a six-ring, the hub with 70 in- and out-edges and a 19-atom chain with two rings; the second
copy's hub row spans slots 228..297, across the tile boundary at 256 (asserted).

Bar (the project's rule, as tests/test_gpu_afp.py): the norm-wise relative error max|a - b| / max|b|
(conftest.rel_err's) <= max(1e-5, 4 e32) per quantity, e32 the same formulas in float32 on the CPU
against their float64 run.  Norm-wise: no entry is masked."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _afp_ref as A
import _mpnn_ref as R
import mvml_gat
from conftest import rel_err
from mvml_gat import MPNNGNN, MPNNPredictor, NNConv, bce_with_logits
from mvml_gat import functional as Fn
from mvml_gat._lib import lib, ptr, stream_ptr, ws_ptr_size

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
TILE = 128  # csrc/nnconv.hip kNnTile
KEYS = {f"gnn.{k}" for k in ("project_node_feats.0.weight", "project_node_feats.0.bias", "gnn_layer.bias",
                             "gnn_layer.edge_func.0.weight", "gnn_layer.edge_func.0.bias", "gnn_layer.edge_func.2.weight",
                             "gnn_layer.edge_func.2.bias", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0",
                             "gru.bias_hh_l0")} | {f"predict.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(what, got, r64, r32):
    for k in r64:
        e, b = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        print(f"mpnn {what} {k}: {e:.2e} / {b:.2e}")
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
    e1 = len(src)
    nn_, ne, src, dst = 2 * nn_, 2 * ne, 2 * src, 2 * dst
    a0, e0 = sum(nn_[:only or 0]), sum(ne[:only or 0])
    if only is not None:
        src, dst = src[e0:e0 + ne[only]], dst[e0:e0 + ne[only]]
        nn_, ne = nn_[only:only + 1], ne[only:only + 1]
    g = mvml_gat.from_arrays(nn_, ne, src, dst).to(DEV)
    return (g, *A.global_ids(nn_, ne, src, dst), (a0, a0 + sum(nn_)), (e0, e0 + sum(ne)))


def _inputs(D, H, De, seed):
    g = _batch()[0]
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen)
    lv = dict(h=rnd(N, D), W1=rnd(H, De) / De ** 0.5, b1=rnd(H), W2=rnd(D * D, H) / (D * H) ** 0.5, b2=rnd(D * D) / D ** 0.5,
              bias=rnd(D))
    return lv, rnd(E, De), rnd(N, D)


def _reference(lv, e, gs):
    _, src, dst, _, _, _ = _batch()
    zs = []

    def fn(l):
        dt = l["h"].dtype
        z = F.relu(e.to(dt) @ l["W1"].T + l["b1"])
        z.retain_grad()
        zs.append(z)
        out = R.nnconv(src, dst, l["h"].shape[0], l["h"], z, l["W2"], l["b2"], l["bias"])
        return {"out": out}, (out * gs.to(dt)).sum()
    res = _both(fn, lv)
    for r, z in zip(res, zs):
        r["g_z"] = z.grad
    return res


def _gpu(g, lv, e, gs):
    """NNConvFunction (a step of its own) on h with a row pitch past D; every quantity in edge-id order."""
    D = lv["h"].shape[1]
    d = {k: v.to(DEV).requires_grad_() for k, v in lv.items() if k != "h"}
    hb = torch.full((g.num_nodes(), D + 8), float("nan"), device=DEV)
    hb[:, :D] = lv["h"].to(DEV)
    h = hb[:, :D].detach().requires_grad_()
    z = Fn.EdgeNetworkFunction.apply(e.to(DEV), g, d["W1"], d["b1"])
    z.retain_grad()
    out = Fn.NNConvFunction.apply(h, z, d["W2"], d["b2"], d["bias"], g, False, None)
    out.backward(gs.to(DEV))
    torch.cuda.synchronize()
    eid = g.in_eid.long()
    return {"out": out.detach(), "g_h": h.grad, "g_z": torch.empty_like(z.grad).index_copy_(0, eid, z.grad),
            **{"g_" + k: v.grad for k, v in d.items()}}, (h, z.detach(), d)


@pytest.mark.parametrize("D,H,De", [(16, 16, 1), (48, 80, 10), (64, 128, 10), (128, 256, 32)])
def test_nnconv_kernels_against_float64(D, H, De):
    g = _batch()[0]
    N, E = g.num_nodes(), g.num_edges()
    rp = g.in_rowptr.cpu()
    hubs = [v for v in range(N) if int(rp[v + 1] - rp[v]) == 70]
    assert E > 3 * TILE and E % TILE and any(int(rp[v]) // TILE != int(rp[v + 1] - 1) // TILE for v in hubs)
    lv, e, gs = _inputs(D, H, De, 100 * D + H + De)
    r64, r32 = _reference(lv, e, gs)
    got, (h, z, d) = _gpu(g, lv, e, gs)
    assert torch.equal(got["out"][0].cpu(), lv["bias"])  # the single atom: no in-edge, exactly bias
    _check(f"nnconv D={D} H={H} De={De}", got, r64, r32)
    # once more with the accumulate flag, onto pre-filled buffers
    gen = torch.Generator().manual_seed(1)
    base = dict(g_z=torch.randn((E, H), generator=gen), g_W2=torch.randn((D * D, H), generator=gen),
                g_b2=torch.randn(D * D, generator=gen), g_bias=torch.randn(D, generator=gen))
    acc = Fn.NNConvShared(Fn.nnconv_image(d["W2"].detach(), D, H), 1)
    acc.dz, acc.dW2, acc.db2, acc.dbias = (base[k].to(DEV) for k in ("g_z", "g_W2", "g_b2", "g_bias"))
    eid = g.in_eid.long()
    acc.dz = acc.dz[eid].contiguous()
    out, S = Fn.nnconv_forward(g, h.detach(), z, d["b2"].detach(), d["bias"].detach(), acc.image, False)
    Fn.nnconv_backward(g, h.detach(), z, d["b2"].detach(), acc.image, S, out, gs.to(DEV), False, acc, True)
    torch.cuda.synchronize()
    got2 = {"g_z": torch.empty_like(acc.dz).index_copy_(0, eid, acc.dz), "g_W2": acc.dW2, "g_b2": acc.db2, "g_bias": acc.dbias}
    _check(f"nnconv accumulate D={D} H={H}", got2, *({k: r[k] + base[k].to(r[k].dtype) for k in got2} for r in (r64, r32)))


def _forward_rows(g, h, z_edge, W2):
    """mvml_nnconv_fwd alone (no bias, no b2 part) on z given in edge-id order."""
    (N, D), H = h.shape, z_edge.shape[1]
    hd, zd = h.to(DEV), z_edge.to(DEV)[g.in_eid.long()].contiguous()
    img, out = Fn.nnconv_image(W2.to(DEV), D, H), torch.empty((N, D), device=DEV)
    wp, wn = ws_ptr_size(lib().mvml_nnconv_fwd_workspace_size(g.num_edges(), D), DEV)
    rc = lib().mvml_nnconv_fwd(N, g.num_edges(), ptr(g.in_rowptr), ptr(g.in_src), ptr(hd), D, D, ptr(zd), H, H, ptr(img),
                               None, ptr(out), D, wp, wn, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().mvml_last_error()
    return out


def test_nnconv_bits_do_not_depend_on_the_batch_or_the_run():
    g = _batch()[0]
    lv, e, gs = _inputs(64, 128, 10, 7)
    once, again = _gpu(g, lv, e, gs)[0], _gpu(g, lv, e, gs)[0]
    for k in once:
        assert torch.equal(_bits(once[k]), _bits(again[k])), k
    one, _, _, _, (a0, a1), (e0, e1) = _batch(8)  # the second copy's hub molecule alone
    z = F.relu(e @ lv["W1"].T + lv["b1"])
    whole, alone = _forward_rows(g, lv["h"], z, lv["W2"]), _forward_rows(one, lv["h"][a0:a1], z[e0:e1], lv["W2"])
    assert torch.equal(_bits(alone), _bits(whole[a0:a1]))


@pytest.mark.parametrize("D,H", [(20, 128), (144, 128), (64, 272)])
def test_nnconv_refuses_other_shapes_before_any_launch(D, H):
    g = _batch()[0]
    buf = torch.zeros((g.num_edges(), 512), device=DEV)
    L, st, N, E = lib(), stream_ptr(), g.num_nodes(), g.num_edges()
    rcs = [L.mvml_nnconv_fwd(N, E, ptr(g.in_rowptr), ptr(g.in_src), ptr(buf), 512, D, ptr(buf), 512, H, ptr(buf), None,
                             ptr(buf), 512, ptr(buf), buf.numel() * 4, st),
           L.mvml_nnconv_bwd_data(N, E, ptr(g.in_src), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_inslot), ptr(buf), 512, D,
                                  ptr(buf), 512, H, ptr(buf), ptr(buf), 512, 0, ptr(buf), 512, ptr(buf), 512, ptr(buf),
                                  buf.numel() * 4, st),
           L.mvml_nnconv_bwd_weight(E, ptr(g.in_src), ptr(g.in_src), ptr(buf), 512, D, ptr(buf), 512, H, ptr(buf), 512, 0,
                                    ptr(buf), ptr(buf), buf.numel() * 4, st),
           L.mvml_nnconv_split_w2(D, H, ptr(buf), ptr(buf), st)]
    torch.cuda.synchronize()
    assert rcs == [1, 1, 1, 1] and lib().mvml_last_error() and float(buf.abs().max()) == 0.0
    assert L.mvml_nnconv_image_bytes(D, H) == 0


def _predictor_case(model, g, src, dst, gid, steps, T, L, what):
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x, e, y = torch.randn(N, 39), torch.randn(E, 10), (torch.rand(B, 3) < 0.5).float()

    def fn(l):
        dt = l["predict.2.bias"].dtype
        z = R.predictor(l, src, dst, gid, B, x.to(dt), e.to(dt), steps, T, L)
        return {"logits": z}, F.binary_cross_entropy_with_logits(z, y.to(dt))
    r64, r32 = _both(fn, sd)
    model = model.to(DEV).train()
    z = model(g, x.to(DEV), e.to(DEV))
    bce_with_logits(z, y.to(DEV)).backward()
    got = {"logits": z.detach(), **{"g_" + k: p.grad for k, p in model.named_parameters()}}
    assert sorted(got) == sorted(r64)
    _check(what, got, r64, r32)


@pytest.mark.parametrize("D,H,steps,T,L", [(16, 16, 1, 2, 2), (64, 128, 3, 6, 3)])
def test_predictor_step_against_float64(D, H, steps, T, L):
    g, src, dst, gid, _, _ = _batch()
    torch.manual_seed(D + steps)
    kw = {} if L == 3 else dict(num_step_set2set=T, num_layer_set2set=L)
    model = MPNNPredictor(39, 10, node_out_feats=D, edge_hidden_feats=H, n_tasks=3, num_step_message_passing=steps, **kw)
    lstm = {f"readout.lstm.{k}_{p}_l{l}" for k in ("weight", "bias") for p in ("ih", "hh") for l in range(L)}
    assert set(model.state_dict()) == KEYS | lstm
    _predictor_case(model, g, src, dst, gid, steps, T, L, f"predictor D={D} H={H} steps={steps}")


def test_a_batch_without_any_bond():
    """Three one-atom molecules: E = 0, empty edge arrays; every NNConv row is its bias."""
    g = mvml_gat.from_arrays([1, 1, 1], [0, 0, 0], [], []).to(DEV)
    none = torch.zeros(0, dtype=torch.long)
    torch.manual_seed(5)
    model = MPNNPredictor(39, 10, node_out_feats=16, edge_hidden_feats=16, n_tasks=3, num_step_message_passing=2,
                          num_step_set2set=1, num_layer_set2set=1)
    _predictor_case(model, g, none, none, torch.arange(3), 2, 1, 1, "no bonds")


def test_modules_refuse_what_the_kernels_do_not_hold():
    net = lambda: torch.nn.Sequential(torch.nn.Linear(10, 32), torch.nn.ReLU(), torch.nn.Linear(32, 256))
    with pytest.raises(ValueError, match="aggregator_type"):
        NNConv(16, 16, net(), aggregator_type="mean")
    with pytest.raises(ValueError, match="residual"):
        NNConv(16, 16, net(), residual=True)
    with pytest.raises(ValueError, match="node_out_feats"):
        MPNNGNN(39, 10, node_out_feats=20)
