"""Weave's pair-update layers on the GPU against the float64 formulas of tests/_weave_pair_ref.py (every
[E, H] intermediate materialised): the kernels of csrc/weave_pair.hip through Fn.WeaveLayerFunction, then
WeaveGNN and WeavePredictor.
Batch: _afp_ref.molecules() (a single atom without in-edge, a hub of in-degree 70), one complete graph with
self-loops on 13 atoms (169 edges) and a star of 140 leaves with edges both ways: the hub's slot run spans
more than one 128-slot tile, other runs straddle tile boundaries.  Inputs from a fixed-seed generator, the
rows at a NaN-filled pitch.
Bar (the project's rule): the norm-wise conftest.rel_err <= max(1e-5, 4 e32) per quantity, e32 the same
formulas in float32 on the CPU against their float64 run; no entry is masked."""
import functools

import pytest
import torch

import _afp_ref as A
import _weave_pair_ref as R
import mvml_gat
from conftest import rel_err
from mvml_gat import WeaveGNN, WeaveLayer, WeavePredictor
from mvml_gat import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _batch():
    nn_, ne, src, dst = A.molecules()
    assert 1 in nn_ and ne[nn_.index(1)] == 0  # an atom without in-edge
    full = [(a, b) for a in range(13) for b in range(13)]
    star = [(0, k) for k in range(1, 141)] + [(k, 0) for k in range(1, 141)]
    for n, edges in ((13, full), (141, star)):
        nn_, ne = nn_ + [n], ne + [len(edges)]
        src, dst = src + [a for a, _ in edges], dst + [b for _, b in edges]
    g = mvml_gat.from_arrays(nn_, ne, src, dst).to(DEV)
    s, d, gid = A.global_ids(nn_, ne, src, dst)
    deg = torch.bincount(d, minlength=g.num_nodes())
    assert int(deg.max()) == 140 and int(deg.min()) == 0
    return g, s, d, gid


def _pitched(x, grad=True, pitch=None):
    """x on the device at a NaN-filled pitch: by default the next multiple of 4 past its width."""
    buf = torch.full((x.shape[0], pitch or x.shape[1] + 8 - x.shape[1] % 4), float("nan"), device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]].detach().requires_grad_(grad)


def _both(fn, leaves):
    """fn's outputs and the gradients of its leaves at float64 and float32: fn(leaves) -> (outs, loss)."""
    res = []
    for dt in (torch.float64, torch.float32):
        ls = {k: v.to(dt).clone().requires_grad_() for k, v in leaves.items()}
        outs, loss = fn(ls)
        loss.backward()
        res.append({**{k: v.detach() for k, v in outs.items()}, **{"g_" + k: v.grad for k, v in ls.items() if v.grad is not None}})
    return res


def _check(what, got, r64, r32):
    assert sorted(got) == sorted(r64)
    for k in r64:
        e, b = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        print(f"weave pair {what} {k}: {e:.2e} / {b:.2e}")
        assert float(r64[k].abs().max()) > 0, k  # (checked on the CPU: no reference quantity is all zero)
        assert bool(torch.isfinite(got[k]).all()) and e <= b, (what, k, e, b)


def _layer_case(dn, de, widths, node_only=False, e_pitch=None):
    g, src, dst, _ = _batch()
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator().manual_seed(1000 * dn + 10 * de + sum(widths))
    layer = WeaveLayer(dn, de, *widths, _slot_input=True)
    sd = {k: torch.randn(v.shape, generator=gen) * (0.5 if k.endswith("bias") else v.shape[-1] ** -0.5)
          for k, v in layer.state_dict().items()}
    x, e = torch.randn((N, dn), generator=gen), torch.randn((E, de), generator=gen)
    gx, ge = torch.randn((N, widths[2]), generator=gen), torch.randn((E, widths[5]), generator=gen)

    def fn(l):
        if node_only:
            xn = R.layer(l, "", src, dst, l["x"], l["e"], node_only=True)
            return {"xn": xn}, (xn * gx.to(xn.dtype)).sum()
        xn, en = R.layer(l, "", src, dst, l["x"], l["e"])
        return {"xn": xn, "en": en}, (xn * gx.to(xn.dtype)).sum() + (en * ge.to(en.dtype)).sum()
    r64, r32 = _both(fn, {"x": x, "e": e, **sd})
    # the kernel's edge rows are in in-CSR slot order: slot s holds edge in_eid[s]
    eid = g.in_eid.cpu().long()
    xd, ed = _pitched(x), _pitched(e[eid], pitch=e_pitch)
    params = {k: v.to(DEV).requires_grad_() for k, v in sd.items()}
    xn, en = Fn.WeaveLayerFunction.apply(xd, ed, g, node_only, True, *[params[f"{n}.{p}"] for n in R.LINEARS for p in ("weight", "bias")])
    loss = (xn * gx.to(DEV)).sum() if node_only else (xn * gx.to(DEV)).sum() + (en * ge.to(DEV)[eid.to(DEV)]).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {"xn": xn.detach().cpu(), "g_x": xd.grad.cpu(), "g_e": torch.empty_like(e).index_copy_(0, eid, ed.grad.cpu())}
    if not node_only:
        got["en"] = torch.empty((E, widths[5])).index_copy_(0, eid, en.detach().cpu())
    got.update({"g_" + k: p.grad.cpu() for k, p in params.items() if p.grad is not None})
    return got, r64, r32


@pytest.mark.parametrize("dn,de,widths,e_pitch", [
    (27, 12, (50,) * 6, None), (8, 1, (16,) * 6, None), (50, 50, (50,) * 6, None), (128, 32, (128,) * 6, None),
    (12, 5, (1,) * 6, None), (27, 12, (16, 24, 20, 40, 8, 36), None),
    (50, 50, (50,) * 6, 51)])  # slot-order rows at a pitch that is no multiple of 4: the launch code re-pitches them
def test_layer_against_float64(dn, de, widths, e_pitch):
    got, r64, r32 = _layer_case(dn, de, widths, e_pitch=e_pitch)
    assert len(r64) == 2 + 2 + 14
    _check(f"dn={dn} de={de} {widths} pitch={e_pitch}", got, r64, r32)


def test_layer_node_only_gives_the_edge_linears_no_gradient():
    got, r64, r32 = _layer_case(27, 12, (50,) * 6, node_only=True)
    assert sorted(k.split(".")[0] for k in got if k.endswith(".weight")) == ["g_edge_to_node", "g_node_to_node", "g_update_node"]
    _check("node_only", got, r64, r32)


@pytest.mark.parametrize("kind", ["layer", "gnn", "predictor"])
def test_modules_against_float64_and_bitwise_repeatable(kind):
    """Weight-tied through the state_dict, train mode, edge rows in edge-id order ("layer": a WeaveLayer
    called directly, whose new edge rows come back in edge-id order).  Two runs bit-equal; the second step
    runs no aten arithmetic operator, as tests/test_gpu_weave.py checks it."""
    from torch.profiler import ProfilerActivity, profile
    g, src, dst, gid = _batch()
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    torch.manual_seed(7)
    model = {"layer": lambda: WeaveLayer(27, 12), "gnn": lambda: WeaveGNN(27, 12),
             "predictor": lambda: WeavePredictor(27, 12, n_tasks=3)}[kind]()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ms = [[float(sd[f"readout.{n}.{k}"]) for k in range(11)] for n in ("means", "stds")] if kind == "predictor" else None
    leaves = {k: v for k, v in sd.items() if v.dtype == torch.float32 and "running" not in k and "readout.means" not in k
              and "readout.stds" not in k}
    gen = torch.Generator().manual_seed(3)
    x, e = torch.randn((N, 27), generator=gen), torch.randn((E, 12), generator=gen)
    gy, ge = torch.randn((B, 3) if kind == "predictor" else (N, 50), generator=gen), torch.randn((E, 50), generator=gen)

    def fn(l):
        if kind == "layer":
            y, en = R.layer(l, "", src, dst, l["x"], l["e"])
            return {"y": y, "en": en}, (y * gy.to(y.dtype)).sum() + (en * ge.to(y.dtype)).sum()
        y = R.gnn(l, "", src, dst, l["x"], l["e"], 2) if kind == "gnn" else R.predictor(l, src, dst, gid, B, l["x"], l["e"], 2, *ms)
        return {"y": y}, (y * gy.to(y.dtype)).sum()
    r64, r32 = _both(fn, {"x": x, "e": e, **leaves})
    model = model.to(DEV).train()
    gyd, ged = gy.to(DEV), ge.to(DEV)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        xd, ed = _pitched(x), _pitched(e)
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            y = model(g, xd, ed)
            y, en = y if kind == "layer" else (y, None)
            torch.autograd.backward([y, en] if kind == "layer" else [y], [gyd, ged] if kind == "layer" else [gyd])
            torch.cuda.synchronize()
        runs.append({"y": y.detach(), **({"en": en.detach()} if kind == "layer" else {}), "g_x": xd.grad, "g_e": ed.grad,
                     **{"g_" + k: p.grad for k, p in model.named_parameters() if p.grad is not None}})
    _check(kind, {k: v.cpu() for k, v in runs[0].items()}, r64, r32)
    for k in runs[0]:
        assert torch.equal(runs[0][k].contiguous().view(torch.int32), runs[1][k].contiguous().view(torch.int32)), k
    ops = {ev.name for ev in prof.events() if ev.name.startswith("aten::")}
    banned = ("add", "sub", "mul", "div", "sum", "mm", "matmul", "linear", "tanh", "tanh_backward", "exp", "index", "scatter",
              "neg", "cat", "stack", "gather", "item", "relu", "threshold_backward", "batch_norm", "native_batch_norm")
    bad = sorted(o for o in ops if o[6:].rstrip("_").split(".")[0] in banned or o[6:].startswith(("addmm", "index_")))
    assert not bad, (bad, sorted(ops))
