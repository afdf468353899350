"""Weave's readout on the GPU against the float64 formulas of tests/_weave_ref.py ([N, F K] materialised):
mvml_weave_gather_fwd / _bwd through Fn.WeaveGatherFunction, then the WeaveGather module.
Batch: _afp_ref.molecules() twice, as tests/test_gpu_schnet.py: ten molecules of 1 to 19 atoms, 80 atoms.
Values uniform in [-3, 3], one exactly on a mean and one at 40, where every exp underflows and the 1e-7
floor decides (p = 1 / K).  The atom rows have a pitch past F, NaN-filled.  The memberships are float32
values, as the module's parameters are; the reference takes those same values.
Bar (the project's rule): the norm-wise conftest.rel_err <= max(1e-5, 4 e32) per quantity, e32 the same
formulas in float32 on the CPU against their float64 run; no entry is masked.  At K = 1 every p is 1 and the
atom rows' gradient is rounding noise in both reference runs; 4 e32 of that pair is the bar all the same."""
import functools

import pytest
import torch

import _afp_ref as A
import _weave_ref as R
import mvml_gat
from conftest import rel_err
from mvml_gat import WeaveGather
from mvml_gat import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _f32(vals):
    return torch.tensor(vals, dtype=torch.float32).tolist()


def _members(K):
    if K == 11:
        return _f32([m for m, _ in Fn.WEAVE_MEMBERSHIPS]), _f32([s for _, s in Fn.WEAVE_MEMBERSHIPS])
    return _f32(torch.linspace(-2, 2, K).tolist() if K > 1 else [0.3]), _f32([0.1 + 0.0125 * k for k in range(K)])


@functools.lru_cache(maxsize=None)
def _batch():
    nn_, ne, src, dst = A.molecules()
    nn_, ne, src, dst = 2 * nn_, 2 * ne, 2 * src, 2 * dst
    return mvml_gat.from_arrays(nn_, ne, src, dst).to(DEV), A.global_ids(nn_, ne, src, dst)[2]


def _values(N, F, means, seed):
    x = torch.rand((N, F), generator=torch.Generator().manual_seed(seed)) * 6 - 3
    x[0, 0], x[N - 1, F - 1] = means[len(means) // 2], 40.0
    return x


def _pitched(x):
    buf = torch.full((x.shape[0], x.shape[1] + 8), float("nan"), device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]].detach().requires_grad_()


def _both(fn, leaves):
    """fn's outputs and the gradients of its leaves at float64 and float32: fn(leaves) -> (outs, loss)."""
    res = []
    for dt in (torch.float64, torch.float32):
        ls = {k: v.to(dt).clone().requires_grad_() for k, v in leaves.items()}
        outs, loss = fn(ls)
        loss.backward()
        res.append({**{k: v.detach() for k, v in outs.items()}, **{"g_" + k: v.grad for k, v in ls.items()}})
    return res


def _check(what, got, r64, r32):
    assert sorted(got) == sorted(r64)
    for k in r64:
        e, b = rel_err(got[k], r64[k]), max(TOL, 4 * rel_err(r32[k], r64[k]))
        print(f"weave {what} {k}: {e:.2e} / {b:.2e}")
        assert bool(torch.isfinite(got[k]).all()) and e <= b, (what, k, e, b)


@pytest.mark.parametrize("F,K", [(4, 1), (128, 11), (1024, 16), (68, 3)])
def test_gather_against_float64(F, K):
    g, gid = _batch()
    N, B = g.num_nodes(), g.batch_size
    means, stds = _members(K)
    x = _values(N, F, means, 10 * F + K)
    dG = torch.randn((B, F * K), generator=torch.Generator().manual_seed(K))

    def fn(l):
        h = R.sum_nodes(R.histogram(l["x"], means, stds), gid, B)
        return {"hist": h}, (h * dG.to(h.dtype)).sum()
    r64, r32 = _both(fn, {"x": x})
    xd = _pitched(x)
    h = Fn.WeaveGatherFunction.apply(xd, g, means, stds)
    h.backward(dG.to(DEV))
    torch.cuda.synchronize()
    assert h.shape == (B, F * K)
    if K > 1:
        assert float(r64["g_x"].abs().max()) > 0 and float(r64["g_x"][N - 1, F - 1]) == 0.0
    _check(f"F={F} K={K}", {"hist": h.detach(), "g_x": xd.grad}, r64, r32)


@pytest.mark.parametrize("kw", [dict(node_in_feats=128), dict(node_in_feats=12, gaussian_expand=False),
                                dict(node_in_feats=8, gaussian_memberships=[(-1., .5), (0., .25), (1., .5)], activation=None)])
def test_module_against_float64_and_bitwise_repeatable(kw):
    """Weight-tied through the state_dict; without gaussian_expand the plain sum.  The second step (the
    memberships' host copy is cached) runs no aten arithmetic operator, as tests/test_gpu_gin.py checks it."""
    from torch.profiler import ProfilerActivity, profile
    g, gid = _batch()
    N, B, F = g.num_nodes(), g.batch_size, kw["node_in_feats"]
    torch.manual_seed(F)
    model = WeaveGather(**kw)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    K = len(sd) // 2 - 1 if sd else 0
    means, stds = ([float(sd.pop(f"{n}.{k}")) for k in range(K)] if K else None for n in ("means", "stds"))
    assert sorted(sd) == (["to_out.bias", "to_out.weight"] if K else [])
    x, gy = _values(N, F, means or [0.0], F), torch.randn((B, F), generator=torch.Generator().manual_seed(1))

    def fn(l):
        y = R.gather(l["x"], gid, B, means, stds, l.get("to_out.weight"), l.get("to_out.bias"), tanh=kw.get("activation", 1) is not None)
        return {"y": y}, (y * gy.to(y.dtype)).sum()
    r64, r32 = _both(fn, {"x": x, **sd})
    model = model.to(DEV).train()
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        xd = _pitched(x)
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            y = model(g, xd)
            y.backward(gy.to(DEV))
            torch.cuda.synchronize()
        runs.append({"y": y.detach(), "g_x": xd.grad, **{"g_" + k: p.grad for k, p in model.named_parameters() if p.requires_grad}})
    _check(f"module F={F} K={K}", runs[0], r64, r32)
    for k in runs[0]:
        assert torch.equal(runs[0][k].contiguous().view(torch.int32), runs[1][k].contiguous().view(torch.int32)), k
    ops = {e.name for e in prof.events() if e.name.startswith("aten::")}
    banned = ("add", "sub", "mul", "div", "sum", "mm", "matmul", "linear", "tanh", "tanh_backward", "exp", "index", "scatter",
              "neg", "cat", "stack", "gather", "item")
    bad = sorted(o for o in ops if o[6:].rstrip("_").split(".")[0] in banned or o[6:].startswith(("addmm", "index_")))
    assert not bad, (bad, sorted(ops))
