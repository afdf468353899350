"""mvml_gcn_agg / mvml_gcn_norm_scales (csrc/gcn_agg.hip) through the C ABI against float64.

Graphs: GRAPHS of tests/test_gpu_agg_shapes.py (a 170-atom mix with a 1-atom molecule, a single
atom, two hub batches whose in-degrees pass the 64-entry chunk) and one batch without self-loops,
in which some atoms have no in-edges and some no out-edges.

Widths: the dispatcher's instances are the sub-wave form (D <= 64) and the one-row form at 1, 2, 3,
4 and 8 float4 slots per lane; D below reaches each with a full and a partly masked last slot, the
sub-wave form's last width (64) and the first past it (68).

Every case runs the forward CSR with (both scales, bias, ReLU), (no scale, no bias, no act) and
(neighbour scale only, bias), and the swapped call over the out-CSR, which must be the reference's
autograd gradient.  X has a row pitch past D with NaN in the pad; out is pre-filled with a sentinel
that must survive in its pad.

Bar: conftest.rel_err <= max(1e-5, 4 e32) per tensor, e32 the same reference in float32 on the CPU
against its float64 run."""
import functools

import numpy as np
import pytest
import torch

import mvml_gat
from conftest import rel_err
from mvml_gat import synth
from mvml_gat._lib import lib, option, ptr, stream_ptr
from test_gpu_agg_shapes import GRAPHS as GAT_GRAPHS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
FILL = -7777.0
MVML_ERR_INVALID = 1
WIDTHS = [4, 60, 64, 68, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048]


def _no_loops():
    """No self-loops: a path with two isolated atoms, a single atom without edges, one-way edges
    (atoms with out-edges only / in-edges only) and a 70-spoke one-way star into atom 0."""
    mols = [mvml_gat.bigraph_from_bonds(5, [[0, 1], [1, 2]], add_self_loop=False),
            mvml_gat.bigraph_from_bonds(1, np.zeros((0, 2)), add_self_loop=False),
            mvml_gat.graph(([0, 0, 1, 3], [1, 2, 2, 2]), num_nodes=5),
            mvml_gat.graph((list(range(1, 71)), [0] * 70), num_nodes=71)]
    return mvml_gat.batch(mols)


GRAPHS = {**{k: (lambda f=f: f().to_graph()) for k, f in GAT_GRAPHS.items()}, "no_loops": _no_loops}


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = GRAPHS[name]().to(DEV)
    return g, g.src.cpu().long(), g.dst.cpu().long()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _call(g, X, D, nbr_scale=None, row_scale=None, bias=None, act=0, transpose=False, rows=True, out=None, ldo=None,
          ldx=None, N=None):
    """One mvml_gcn_agg call; returns (rc, out incl. its pad, out_amax, out_row_amax)."""
    N = g.num_nodes() if N is None else N
    ldo = D + 4 if ldo is None else ldo
    if out is None:
        out = torch.full((max(N, 1), ldo), FILL, device=DEV)
    omx = torch.zeros(1, dtype=torch.int32, device=DEV)
    orow = torch.zeros(max(N, 1), dtype=torch.int32, device=DEV)
    rowptr, nbr = (g.out_rowptr, g.out_dst) if transpose else (g.in_rowptr, g.in_src)
    rc = lib().mvml_gcn_agg(N, ptr(rowptr), ptr(nbr), ptr(X), X.stride(0) if ldx is None else ldx, D, ptr(nbr_scale),
                            ptr(row_scale), ptr(bias), act, ptr(out), ldo, ptr(omx), ptr(orow) if rows else None,
                            stream_ptr())
    torch.cuda.synchronize()
    return rc, out, omx, orow


def _ref(src, dst, X, ns, rs, bias, act, dtype, g_out=None):
    """act(rs * sum_{u -> v} ns[u] X[u] + bias) on the CPU and, with g_out, its gradient in X."""
    X = X.to(dtype).clone().requires_grad_()
    h = X if ns is None else X * ns.to(dtype).unsqueeze(1)
    out = torch.zeros_like(X).index_add(0, dst, h[src])
    if rs is not None:
        out = out * rs.to(dtype).unsqueeze(1)
    if bias is not None:
        out = out + bias.to(dtype)
    if act:
        out = torch.relu(out)
    if g_out is None:
        return out.detach()
    out.backward(g_out.to(dtype))
    return X.grad


def _inputs(N, D, seed):
    gen = torch.Generator().manual_seed(seed)
    X = torch.full((N, D + 12), float("nan"))
    X[:, :D] = torch.randn((N, D), generator=gen)
    return dict(X=X, ns=torch.rand(N, generator=gen) + 0.25, rs=torch.rand(N, generator=gen) + 0.25,
                bias=torch.randn(D, generator=gen) * 0.5, g=torch.randn((N, D), generator=gen))


@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("D", WIDTHS)
def test_gcn_agg_against_float64(D, graph):
    g, src, dst = _graph(graph)
    N = g.num_nodes()
    inp = _inputs(N, D, seed=100 * D + len(graph))
    dev = {k: v.to(DEV) for k, v in inp.items()}
    Xc = inp["X"][:, :D]
    worst = (0.0, None)
    configs = {"scales+bias+relu": ("ns", "rs", "bias", 1), "plain": (None, None, None, 0),
               "nbr_scale+bias": ("ns", None, "bias", 0), "row_scale+relu": (None, "rs", None, 1)}
    for name, (ns, rs, bias, act) in configs.items():
        args = [inp.get(ns), inp.get(rs), inp.get(bias), act]
        r64, r32 = (_ref(src, dst, Xc, *args, dt) for dt in (torch.float64, torch.float32))
        budget = max(TOL, 4 * rel_err(r32, r64))
        rc, out, omx, orow = _call(g, dev["X"], D, dev.get(ns), dev.get(rs), dev.get(bias), act)
        assert rc == 0, lib().mvml_last_error()
        got = out[:N, :D]
        assert bool(torch.isfinite(got).all()), (name, "NaN / inf: a masked lane read the pad")
        err = rel_err(got, r64)
        print(f"GCN_AGG D={D} graph={graph} {name}: err {err:.2e} budget {budget:.2e}")
        worst = max(worst, (err / budget, name))
        assert err <= budget, (name, err, budget)
        assert bool((out[:, D:] == FILL).all()), (name, "out columns past D written")
        # the maxima are, as bits, those of the stored fp32 values
        assert _bits(omx).item() == _bits(got.abs().max().reshape(1)).item(), (name, "out_amax")
        assert torch.equal(_bits(orow[:N]), _bits(got.abs().max(dim=1).values)), (name, "out_row_amax")
        # out_amax alone (folded per block) is the same number; a second run gives the same bits
        rc, out2, omx2, _ = _call(g, dev["X"], D, dev.get(ns), dev.get(rs), dev.get(bias), act, rows=False)
        assert rc == 0 and torch.equal(out2, out) and omx2.item() == omx.item(), (name, "repeat / out_amax alone")
        if D <= 64:  # the sub-wave form is bitwise the one-row form
            res = []
            for sub in (0, 1):
                with option("gcn_subwave", sub):
                    res.append(_call(g, dev["X"], D, dev.get(ns), dev.get(rs), dev.get(bias), act))
            assert res[0][0] == 0 and res[1][0] == 0
            for a, b in zip(res[0][1:], res[1][1:]):
                assert torch.equal(a, b), (name, "sub-wave form vs one row per wave")
    # the swapped call over the out-CSR is the gradient of the sum
    for name, ns, rs in (("scaled", inp["ns"], inp["rs"]), ("plain", None, None)):
        d64, d32 = (_ref(src, dst, Xc, ns, rs, None, 0, dt, g_out=inp["g"]) for dt in (torch.float64, torch.float32))
        budget = max(TOL, 4 * rel_err(d32, d64))
        rc, dX, omx, orow = _call(g, dev["g"], D, None if rs is None else dev["rs"], None if ns is None else dev["ns"],
                                  transpose=True)
        assert rc == 0, lib().mvml_last_error()
        err = rel_err(dX[:N, :D], d64)
        print(f"GCN_AGG D={D} graph={graph} adjoint {name}: err {err:.2e} budget {budget:.2e}")
        worst = max(worst, (err / budget, "adjoint " + name))
        assert err <= budget, ("adjoint", name, err, budget)
        assert bool((dX[:, D:] == FILL).all())
        assert torch.equal(_bits(orow[:N]), _bits(dX[:N, :D].abs().max(dim=1).values))
    print(f"worst err/budget {worst[1]}: {worst[0]:.3f}")


def test_row_without_entries_gives_act_bias():
    g, src, dst = _graph("no_loops")
    N, D = g.num_nodes(), 8
    assert g.has_zero_in_degree
    inp = _inputs(N, D, seed=5)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    empty = torch.bincount(dst, minlength=N) == 0
    assert int(empty.sum()) >= 4
    for act in (0, 1):
        rc, out, _, orow = _call(g, dev["X"], D, dev["ns"], dev["rs"], dev["bias"], act)
        want = torch.relu(inp["bias"]) if act else inp["bias"]
        assert rc == 0 and torch.equal(out[:N, :D].cpu()[empty], want.expand(int(empty.sum()), D))
    rc, out, _, orow = _call(g, dev["X"], D, dev["ns"], dev["rs"], None, 0)
    assert rc == 0 and float(out[:N, :D].cpu()[empty].abs().max()) == 0.0 and int(orow.cpu()[:N][empty].max()) == 0


@pytest.mark.parametrize("graph,mol", [("mixed", 2), ("mixed", 6), ("hubs", 1), ("mixed", 1)])
@pytest.mark.parametrize("D", [4, 64, 260])
def test_molecule_alone_is_bitwise_its_rows_of_the_batch(D, graph, mol):
    sb = GAT_GRAPHS[graph]()
    g, _, _ = _graph(graph)
    N = g.num_nodes()
    inp = _inputs(N, D, seed=3)
    lo = int(sb.num_nodes[:mol].sum())
    n = int(sb.num_nodes[mol])
    one = synth.slice_batch(sb, mol, mol + 1).to_graph().to(DEV)
    X, ns, rs, bias = (inp[k].to(DEV) for k in ("X", "ns", "rs", "bias"))
    rc, full, _, frow = _call(g, X, D, ns, rs, bias, 1)
    rc1, part, _, prow = _call(one, X[lo:lo + n], D, ns[lo:lo + n].clone(), rs[lo:lo + n].clone(), bias, 1)
    assert rc == 0 and rc1 == 0
    assert torch.equal(part[:n], full[lo:lo + n]) and torch.equal(prow[:n], frow[lo:lo + n])


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_norm_scales(graph):
    g, src, dst = _graph(graph)
    N = g.num_nodes()
    indeg = np.maximum(np.bincount(dst.numpy(), minlength=N), 1).astype(np.float64)
    outdeg = np.maximum(np.bincount(src.numpy(), minlength=N), 1).astype(np.float64)
    one = np.ones(N, dtype=np.float32)
    want = {0: (one, one), 1: (outdeg ** -0.5, indeg ** -0.5), 2: (one, 1.0 / indeg), 3: (1.0 / outdeg, one)}
    for norm, (ws, wd) in want.items():
        s = torch.full((2, N), FILL, device=DEV)
        rc = lib().mvml_gcn_norm_scales(N, ptr(g.in_rowptr), ptr(g.out_rowptr), norm, ptr(s[0]), ptr(s[1]), stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, lib().mvml_last_error()
        for got, w in ((s[0], ws), (s[1], wd)):
            got = got.cpu().numpy()
            if w is one:
                assert np.array_equal(got, one), norm
            else:
                ulp = np.abs(got.view(np.int32).astype(np.int64) - w.astype(np.float32).view(np.int32).astype(np.int64))
                assert int(ulp.max()) <= 1, (norm, int(ulp.max()))
    s = torch.full((2, N), FILL, device=DEV)
    for norm in (-1, 4):
        rc = lib().mvml_gcn_norm_scales(N, ptr(g.in_rowptr), ptr(g.out_rowptr), norm, ptr(s[0]), ptr(s[1]), stream_ptr())
        assert rc == MVML_ERR_INVALID and b"norm" in lib().mvml_last_error()
    assert lib().mvml_gcn_norm_scales(N, None, ptr(g.out_rowptr), 1, ptr(s[0]), ptr(s[1]), stream_ptr()) == MVML_ERR_INVALID
    assert lib().mvml_gcn_norm_scales(N, ptr(g.in_rowptr), ptr(g.out_rowptr), 1, None, ptr(s[1]), stream_ptr()) == MVML_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((s == FILL).all())


def test_scales_are_cached_per_graph_and_norm_and_dropped_by_recollate():
    from mvml_gat import functional as Fn
    g = GAT_GRAPHS["mixed"]().to_graph().to(DEV)
    assert Fn.gcn_scales(g, "none") == (None, None)
    s, d = Fn.gcn_scales(g, "both")
    assert Fn.gcn_scales(g, "both")[0] is s and Fn.gcn_scales(g, "both")[1] is d
    assert Fn.gcn_scales(g, "right")[0] is None and Fn.gcn_scales(g, "left")[1] is None
    g.recollate()
    s2, d2 = Fn.gcn_scales(g, "both")
    assert s2 is not s and torch.equal(s2, s) and torch.equal(d2, d)


def test_invalid_arguments_are_refused_and_write_nothing():
    g, _, _ = _graph("mixed")
    N, D = g.num_nodes(), 64
    X = torch.randn((N, D + 12), device=DEV)
    bias = torch.randn(D + 4, device=DEV)
    flat = torch.full((N * (D + 4) + 8,), FILL, device=DEV)
    out = flat[:N * (D + 4)].view(N, D + 4)
    cases = {"D % 4": dict(D=6), "D = 0": dict(D=0), "D > 2048": dict(D=2052), "ldx < D": dict(ldx=60),
             "ldx % 4": dict(ldx=D + 3), "ldo < D": dict(ldo=60), "ldo % 4": dict(ldo=D + 2), "act": dict(act=2),
             "X alignment": dict(X=X.view(-1)[1:1 + (N - 1) * (D + 12)].view(N - 1, D + 12), N=N - 1),
             "bias alignment": dict(bias=bias[1:D + 1]),
             "out alignment": dict(out=flat[1:1 + N * (D + 4)].view(N, D + 4)),
             "negative N": dict(N=-1)}
    for why, kw in cases.items():
        a = dict(X=X, D=D, bias=bias[:D], act=1, out=out)
        a.update(kw)
        Xa = a.pop("X")
        if why == "X alignment":
            a["ldx"] = D + 12
        rc, o, omx, orow = _call(g, Xa, a.pop("D"), None, None, a.pop("bias"), a.pop("act"), **a)
        assert rc == MVML_ERR_INVALID and lib().mvml_last_error(), why
        assert bool((flat == FILL).all()) and int(omx.item()) == 0 and int(orow.abs().max().item()) == 0, why
    # out aliasing X (the same rows, or rows that overlap them)
    for o in (X, X[:, 4:]):
        before = X.clone()
        rc = lib().mvml_gcn_agg(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(X), D + 12, 8, None, None, None, 0, ptr(o),
                                D + 12, None, None, stream_ptr())
        torch.cuda.synchronize()
        assert rc == MVML_ERR_INVALID and b"alias" in lib().mvml_last_error() and torch.equal(X, before)
    # an empty batch is no error and launches nothing
    assert _call(g, X, D, N=0)[0] == 0
