"""mvml_sage_max_fwd / mvml_sage_max_bwd / mvml_sage_gcn_scale / mvml_sage_self_add
(csrc/sage_agg.hip) through the C ABI against the CPU reference (tests/_sage_ref.py).

Graphs: GRAPHS of tests/test_gpu_agg_shapes.py (a 170-atom mix with a 1-atom molecule, a single
atom, two hub batches whose in-degrees pass the 64-entry chunk), the batch without self-loops of
tests/test_gpu_gcn_agg.py (empty in-rows, empty out-rows, a 70-spoke star) and one graph with a
duplicated edge.

Widths: the dispatcher's instances are the sub-wave form (D <= 64) and the one-row form at 1, 2, 3,
4 and 8 float4 slots per lane; WIDTHS reaches each with a full and a partly masked last slot, the
sub-wave form's last width (64) and the first past it (68).

X has a row pitch past D with NaN in the pad; out, arg and gX are pre-filled with a sentinel that
must survive in their pads.

Forward: a maximum rounds nothing, so out is BIT-equal to the float32 CPU maximum and arg equals the
reference's first maximiser in in-CSR order.  Backward: conftest.rel_err <= max(1e-5, 4 e32) against
the float64 gradient of the reference gathering at the same arg, e32 the same reference in float32
against its float64 run."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mvml_gat
from _sage_ref import first_argmax, in_csr, neighbour_max
from conftest import rel_err
from mvml_gat import synth
from mvml_gat._lib import lib, option, ptr, stream_ptr
from test_gpu_agg_shapes import GRAPHS as GAT_GRAPHS
from test_gpu_gcn_agg import _no_loops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
FILL = -7777.0
IFILL = -7777
MVML_ERR_INVALID = 1
WIDTHS = [4, 60, 64, 68, 256, 260, 512, 516, 768, 772, 1024, 1028, 2048]


def _dup_edge():
    """0 -> 2 twice (slots 0 and 2 of atom 2's in-row, 1 -> 2 between them), 2 -> 0, 3 -> 0; atoms 1
    and 3 have no in-edges."""
    return mvml_gat.batch([mvml_gat.graph(([0, 1, 0, 2, 3], [2, 2, 2, 0, 0]), num_nodes=4)])


GRAPHS = {**{k: (lambda f=f: f().to_graph()) for k, f in GAT_GRAPHS.items()}, "no_loops": _no_loops,
          "dup_edge": _dup_edge}


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = GRAPHS[name]().to(DEV)
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    rowptr, in_src, order = in_csr(src, dst, g.num_nodes())
    assert torch.equal(g.in_src.cpu().long(), in_src) and torch.equal(g.in_rowptr.cpu().long(), rowptr)
    return g, src, dst


def _bits(x):
    return x.contiguous().view(torch.int32)


def _fwd(g, X, D, rows=True, N=None, ldx=None, ldo=None, lda=None, out=None, arg=None):
    """One mvml_sage_max_fwd call; returns (rc, out incl. pad, arg incl. pad, out_amax, out_row_amax)."""
    N = g.num_nodes() if N is None else N
    ldo = D + 4 if ldo is None else ldo
    lda = D + 8 if lda is None else lda
    if out is None:
        out = torch.full((max(N, 1), ldo), FILL, device=DEV)
    if arg is None:
        arg = torch.full((max(N, 1), lda), IFILL, dtype=torch.int32, device=DEV)
    omx = torch.zeros(1, dtype=torch.int32, device=DEV)
    orow = torch.zeros(max(N, 1), dtype=torch.int32, device=DEV)
    rc = lib().mvml_sage_max_fwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(X), X.stride(0) if ldx is None else ldx, D,
                                 ptr(out), ldo, ptr(arg), lda, ptr(omx), ptr(orow) if rows else None, stream_ptr())
    torch.cuda.synchronize()
    return rc, out, arg, omx, orow


def _bwd(g, G, arg, D, P=None, N=None, ldg=None, lda=None, ldp=None, gX=None, ldgx=None):
    """One mvml_sage_max_bwd call; returns (rc, gX incl. pad)."""
    N = g.num_nodes() if N is None else N
    ldgx = D + 4 if ldgx is None else ldgx
    if gX is None:
        gX = torch.full((max(N, 1), ldgx), FILL, device=DEV)
    rc = lib().mvml_sage_max_bwd(N, ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(G),
                                 G.stride(0) if ldg is None else ldg, ptr(arg), arg.stride(0) if lda is None else lda, D,
                                 ptr(P), (0 if P is None else P.stride(0)) if ldp is None else ldp, ptr(gX), ldgx,
                                 stream_ptr())
    torch.cuda.synchronize()
    return rc, gX


def _padded(t, pad=12):
    """t's rows at a row pitch past its width, NaN in the pad."""
    X = torch.full((t.shape[0], t.shape[1] + pad), float("nan"))
    X[:, :t.shape[1]] = t
    return X


def _check_forward(g, src, dst, Xc, D, what):
    """Forward of the [N, D] float32 CPU tensor Xc: bits, arg, pads, maxima, repeat, both forms.
    Returns the device (X with NaN pad, arg incl. pad)."""
    N = g.num_nodes()
    X = _padded(Xc).to(DEV)
    want, own = neighbour_max(src, dst, Xc)
    rc, out, arg, omx, orow = _fwd(g, X, D)
    assert rc == 0, lib().mvml_last_error()
    got = out[:N, :D]
    assert torch.equal(_bits(got.cpu()), _bits(want)), (what, "out is not the float32 maximum, bit for bit")
    assert torch.equal(arg[:N, :D].cpu().long(), own), (what, "arg is not the first maximiser in in-CSR order")
    empty = torch.bincount(dst, minlength=N) == 0
    if bool(empty.any()):
        assert float(got.cpu()[empty].abs().max()) == 0.0 and bool((arg[:N, :D].cpu()[empty] == -1).all()), what
    assert bool((out[:, D:] == FILL).all()) and bool((arg[:, D:] == IFILL).all()), (what, "columns past D written")
    assert _bits(omx).item() == _bits(got.abs().max().reshape(1)).item(), (what, "out_amax")
    assert torch.equal(_bits(orow[:N]), _bits(got.abs().max(dim=1).values)), (what, "out_row_amax")
    rc, out2, arg2, omx2, _ = _fwd(g, X, D, rows=False)
    assert rc == 0 and torch.equal(_bits(out2), _bits(out)) and torch.equal(arg2, arg) and omx2.item() == omx.item(), \
        (what, "repeat / out_amax alone")
    if D <= 64:  # the sub-wave form is bitwise the one-row form
        for sub in (0, 1):
            with option("sage_subwave", sub):
                res = _fwd(g, X, D)
            assert res[0] == 0
            for a, b in zip(res[1:], (out, arg, omx, orow)):
                assert torch.equal(_bits(a), _bits(b)), (what, f"sage_subwave={sub} against the default")
    return X, arg


def _ref_grad(src, dst, pre, arg, G, gated, dtype):
    """d/d pre of sum(G * max_in act(pre)) gathered at `arg`; act ReLU when gated, else identity."""
    p = pre.to(dtype).clone().requires_grad_()
    out, _ = neighbour_max(src, dst, F.relu(p) if gated else p, arg)
    out.backward(G.to(dtype))
    return p.grad


def _check_backward(g, src, dst, pre, X, arg, D, gated, seed, what):
    N = g.num_nodes()
    Gc = torch.randn((N, D), generator=torch.Generator().manual_seed(seed))
    G = _padded(Gc).to(DEV)
    argc = arg[:N, :D].cpu().long()
    d64, d32 = (_ref_grad(src, dst, pre, argc, Gc, gated, dt) for dt in (torch.float64, torch.float32))
    budget = max(TOL, 4 * rel_err(d32, d64))
    rc, gX = _bwd(g, G, arg, D, P=X if gated else None)
    assert rc == 0, lib().mvml_last_error()
    got = gX[:N, :D]
    assert bool(torch.isfinite(got).all()), (what, "NaN / inf: a masked lane read the pad")
    err = rel_err(got, d64)
    print(f"SAGE_MAX_BWD D={D} {what} gated={gated}: err {err:.2e} budget {budget:.2e} ratio {err / budget:.3f}")
    assert err <= budget, (what, gated, err, budget)
    assert bool((gX[:, D:] == FILL).all()), (what, "gX columns past D written")
    rc, gX2 = _bwd(g, G, arg, D, P=X if gated else None)
    assert rc == 0 and torch.equal(_bits(gX2), _bits(gX)), (what, "not bitwise repeatable")
    if D <= 64:
        for sub in (0, 1):
            with option("sage_subwave", sub):
                rc, gX3 = _bwd(g, G, arg, D, P=X if gated else None)
            assert rc == 0 and torch.equal(_bits(gX3), _bits(gX)), (what, f"sage_subwave={sub} against the default")


@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("D", WIDTHS)
def test_sage_max_forward_bitwise_and_backward_against_float64(D, graph):
    g, src, dst = _graph(graph)
    N = g.num_nodes()
    gen = torch.Generator().manual_seed(100 * D + len(graph))
    pre = torch.randn((N, D), generator=gen)
    X, arg = _check_forward(g, src, dst, pre, D, f"{graph} plain")
    _check_backward(g, src, dst, pre, X, arg, D, False, D + 1, graph)
    # a ReLU output (half of it zeros: ties at 0), its backward folded into the gather by the gate
    X, arg = _check_forward(g, src, dst, F.relu(pre), D, f"{graph} relu")
    _check_backward(g, src, dst, pre, X, arg, D, True, D + 2, graph)


@pytest.mark.parametrize("graph", ["mixed", "hubs", "no_loops", "dup_edge"])
@pytest.mark.parametrize("D", [4, 64, 260])
@pytest.mark.parametrize("kind", ["integers", "relu_zeros"])
def test_ties_go_to_the_first_maximiser_and_hand_their_gradient_to_one_slot(kind, D, graph):
    g, src, dst = _graph(graph)
    N = g.num_nodes()
    gen = torch.Generator().manual_seed(7 * D + len(graph))
    if kind == "integers":
        Xc = torch.randint(-1, 3, (N, D), generator=gen).float()
    else:
        Xc = F.relu(torch.randn((N, D), generator=gen) - 1.0)  # about 5 in 6 are zeros
    X, arg = _check_forward(g, src, dst, Xc, D, f"{graph} {kind}")
    argc = arg[:N, :D].cpu().long()
    _, in_src, _ = in_csr(src, dst, N)
    has = argc >= 0
    assert int(has.sum()) > 0
    owner = in_src[argc.clamp(min=0)]
    cols = torch.arange(D).expand(N, D)
    # G = 1 everywhere: every (v, c) with in-edges hands its 1 to exactly one in-slot, so gX counts
    # the (v, c) each source owns (small integers: exact), and they add up to the number of (v, c)
    want = torch.zeros((N, D)).index_put((owner[has], cols[has]), torch.ones(int(has.sum())), accumulate=True)
    rc, gX = _bwd(g, torch.ones((N, D), device=DEV), arg, D)
    assert rc == 0 and torch.equal(gX[:N, :D].cpu(), want) and float(gX[:N, :D].sum()) == float(has.sum())
    # one-hot G at single (v, c): the whole gradient lands on the first maximiser's source, once
    picks = [(int(v), int(c)) for v, c in zip(torch.randint(0, N, (3,), generator=gen), torch.randint(0, D, (3,), generator=gen))]
    if graph == "dup_edge":
        picks = [(2, c) for c in range(min(D, 4))] + picks  # atom 2: in-row [0, 1, 0]
    for v, c in picks:
        G = torch.zeros((N, D), device=DEV)
        G[v, c] = 1.0
        rc, gX = _bwd(g, G, arg, D)
        hot = torch.zeros((N, D))
        if bool(has[v, c]):
            hot[owner[v, c], c] = 1.0
        assert rc == 0 and torch.equal(gX[:N, :D].cpu(), hot), (v, c)


def test_duplicated_edge_receives_the_gradient_once():
    g, src, dst = _graph("dup_edge")
    N, D = 4, 4
    # atom 2's in-row is [0, 1, 0]: column 0 has its maximum at source 0 (slots 0 and 2 tie: slot 0
    # owns it), column 1 at source 1, columns 2 and 3 tie between all three (slot 0)
    Xc = torch.tensor([[5.0, 1.0, 2.0, 0.0], [3.0, 4.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0], [9.0, 9.0, 9.0, 9.0]])
    X, arg = _check_forward(g, src, dst, Xc, D, "dup_edge by hand")
    base = int(g.in_rowptr[2])
    assert arg[2, :D].cpu().tolist() == [base, base + 1, base, base]
    G = torch.zeros((N, D), device=DEV)
    G[2] = torch.tensor([1.0, 10.0, 100.0, 1000.0])
    rc, gX = _bwd(g, G, arg, D)
    assert rc == 0
    assert gX[:N, :D].cpu().tolist() == [[1.0, 0.0, 100.0, 1000.0], [0.0, 10.0, 0.0, 0.0], [0.0] * 4, [0.0] * 4]
    rc, gX = _bwd(g, G, arg, D, P=X)  # gated by X > 0: column 3 (a maximum of 0) passes nothing
    assert gX[:N, :D].cpu().tolist() == [[1.0, 0.0, 100.0, 0.0], [0.0, 10.0, 0.0, 0.0], [0.0] * 4, [0.0] * 4]


@pytest.mark.parametrize("graph,mol", [("mixed", 2), ("mixed", 6), ("hubs", 1), ("mixed", 1)])
@pytest.mark.parametrize("D", [4, 64, 260])
def test_molecule_alone_is_bitwise_its_rows_of_the_batch(D, graph, mol):
    sb = GAT_GRAPHS[graph]()
    g, _, _ = _graph(graph)
    N = g.num_nodes()
    X = _padded(torch.randn((N, D), generator=torch.Generator().manual_seed(3))).to(DEV)
    lo, n = int(sb.num_nodes[:mol].sum()), int(sb.num_nodes[mol])
    one = synth.slice_batch(sb, mol, mol + 1).to_graph().to(DEV)
    rc, full, farg, _, frow = _fwd(g, X, D)
    rc1, part, parg, _, prow = _fwd(one, X[lo:lo + n], D)
    assert rc == 0 and rc1 == 0
    assert torch.equal(_bits(part[:n]), _bits(full[lo:lo + n])) and torch.equal(prow[:n], frow[lo:lo + n])
    # the slots are global: the molecule's own CSR starts at 0, the batch's at the molecule's first in-edge
    shift = int(g.in_rowptr[lo])
    assert torch.equal(parg[:n, :D] + shift, farg[lo:lo + n, :D])


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_gcn_scale_and_self_add(graph):
    g, src, dst = _graph(graph)
    N, D = g.num_nodes(), 68
    s = torch.full((N + 1,), FILL, device=DEV)
    rc = lib().mvml_sage_gcn_scale(N, ptr(g.in_rowptr), ptr(s), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().mvml_last_error()
    want = 1.0 / (np.bincount(dst.numpy(), minlength=N).astype(np.float64) + 1.0)
    got = s[:N].cpu().numpy()
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.astype(np.float32).view(np.int32).astype(np.int64))
    assert int(ulp.max()) <= 1 and float(s[N]) == FILL
    gen = torch.Generator().manual_seed(11)
    Xc, oc, bias = torch.randn((N, D), generator=gen), torch.randn((N, D), generator=gen), torch.randn(D, generator=gen)
    X = _padded(Xc).to(DEV)
    sc = s[:N].cpu()
    for b, act in ((None, 0), (bias, 0), (bias, 1)):
        refs = []
        for dt in (torch.float64, torch.float32):
            r = sc.to(dt).unsqueeze(1) * Xc.to(dt) + oc.to(dt) + (0 if b is None else b.to(dt))
            refs.append(torch.relu(r) if act else r)
        out = torch.full((N, D + 4), FILL, device=DEV)
        out[:, :D] = oc.to(DEV)
        rc = lib().mvml_sage_self_add(N, ptr(X), X.stride(0), D, ptr(s), ptr(None if b is None else b.to(DEV)), act,
                                      ptr(out), D + 4, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, lib().mvml_last_error()
        err, budget = rel_err(out[:, :D], refs[0]), max(TOL, 4 * rel_err(refs[1], refs[0]))
        assert err <= budget and bool((out[:, D:] == FILL).all()), (act, err, budget)
    # refusals write nothing
    out = torch.full((N, D + 4), FILL, device=DEV)
    bad = [dict(D=6), dict(D=0), dict(D=2052), dict(ldx=D - 4), dict(ldo=D + 2), dict(act=2), dict(N=-1), dict(s=None)]
    for kw in bad:
        a = dict(N=N, D=D, ldx=X.stride(0), ldo=D + 4, act=0, s=s)
        a.update(kw)
        rc = lib().mvml_sage_self_add(a["N"], ptr(X), a["ldx"], a["D"], ptr(a["s"]), None, a["act"], ptr(out), a["ldo"],
                                      stream_ptr())
        assert rc == MVML_ERR_INVALID and lib().mvml_last_error(), kw
    assert lib().mvml_sage_self_add(N, ptr(X), X.stride(0), 8, ptr(s), None, 0, ptr(X[:, 4:]), X.stride(0),
                                    stream_ptr()) == MVML_ERR_INVALID and b"alias" in lib().mvml_last_error()
    assert lib().mvml_sage_gcn_scale(N, None, ptr(s), stream_ptr()) == MVML_ERR_INVALID
    assert lib().mvml_sage_gcn_scale(N, ptr(g.in_rowptr), None, stream_ptr()) == MVML_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and not bool(torch.isnan(X[:, :D]).any())


def test_gcn_scale_is_cached_on_the_batch_and_dropped_by_recollate():
    from mvml_gat import functional as Fn
    g = GAT_GRAPHS["mixed"]().to_graph().to(DEV)
    s = Fn.sage_gcn_scale(g)
    assert Fn.sage_gcn_scale(g) is s
    g.recollate()
    s2 = Fn.sage_gcn_scale(g)
    assert s2 is not s and torch.equal(s2, s)


def test_invalid_arguments_are_refused_and_write_nothing():
    g, _, _ = _graph("mixed")
    N, D = g.num_nodes(), 64
    X = torch.randn((N, D + 12), device=DEV)
    flat = torch.full((N * (D + 4) + 8,), FILL, device=DEV)
    iflat = torch.full((N * (D + 8) + 8,), IFILL, dtype=torch.int32, device=DEV)
    out, arg = flat[:N * (D + 4)].view(N, D + 4), iflat[:N * (D + 8)].view(N, D + 8)
    cases = {"D % 4": dict(D=6), "D = 0": dict(D=0), "D > 2048": dict(D=2052), "ldx < D": dict(ldx=60),
             "ldx % 4": dict(ldx=D + 3), "ldo < D": dict(ldo=60), "ldo % 4": dict(ldo=D + 2), "lda < D": dict(lda=60),
             "lda % 4": dict(lda=D + 6),
             "X alignment": dict(X=X.view(-1)[1:1 + (N - 1) * (D + 12)].view(N - 1, D + 12), N=N - 1, ldx=D + 12),
             "out alignment": dict(out=flat[1:1 + N * (D + 4)].view(N, D + 4)),
             "arg alignment": dict(arg=iflat[1:1 + N * (D + 8)].view(N, D + 8)),
             "negative N": dict(N=-1)}
    for why, kw in cases.items():
        a = dict(X=X, D=D, out=out, arg=arg)
        a.update(kw)
        rc, _, _, omx, orow = _fwd(g, a.pop("X"), a.pop("D"), **a)
        assert rc == MVML_ERR_INVALID and lib().mvml_last_error(), why
        assert bool((flat == FILL).all()) and bool((iflat == IFILL).all()), why
        assert int(omx.item()) == 0 and int(orow.abs().max().item()) == 0, why
    # out or arg aliasing X (the same rows, or rows that overlap them), or each other
    before = X.clone()
    for o, a_ in ((X, arg), (X[:, 4:], arg), (out, X.view(torch.int32)), (out, out.view(torch.int32))):
        rc = lib().mvml_sage_max_fwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(X), D + 12, 8, ptr(o), o.stride(0), ptr(a_),
                                     a_.stride(0), None, None, stream_ptr())
        torch.cuda.synchronize()
        assert rc == MVML_ERR_INVALID and b"alias" in lib().mvml_last_error()
    assert torch.equal(X, before) and bool((flat == FILL).all()) and bool((iflat == IFILL).all())
    assert lib().mvml_sage_max_fwd(N, None, ptr(g.in_src), ptr(X), D + 12, D, ptr(out), D + 4, ptr(arg), D + 8, None, None,
                                   stream_ptr()) == MVML_ERR_INVALID
    assert _fwd(g, X, D, N=0)[0] == 0  # an empty batch is no error and launches nothing

    # ---- the backward ----
    rc, _, arg_ok, _, _ = _fwd(g, X, D)
    assert rc == 0
    G = torch.randn((N, D + 12), device=DEV)
    P = torch.rand((N, D + 4), device=DEV)
    gflat = torch.full((N * (D + 4) + 8,), FILL, device=DEV)
    gX = gflat[:N * (D + 4)].view(N, D + 4)
    cases = {"D % 4": dict(D=6), "D = 0": dict(D=0), "D > 2048": dict(D=2052), "ldg < D": dict(ldg=60),
             "ldg % 4": dict(ldg=D + 3), "lda < D": dict(lda=60), "lda % 4": dict(lda=D + 6), "ldp < D": dict(ldp=60),
             "ldp % 4": dict(ldp=D + 2), "ldgx < D": dict(ldgx=60), "ldgx % 4": dict(ldgx=D + 2),
             "G alignment": dict(G=G.view(-1)[1:1 + (N - 1) * (D + 12)].view(N - 1, D + 12), N=N - 1, ldg=D + 12),
             "P alignment": dict(P=P.view(-1)[1:1 + (N - 1) * (D + 4)].view(N - 1, D + 4), N=N - 1, ldp=D + 4),
             "arg alignment": dict(arg=arg_ok.view(-1)[1:1 + (N - 1) * (D + 8)].view(N - 1, D + 8), N=N - 1, lda=D + 8),
             "gX alignment": dict(gX=gflat[1:1 + N * (D + 4)].view(N, D + 4)),
             "negative N": dict(N=-1)}
    for why, kw in cases.items():
        a = dict(G=G, arg=arg_ok, D=D, P=P, gX=gX)
        a.update(kw)
        rc, _ = _bwd(g, a.pop("G"), a.pop("arg"), a.pop("D"), **a)
        assert rc == MVML_ERR_INVALID and lib().mvml_last_error(), why
        assert bool((gflat == FILL).all()), why
    gb, ab = G.clone(), arg_ok.clone()
    for o in (G, G[:, 4:], arg_ok.view(torch.float32)):
        rc = lib().mvml_sage_max_bwd(N, ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(G), D + 12, ptr(arg_ok),
                                     D + 8, 8, None, 0, ptr(o), o.stride(0), stream_ptr())
        torch.cuda.synchronize()
        assert rc == MVML_ERR_INVALID and b"alias" in lib().mvml_last_error()
    assert torch.equal(G, gb) and torch.equal(arg_ok, ab)
    assert lib().mvml_sage_max_bwd(N, ptr(g.out_rowptr), ptr(g.out_dst), None, ptr(G), D + 12, ptr(arg_ok), D + 8, D, None,
                                   0, ptr(gX), D + 4, stream_ptr()) == MVML_ERR_INVALID
    assert _bwd(g, G, arg_ok, D, N=0)[0] == 0 and bool((gflat == FILL).all())
