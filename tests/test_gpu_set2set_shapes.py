"""Set2Set (csrc/set2set.hip) at every width class and on both input-gradient kernels, against
float64 (oracle.gnn_ref.set2set_ref).

The segment kernels hold a molecule's D columns as NV = ceil(D / 256) float4 slots per lane
(NV = 1 .. 4, D <= 1024); a D that is no multiple of 256 leaves the last slot partly masked
(D = 260: one live lane, 516: one, 772: one, 100: 25 lanes, 4: one lane of slot 0).
mvml_set2set_gx runs one wave per molecule for T <= 6 and D <= 512 (seg_gx_mol_kernel, the atoms'
coefficients 64 at a time) and one wave per atom otherwise (seg_gx_kernel): (7, 1) and every
D > 512 take the latter.  Molecule sizes sit on the 64-atom chunk edges of seg_gx_mol_kernel.

Bars: those of test_gpu_parity.test_set2set_parity (1e-5 norm-wise on the output, dX and every LSTM
parameter gradient)."""
import math

import numpy as np
import pytest
import torch

from _util import batch_of_sizes, graph_dict
from conftest import rel_err
from mvml_gat._lib import call, ptr, stream_ptr
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SIZES = [1, 2, 63, 64, 65, 130, 7]

CASES = [(4, 1, 1), (4, 6, 3), (100, 6, 3), (260, 1, 1), (260, 6, 3), (516, 6, 3), (772, 6, 3),
         (1024, 1, 1), (1024, 6, 3), (100, 7, 1), (516, 7, 1)]


@pytest.fixture(scope="module")
def batch():
    sb = batch_of_sizes(SIZES, seed=9)
    return sb, graph_dict(sb), sb.to_graph().to(DEV)


@pytest.mark.parametrize("D,n_iters,n_layers", CASES)
def test_set2set_widths(batch, D, n_iters, n_layers):
    from mvml_gat.nn import Set2Set
    sb, gd, g = batch
    torch.manual_seed(D + n_iters)
    s2s = Set2Set(D, n_iters, n_layers)
    X = torch.randn(int(sb.num_nodes.sum()), D, dtype=torch.float64)
    lstm64 = torch.nn.LSTM(2 * D, D, n_layers).double()
    lstm64.load_state_dict({k: v.double() for k, v in s2s.lstm.state_dict().items()})
    Xr = X.clone().requires_grad_()
    out_r = gnn_ref.set2set_ref(gd["node_offsets"], Xr, lstm64, n_iters)
    gout = torch.randn_like(out_r)
    out_r.backward(gout)
    s2s = s2s.to(DEV)
    Xp = X.float().to(DEV).requires_grad_()
    out_p = s2s(g, Xp)
    out_p.backward(gout.float().to(DEV))
    errs = {"out": rel_err(out_p, out_r), "dX": rel_err(Xp.grad, Xr.grad)}
    for (n, p), (n2, p2) in zip(s2s.lstm.named_parameters(), lstm64.named_parameters()):
        assert n == n2
        errs[n] = rel_err(p.grad, p2.grad)
    worst = max(errs, key=errs.get)
    print(f"S2S D={D} T={n_iters} L={n_layers} worst err/budget {worst}: {errs[worst] / TOL:.3f}")
    for n, e in errs.items():
        assert e < TOL, (n, e)


def _offsets(sizes):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)


@pytest.mark.parametrize("T", [1, 6])
@pytest.mark.parametrize("D", [4, 100, 260, 512])
def test_set2set_gx_paths_bitwise(D, T):
    """mvml_set2set_gx by molecule (node_offsets given) and by atom (node_graph only) on the same
    buffers: the same per-element expression and t order, so the same bits — and both within fp32
    rounding of the float64 sum."""
    offs = _offsets(SIZES)
    B, N = len(SIZES), int(offs[-1])
    gen = torch.Generator().manual_seed(D + T)
    ld = 2 * D + 4  # a row pitch past 2 D
    qs = torch.randn((T, B, ld), generator=gen)
    gqs = torch.randn((T, B, ld), generator=gen)
    al = torch.rand((T, N), generator=gen)
    ge = torch.randn((T, N), generator=gen)
    gid = torch.repeat_interleave(torch.arange(B), torch.as_tensor(SIZES))
    want = sum(al[t].double()[:, None] * gqs[t].double()[gid, D:2 * D]
               + ge[t].double()[:, None] * qs[t].double()[gid, :D] for t in range(T))
    d = {k: v.to(DEV) for k, v in dict(qs=qs, gqs=gqs, al=al, ge=ge, offs=offs, gid=gid.int()).items()}
    got = []
    for by_mol in (True, False):
        gX = torch.full((N + 1, D), float("nan"), device=DEV)  # one guard row
        call("mvml_set2set_gx", N, D, T, ptr(d["gid"]), ptr(d["offs"]) if by_mol else None, B if by_mol else 0,
             ptr(d["qs"]), ld, B * ld, ptr(d["gqs"]), ld, B * ld, ptr(d["al"]), ptr(d["ge"]), ptr(gX),
             stream_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(gX[N]).all(), "row past the last atom written"
        assert rel_err(gX[:N], want) < 1e-6
        got.append(gX[:N])
    assert torch.equal(got[0], got[1]), (got[0] - got[1]).abs().max().item()


@pytest.mark.parametrize("D", [4, 260, 1024])
def test_set2set_segment_without_atoms(D):
    """A molecule without atoms: r = 0, lse = -inf, g_q = g_qstar[:, :D], and no alpha / g_e entry
    is touched; the molecules around it against float64."""
    sizes = [3, 0, 65, 0]
    offs = _offsets(sizes)
    B, N = len(sizes), int(offs[-1])
    gen = torch.Generator().manual_seed(D)
    ld = 2 * D
    X = torch.randn((N, D), generator=gen)
    qstar = torch.randn((B, ld), generator=gen) / math.sqrt(D)
    g_qstar = torch.randn((B, ld), generator=gen)
    d_offs, d_X, d_q, d_gq = offs.to(DEV), X.to(DEV), qstar.to(DEV), g_qstar.to(DEV)
    d_q[:, D:] = 7.0  # r: to be overwritten
    lse = torch.full((B,), 7.0, device=DEV)
    st = stream_ptr()
    call("mvml_set2set_seg_fwd", B, D, ptr(d_offs), ptr(d_X), ptr(d_q), ld, ptr(lse), st)
    g_q = torch.full((B, D), 7.0, device=DEV)
    alpha = torch.full((N + 8,), 7.0, device=DEV)
    g_e = torch.full((N + 8,), 7.0, device=DEV)
    call("mvml_set2set_seg_bwd", B, D, ptr(d_offs), ptr(d_X), ptr(d_q), ld, ptr(lse), ptr(d_gq), ld, ptr(g_q), D,
         ptr(alpha), ptr(g_e), st)
    torch.cuda.synchronize()
    for b in (1, 3):
        assert bool((d_q[b, D:] == 0).all())
        assert lse[b].item() == -math.inf
        assert torch.equal(g_q[b], d_gq[b, :D])
    assert bool((alpha[N:] == 7.0).all()) and bool((g_e[N:] == 7.0).all())
    # the live molecules: float64 softmax readout and its gradient
    Xd, q = X.double(), qstar[:, :D].double().requires_grad_()
    for b in (0, 2):
        xs = Xd[offs[b]:offs[b + 1]]
        a = torch.softmax(xs @ q[b], 0)
        r = a @ xs
        assert rel_err(d_q[b, D:], r) < TOL
        assert rel_err(alpha[offs[b]:offs[b + 1]], a) < TOL
        gq, = torch.autograd.grad(r, q, g_qstar[b, D:].double())
        assert rel_err(g_q[b], g_qstar[b, :D].double() + gq[b]) < TOL
