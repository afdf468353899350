"""The GAT aggregation (mvml_gat_agg_fwd / mvml_gat_agg_bwd, csrc/gat_agg_*.hip) through the C ABI
against float64 (oracle.gnn_ref.gat_agg_ref, the same cut: Z, R and [el | er] given) over the
dispatch grid: every head count H in {1, 2, 4, 8}, the column chunks CW 32 / 16 / 8 / 4 of the
window kernels, the destination-wave forward's NJ = 1, 2, 3, 4, 8 slots with full and partly
masked last slots (and its H = 4, nj = 3 late-residual instance), the per-atom backward pair at
VPL 1 .. 8, the source-atom backwards at NJ 1 .. 4 (head mean) and 1 .. 8 (flatten), the LDS
backward (F % 32 == 0 only), the big windows (H <= 4, F % 16 == 0 only), and the head-mean shapes
past the destination-wave kernel's slots, which take the window kernels on every dst_fwd value.

One pytest case is one (shape, graph): the float64 reference is computed once and every kernel
path (option dst_fwd 0 / 1 / 2; the default backward, bwd_atomwise = 1, big_window = 0, mean_src
0 / 1 or flat_src 0 / 2) is compared with it.

Inputs: the projection rows Y are padded to a row pitch past their C columns and the pad is NaN;
out, attn and ALL of gY are pre-filled with a sentinel, which must survive in gY's columns past
C + 2H.  The LeakyReLU side of every (edge, head) is the kernels' own fp32 test
(el[src] + er[dst]) > 0 evaluated on the host from the same fp32 elr (one IEEE add: no edge can
disagree, so there is no flip allowance).

Bar (BASELINE.json north_star): 1e-5 norm-wise relative error per quantity (out, attn, and the
four gY blocks dZ | dR | d el | d er each against its own float64 block), or 4 x e32 where e32, the
error of gat_agg_ref run in fp32 on the CPU against its float64 run on this very batch, is larger.
"""
import functools

import pytest
import torch

from _util import batch_of_sizes
from conftest import rel_err
from mvml_gat._lib import lib, option
from oracle import gnn_ref
from test_gpu_parity_configs import _agg_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
FILL = -7777.0
MVML_ERR_INVALID = 1

# (4, 384), (8, 224): H F = 1536 / 1792, the source-atom flatten backward's NJ = 6 / 7 and the
# per-atom pair's VPL = 6 / 7 in the flatten modes (no other shape of the list reaches them)
FLATTEN = [(1, 4), (2, 12), (8, 8), (4, 20), (4, 48), (4, 72), (2, 160), (4, 132), (8, 96), (4, 256),
           (4, 260), (8, 256), (1, 2048), (4, 384), (8, 224)]
# (1, 1028): H = 1 past the destination-wave kernel's 4 slots (with (2, 516) and (2, 1024));
# (2, 260), (2, 388), (1, 516): the destination-wave forward's head-mean nj = 3 / 4 instances at
# H = 2 and nj = 3 at H = 1 (= the source-atom backward's NJ = 3), each with a partial last slot
MEAN = [(1, 4), (1, 260), (1, 1024), (2, 24), (8, 64), (4, 132), (4, 260), (4, 388), (4, 512), (8, 256),
        (2, 516), (2, 1024), (1, 1028), (2, 260), (2, 388), (1, 516)]
SHAPES = [(H, F, m) for m in (0, 2) for H, F in FLATTEN] + [(H, F, 1) for H, F in MEAN]

GRAPHS = {"mixed": lambda: batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1),
          "one_atom": lambda: batch_of_sizes([1], seed=2),
          "hubs": lambda: batch_of_sizes([150, 90], seed=7, hubs=True),
          "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109)}
HUB_GRAPHS = ("hubs", "table_overflow")


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(device graph, src, dst, in-CSR edge ids) — built once per graph."""
    g = GRAPHS[name]().to_graph().to(DEV)
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    order = torch.argsort(dst, stable=True)
    assert torch.equal(g.in_eid.cpu().long(), order), "in-CSR slots are the edges stably sorted by dst"
    assert torch.equal(g.in_src.cpu().long(), src[order])
    return g, src, dst


def _paths(mode):
    """(name, {option: value}) of every kernel path of one mode; the library defaults are
    dst_fwd 0, big_window 1, bwd_atomwise 0, mean_src 1, flat_src 0."""
    p = [("dst_fwd=0", {"dst_fwd": 0}), ("dst_fwd=1", {"dst_fwd": 1}), ("dst_fwd=2", {"dst_fwd": 2})]
    if mode == 1:
        # (bwd_atomwise / big_window reach the head-mean backward only with mean_src off)
        p += [("mean_src=0", {"dst_fwd": 0, "mean_src": 0}),
              ("mean_src=0,bwd_atomwise=1", {"dst_fwd": 0, "mean_src": 0, "bwd_atomwise": 1}),
              ("mean_src=0,big_window=0", {"dst_fwd": 0, "mean_src": 0, "big_window": 0}),
              ("mean_src=1,big_window=0", {"dst_fwd": 0, "mean_src": 1, "big_window": 0})]
    else:
        p += [("bwd_atomwise=1", {"dst_fwd": 0, "flat_src": 0, "bwd_atomwise": 1}),
              ("big_window=0", {"dst_fwd": 0, "flat_src": 0, "big_window": 0}),
              ("flat_src=2", {"dst_fwd": 0, "flat_src": 2})]
    base = {"dst_fwd": 0, "big_window": 1, "bwd_atomwise": 0, "mean_src": 1, "flat_src": 0, "dst_unr": 0}
    return [(n, {**base, **o}) for n, o in p]


class _options:
    """Several kernel-path options at once, restored on exit."""

    def __init__(self, opts):
        self.ctx = [option(k, v) for k, v in opts.items()]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)
        return False


def _inputs(N, H, F, mode, seed):
    """Seeded fp32 inputs on the host: Y [N, ldy] with the pad columns [C, ldy) NaN."""
    C = lib().mvml_gat_proj_cols(H, F, int(mode == 1))
    ldy = (C // 64 + 1) * 64  # always a pad
    gen = torch.Generator().manual_seed(seed)
    Y = torch.full((N, ldy), float("nan"))
    Y[:, :C] = torch.randn((N, C), generator=gen) * 0.3
    elr = torch.randn((N, 2 * H), generator=gen)
    bias = torch.randn(H * F, generator=gen) * 0.1
    g_out = torch.randn((N, F if mode == 1 else H * F), generator=gen)
    return C, {"Y": Y, "elr": elr, "bias": bias, "g_out": g_out}


def _reference(src, dst, inp, C, H, F, mode, branch, dtype):
    """(out, attn, dZ, dR, d el, d er) of gat_agg_ref in `dtype` on the CPU."""
    N, HF = inp["Y"].shape[0], H * F
    Z = inp["Y"][:, :HF].to(dtype).view(N, H, F).clone().requires_grad_()
    R = inp["Y"][:, HF:C].to(dtype).clone().requires_grad_()
    elr = inp["elr"].to(dtype).clone().requires_grad_()
    out, attn = gnn_ref.gat_agg_ref(src, dst, Z, R, elr, inp["bias"].to(dtype), H, F, mode, 0.2, branch)
    out.backward(inp["g_out"].to(dtype))
    return {"out": out.detach(), "attn": attn.detach(), "dZ": Z.grad.reshape(N, HF), "dR": R.grad,
            "d_el": elr.grad[:, :H], "d_er": elr.grad[:, H:]}


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("H,F,mode", SHAPES, ids=[f"H{H}-F{F}-mode{m}" for H, F, m in SHAPES])
def test_agg_against_float64(H, F, mode, graph):
    g, src, dst = _graph(graph)
    N = g.num_nodes()
    HF = H * F
    C, inp = _inputs(N, H, F, mode, seed=1000 * H + F + mode)
    CE = C + 2 * H
    e = inp["elr"]
    branch = (e[:, :H][src] + e[:, H:][dst]) > 0  # fp32, the kernels' own add and test
    ref = _reference(src, dst, inp, C, H, F, mode, branch, torch.float64)
    r32 = _reference(src, dst, inp, C, H, F, mode, branch, torch.float32)
    budget = {k: max(TOL, 4 * rel_err(r32[k], ref[k])) for k in ref}
    dev_in = {k: v.to(DEV) for k, v in inp.items()}

    results = {}
    worst = (0.0, None, None)
    for name, opts in _paths(mode):
        with _options(opts):
            res = _agg_outputs(None, H, F, mode, inputs=dev_in, fill=FILL, graph=g, full=True)
        out, attn, gY, omx, orow, gmx, grow, info = res
        assert info["rc_fwd"] == 0 and info["rc_bwd"] == 0, (name, info["error"])
        assert gY.shape[1] == CE
        got = {"out": out, "attn": attn, "dZ": gY[:, :HF], "dR": gY[:, HF:C], "d_el": gY[:, C:C + H],
               "d_er": gY[:, C + H:]}
        path_worst = (0.0, None)
        for k, v in got.items():
            assert torch.isfinite(v).all(), (name, k, "NaN / inf: a masked lane read the pad")
            err = rel_err(v, ref[k])
            if err / budget[k] > path_worst[0]:
                path_worst = (err / budget[k], k)
            assert err < budget[k], (name, k, err, budget[k])
        print(f"AGG H={H} F={F} mode={mode} graph={graph} path={name} worst={path_worst[1]} "
              f"err/budget={path_worst[0]:.3f}")
        if path_worst[0] > worst[0]:
            worst = (path_worst[0], path_worst[1], name)
        # the sentinel past the row's C + 2H columns is intact
        pad = info["gY"][:, CE:]
        assert pad.numel() == 0 or bool((pad == FILL).all()), (name, "gY columns past C + 2H written")
        # the folded maxima are, as bits, those of the fp32 tensors the call stored
        assert _bits(omx).item() == _bits(out.abs().max().reshape(1)).item(), (name, "out_amax")
        assert torch.equal(_bits(orow), _bits(out.abs().max(dim=1).values)), (name, "out_row_amax")
        assert _bits(gmx).item() == _bits(gY.abs().max().reshape(1)).item(), (name, "gy_amax")
        assert torch.equal(_bits(grow), _bits(gY.abs().max(dim=1).values)), (name, "gy_row_amax")
        results[name] = res
    print(f"worst err/budget {worst[1]} on {worst[2]}: {worst[0]:.3f}")

    # Bitwise promises of the source (csrc/gat_agg_*.hip): the destination-wave forward sums each row
    # in edge order from 0 as the window / gather kernels do, with softmax_pair's arithmetic — on
    # molecules without hubs (the gather kernel's hub pass sums long rows in another order) — and
    # its two kinds (softmax fused / as its own launch) agree on every graph.
    def same(a, b, idx, what):
        for i in idx:
            assert torch.equal(results[a][i], results[b][i]), (
                what, a, b, i, (results[a][i].double() - results[b][i].double()).abs().max().item())

    same("dst_fwd=1", "dst_fwd=2", (0, 1, 3, 4), "destination-wave kinds")
    if graph not in HUB_GRAPHS:
        same("dst_fwd=0", "dst_fwd=1", (0, 1, 3, 4), "destination wave vs windows")
    if mode == 1:
        # gat_mean_bwd_src_kernel: "bitwise the atomwise dZ"
        a, b = results["dst_fwd=0"][2][:, :HF], results["mean_src=0,bwd_atomwise=1"][2][:, :HF]
        assert torch.equal(a, b), ("mean_src dZ vs the per-atom pair", (a.double() - b.double()).abs().max().item())


@pytest.mark.parametrize("H,F,mode,why", [(3, 8, 0, "num_heads"), (4, 6, 1, "out_feats"), (4, 516, 2, "H*F"),
                                          (8, 260, 1, "H*F")])
def test_agg_refuses_unsupported_shape(H, F, mode, why):
    """A shape outside check_shapes' range: MVML_ERR_INVALID, mvml_last_error() names the limit,
    and nothing is written (never a wrong result)."""
    g, _, _ = _graph("mixed")
    N = g.num_nodes()
    C, inp = _inputs(N, H, F, mode, seed=0)
    dev_in = {k: v.to(DEV) for k, v in inp.items()}
    for opts in ({"dst_fwd": 0}, {"dst_fwd": 1}, {"dst_fwd": 2}):
        with _options(opts):
            out, attn, gY, omx, orow, gmx, grow, info = _agg_outputs(None, H, F, mode, inputs=dev_in, fill=FILL,
                                                                     graph=g, full=True)
        assert info["rc_fwd"] == MVML_ERR_INVALID and why in info["error"], info
        assert bool((out == FILL).all()) and bool((attn == FILL).all())
        assert int(omx.item()) == 0 and int(orow.abs().max().item()) == 0
    # the backward alone refuses too
    from mvml_gat._lib import ptr, stream_ptr
    L = lib()
    ws = torch.empty(max(L.mvml_gat_agg_bwd_workspace_size(g.num_edges(), H), 1), dtype=torch.uint8, device=DEV)
    ldg = info["gY"].shape[1]
    rc = L.mvml_gat_agg_bwd(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                            ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(dev_in["Y"]),
                            dev_in["Y"].shape[1], ptr(dev_in["elr"]), ptr(attn), ptr(out), ptr(dev_in["g_out"]),
                            H, F, 0.2, mode, ptr(info["gY"]), ldg, ptr(gmx), ptr(grow), ptr(ws), ws.numel(),
                            stream_ptr())
    torch.cuda.synchronize()
    assert rc == MVML_ERR_INVALID and why in L.mvml_last_error().decode(), L.mvml_last_error()
    assert bool((info["gY"] == FILL).all()) and int(gmx.item()) == 0 and int(grow.abs().max().item()) == 0
