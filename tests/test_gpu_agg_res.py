"""mvml_gat_agg_fwd_res / mvml_gat_agg_bwd_res (csrc/gat_agg_*.hip) through the C ABI: the residual
as an input of its own (R, its own row pitch), no residual (R = NULL), each with and without a
bias, against float64 (oracle.gnn_ref.gat_agg_ref at the same cut, with R = zeros for no residual
and bias = zeros for no bias), on every kernel-path option list of test_gpu_agg_shapes._paths.

Inputs: Y holds only [Z] and its row pad is NaN; R has a pitch of its own whose pad is NaN; out,
attn, gY and gR are views into buffers pre-filled with a sentinel that must survive around them,
in gY's columns past H F + 2H, in gR's row pad, and in the whole of a gR that is not formed (no
residual and no bias: gR = NULL is passed).  The LeakyReLU side of every (edge, head) is the
kernels' own fp32 test on the same fp32 elr, so there is no flip allowance.

Bar: the project's, per quantity (out, attn, dZ, dR where formed, d el, d er): 1e-5 norm-wise
relative error, or 4 x e32 (gat_agg_ref in fp32 on the CPU against its float64 run) where larger.

Maxima: gy_amax / gy_row_amax cover dZ, d el and d er — the columns of gY that exist — and not
a dR that lies apart from gY.

Shapes: the smallest that reach each instance family whose residual load differs — the
destination-wave forward's slot counts (flatten nj 1, 2, 3, 8 with full and partly masked last
slots; head mean nj 1 .. 4 and the 8-slot instances past them at H = 2 and H = 1), the LDS
backward (F % 32 == 0) and the per-atom pair (other F), the source-atom backwards.
"""
import ctypes

import pytest
import torch

from conftest import rel_err
from mvml_gat._lib import lib, ptr, stream_ptr
from oracle import gnn_ref
from test_gpu_agg_shapes import FILL, TOL, _bits, _graph, _options, _paths
from test_gpu_parity_configs import _agg_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MVML_ERR_INVALID = 1
GUARD = 64  # sentinel floats before and after every output buffer (256 B: keeps 16-B alignment)

FLATTEN = [(1, 4), (4, 20), (4, 48), (2, 160), (4, 132), (8, 256)]
MEAN = [(1, 4), (2, 24), (8, 64), (4, 132), (4, 512), (2, 516), (1, 1028)]
SHAPES = [(H, F, m) for m in (0, 2) for H, F in FLATTEN] + [(H, F, 1) for H, F in MEAN]
GRAPH_NAMES = ("mixed", "one_atom", "hubs")
# (residual given, bias given)
KINDS = [(True, True), (True, False), (False, True), (False, False)]


class _Guarded:
    """A [rows, ld] float32 device buffer between two sentinel guards, all pre-filled."""

    def __init__(self, rows, ld, dtype=torch.float32):
        self.whole = torch.full((rows * ld + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + rows * ld].view(rows, ld)

    def guards_intact(self):
        return bool((self.whole[:GUARD] == FILL).all()) and bool((self.whole[-GUARD:] == FILL).all())


def _host_inputs(N, H, F, mode, seed):
    HF, RW = H * F, (F if mode == 1 else H * F)
    gen = torch.Generator().manual_seed(seed)
    ldy = (HF // 64 + 1) * 64  # always a pad
    ldr = RW + 12              # a pitch of its own: a multiple of 4, not of 64
    Y = torch.full((N, ldy), float("nan"))
    Y[:, :HF] = torch.randn((N, HF), generator=gen) * 0.3
    R = torch.full((N, ldr), float("nan"))
    R[:, :RW] = torch.randn((N, RW), generator=gen) * 0.3
    return {"Y": Y, "R": R, "elr": torch.randn((N, 2 * H), generator=gen),
            "bias": torch.randn(HF, generator=gen) * 0.1,
            "g_out": torch.randn((N, F if mode == 1 else HF), generator=gen)}


def _reference(src, dst, inp, H, F, mode, branch, dtype, with_r, with_b):
    N, HF, RW = inp["Y"].shape[0], H * F, (F if mode == 1 else H * F)
    Z = inp["Y"][:, :HF].to(dtype).view(N, H, F).clone().requires_grad_()
    R = (inp["R"][:, :RW].to(dtype).clone() if with_r else torch.zeros((N, RW), dtype=dtype)).requires_grad_()
    bias = inp["bias"].to(dtype) if with_b else torch.zeros(HF, dtype=dtype)
    elr = inp["elr"].to(dtype).clone().requires_grad_()
    out, attn = gnn_ref.gat_agg_ref(src, dst, Z, R, elr, bias, H, F, mode, 0.2, branch)
    out.backward(inp["g_out"].to(dtype))
    return {"out": out.detach(), "attn": attn.detach(), "dZ": Z.grad.reshape(N, HF), "dR": R.grad,
            "d_el": elr.grad[:, :H], "d_er": elr.grad[:, H:]}


def _call_res(g, H, F, mode, dev, R=None, ldr=0, bias=None, form_gr=True, elr_col=None, bufs=None):
    """One mvml_gat_agg_fwd_res + mvml_gat_agg_bwd_res on guarded, sentinel-filled outputs."""
    L = lib()
    N, E, HF = g.num_nodes(), g.num_edges(), H * F
    oc, RW = (F if mode == 1 else HF), (F if mode == 1 else HF)
    elc = HF if elr_col is None else elr_col
    ldg = ((elc + 2 * H) // 64 + 1) * 64
    ldgr = RW + 8
    b = bufs or {"out": _Guarded(N, oc), "attn": _Guarded(E, H), "gY": _Guarded(N, ldg), "gR": _Guarded(N, ldgr)}
    omx = torch.zeros(1, dtype=torch.int32, device=DEV)
    orow = torch.zeros(N, dtype=torch.int32, device=DEV)
    gmx = torch.zeros(1, dtype=torch.int32, device=DEV)
    grow = torch.zeros(N, dtype=torch.int32, device=DEV)
    st = stream_ptr()
    Y = dev["Y"]
    rc_f = L.mvml_gat_agg_fwd_res(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                  ptr(Y), Y.shape[1], H, F, ptr(dev["elr"]), R, ldr, ptr(bias), 0.2, mode,
                                  ptr(b["out"].t), ptr(b["attn"].t), ptr(omx), ptr(orow), st)
    err = L.mvml_last_error().decode(errors="replace") if rc_f else ""
    rc_b = None
    if rc_f == 0:
        wsz = L.mvml_gat_agg_bwd_workspace_size(E, H)
        ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=DEV)
        rc_b = L.mvml_gat_agg_bwd_res(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                      ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), Y.shape[1],
                                      ptr(dev["elr"]), ptr(b["attn"].t), ptr(b["out"].t), ptr(dev["g_out"]), H, F,
                                      0.2, mode, ptr(b["gY"].t), ldg, elc,
                                      ptr(b["gR"].t) if form_gr else None, ldgr if form_gr else 0,
                                      ptr(gmx), ptr(grow), ptr(ws), wsz, st)
        err = L.mvml_last_error().decode(errors="replace") if rc_b else ""
    torch.cuda.synchronize()
    return b, omx, orow, gmx, grow, {"rc_fwd": rc_f, "rc_bwd": rc_b, "error": err, "ldg": ldg, "ldgr": ldgr}


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("H,F,mode", SHAPES, ids=[f"H{H}-F{F}-mode{m}" for H, F, m in SHAPES])
def test_agg_res_against_float64(H, F, mode, graph):
    g, src, dst = _graph(graph)
    N, HF, RW = g.num_nodes(), H * F, (F if mode == 1 else H * F)
    CE = HF + 2 * H
    inp = _host_inputs(N, H, F, mode, seed=2000 * H + F + mode)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    e = inp["elr"]
    branch = (e[:, :H][src] + e[:, H:][dst]) > 0  # fp32, the kernels' own add and test
    worst = (0.0, None, None, None)
    for with_r, with_b in KINDS:
        ref = _reference(src, dst, inp, H, F, mode, branch, torch.float64, with_r, with_b)
        r32 = _reference(src, dst, inp, H, F, mode, branch, torch.float32, with_r, with_b)
        budget = {k: max(TOL, 4 * rel_err(r32[k], ref[k])) for k in ref}
        form_gr = with_r or with_b
        kind = f"R={'given' if with_r else 'NULL'},bias={'given' if with_b else 'NULL'}"
        for name, opts in _paths(mode):
            with _options(opts):
                b, omx, orow, gmx, grow, info = _call_res(
                    g, H, F, mode, dev, R=ptr(dev["R"]) if with_r else None,
                    ldr=dev["R"].shape[1] if with_r else 0, bias=dev["bias"] if with_b else None,
                    form_gr=form_gr)
            where = (kind, name)
            assert info["rc_fwd"] == 0 and info["rc_bwd"] == 0, (where, info["error"])
            out, attn, gY, gR = b["out"].t, b["attn"].t, b["gY"].t, b["gR"].t
            got = {"out": out, "attn": attn, "dZ": gY[:, :HF], "d_el": gY[:, HF:HF + H], "d_er": gY[:, HF + H:CE]}
            if form_gr:
                got["dR"] = gR[:, :RW]
            for k, v in got.items():
                assert torch.isfinite(v).all(), (where, k, "NaN / inf: a masked lane read a pad")
                err = rel_err(v, ref[k])
                if err / budget[k] > worst[0]:
                    worst = (err / budget[k], k, kind, name)
                assert err < budget[k], (where, k, err, budget[k])
            # sentinels: around every buffer, past gY's columns, in gR's pad / an unformed gR
            for k, buf in b.items():
                assert buf.guards_intact(), (where, k, "written outside the buffer")
            assert bool((gY[:, CE:] == FILL).all()), (where, "gY columns past H F + 2H written")
            if form_gr:
                assert bool((gR[:, RW:] == FILL).all()), (where, "gR's row pad written")
            else:
                assert bool((gR == FILL).all()), (where, "a gR that is not formed was written")
            # the folded maxima are, as bits, those of the fp32 tensors the call stored
            assert _bits(omx).item() == _bits(out.abs().max().reshape(1)).item(), (where, "out_amax")
            assert torch.equal(_bits(orow), _bits(out.abs().max(dim=1).values)), (where, "out_row_amax")
            assert _bits(gmx).item() == _bits(gY[:, :CE].abs().max().reshape(1)).item(), (where, "gy_amax")
            assert torch.equal(_bits(grow), _bits(gY[:, :CE].abs().max(dim=1).values)), (where, "gy_row_amax")
    print(f"AGG_RES H={H} F={F} mode={mode} graph={graph} worst err/budget {worst[1]} "
          f"({worst[2]}, {worst[3]}): {worst[0]:.3f}")


@pytest.mark.parametrize("opts", [{}, {"dst_fwd": 2, "flat_src": 2}], ids=["defaults", "python-policy"])
@pytest.mark.parametrize("graph", ["mixed", "hubs"])
@pytest.mark.parametrize("H,F,mode", [(4, 48, 0), (2, 160, 2), (4, 132, 1)])
def test_res_entries_in_projection_layout_are_bitwise_the_old_entries(H, F, mode, graph, opts):
    """R = Y + H F, gR = gY + H F and the el / er column at C: out, attn, the whole of gY (pad
    included) and the four maxima are bitwise those of mvml_gat_agg_fwd / mvml_gat_agg_bwd."""
    from test_gpu_agg_shapes import _inputs
    g, _, _ = _graph(graph)
    N, HF = g.num_nodes(), H * F
    C, inp = _inputs(N, H, F, mode, seed=77 + F)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    with _options(opts):
        out0, attn0, _, omx0, orow0, gmx0, grow0, info0 = _agg_outputs(None, H, F, mode, inputs=dev, fill=FILL,
                                                                       graph=g, full=True)
        assert info0["rc_fwd"] == 0 and info0["rc_bwd"] == 0, info0["error"]
        ldg = info0["gY"].shape[1]
        bufs = {"out": _Guarded(N, out0.shape[1]), "attn": _Guarded(g.num_edges(), H), "gY": _Guarded(N, ldg)}
        Y = dev["Y"]
        gYv = bufs["gY"].t
        L = lib()
        st = stream_ptr()
        omx = torch.zeros(1, dtype=torch.int32, device=DEV)
        orow = torch.zeros(N, dtype=torch.int32, device=DEV)
        gmx = torch.zeros(1, dtype=torch.int32, device=DEV)
        grow = torch.zeros(N, dtype=torch.int32, device=DEV)
        rc = L.mvml_gat_agg_fwd_res(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                    ptr(Y), Y.shape[1], H, F, ptr(dev["elr"]),
                                    ctypes.c_void_p(Y.data_ptr() + 4 * HF), Y.shape[1], ptr(dev["bias"]), 0.2, mode,
                                    ptr(bufs["out"].t), ptr(bufs["attn"].t), ptr(omx), ptr(orow), st)
        assert rc == 0, L.mvml_last_error()
        wsz = L.mvml_gat_agg_bwd_workspace_size(g.num_edges(), H)
        ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=DEV)
        rc = L.mvml_gat_agg_bwd_res(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                    ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), Y.shape[1],
                                    ptr(dev["elr"]), ptr(bufs["attn"].t), ptr(bufs["out"].t), ptr(dev["g_out"]),
                                    H, F, 0.2, mode, ptr(gYv), ldg, C, ctypes.c_void_p(gYv.data_ptr() + 4 * HF), ldg,
                                    ptr(gmx), ptr(grow), ptr(ws), wsz, st)
        assert rc == 0, L.mvml_last_error()
        torch.cuda.synchronize()
    for name, a, b in (("out", bufs["out"].t, out0), ("attn", bufs["attn"].t, attn0), ("gY", gYv, info0["gY"]),
                       ("out_amax", omx, omx0), ("out_row_amax", orow, orow0), ("gy_amax", gmx, gmx0),
                       ("gy_row_amax", grow, grow0)):
        assert torch.equal(_bits(a), _bits(b)), name
    assert all(buf.guards_intact() for buf in bufs.values())


def _untouched(b, omx, orow, gmx, grow):
    return (all(bool((buf.whole == FILL).all()) for buf in b.values()) and int(omx.item()) == 0
            and int(orow.abs().max().item()) == 0 and int(gmx.item()) == 0 and int(grow.abs().max().item()) == 0)


@pytest.mark.parametrize("H,F,mode,why", [(3, 8, 0, "num_heads"), (4, 6, 1, "out_feats"), (4, 516, 2, "H*F"),
                                          (8, 260, 1, "H*F")])
def test_res_entries_refuse_unsupported_shape(H, F, mode, why):
    g, _, _ = _graph("mixed")
    inp = _host_inputs(g.num_nodes(), H, F, mode, seed=0)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    b, omx, orow, gmx, grow, info = _call_res(g, H, F, mode, dev, R=ptr(dev["R"]), ldr=dev["R"].shape[1],
                                              bias=dev["bias"])
    assert info["rc_fwd"] == MVML_ERR_INVALID and why in info["error"], info
    assert _untouched(b, omx, orow, gmx, grow)


@pytest.mark.parametrize("mode", [0, 1])
def test_res_entries_refuse_misaligned_residual(mode):
    """R off a 16-byte boundary, or a row stride that is no multiple of 4 floats (rows would leave
    the boundary), gives MVML_ERR_INVALID before any launch; so does such a gR in the backward."""
    H, F = 4, 48
    g, _, _ = _graph("mixed")
    N, HF = g.num_nodes(), H * F
    inp = _host_inputs(N, H, F, mode, seed=1)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    R = dev["R"]
    for rp, ldr in ((ctypes.c_void_p(R.data_ptr() + 4), R.shape[1] - 4), (ptr(R), R.shape[1] - 1),
                    (ptr(R), (F if mode == 1 else HF) - 4)):
        b, omx, orow, gmx, grow, info = _call_res(g, H, F, mode, dev, R=rp, ldr=ldr, bias=dev["bias"])
        assert info["rc_fwd"] == MVML_ERR_INVALID and "R must be" in info["error"], info
        assert _untouched(b, omx, orow, gmx, grow)
    # the backward alone: a forward that succeeds, then a misaligned gR
    L = lib()
    b, omx, orow, gmx, grow, info = _call_res(g, H, F, mode, dev, R=ptr(R), ldr=R.shape[1], bias=dev["bias"])
    assert info["rc_fwd"] == 0 and info["rc_bwd"] == 0, info
    gY2, gR2 = _Guarded(N, info["ldg"]), _Guarded(N, info["ldgr"])
    gmx2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    grow2 = torch.zeros(N, dtype=torch.int32, device=DEV)
    wsz = L.mvml_gat_agg_bwd_workspace_size(g.num_edges(), H)
    ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=DEV)
    for gp, ldgr in ((ctypes.c_void_p(gR2.t.data_ptr() + 8), info["ldgr"] - 4), (ptr(gR2.t), info["ldgr"] - 2)):
        rc = L.mvml_gat_agg_bwd_res(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                    ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(dev["Y"]),
                                    dev["Y"].shape[1], ptr(dev["elr"]), ptr(b["attn"].t), ptr(b["out"].t),
                                    ptr(dev["g_out"]), H, F, 0.2, mode, ptr(gY2.t), info["ldg"], HF, gp, ldgr,
                                    ptr(gmx2), ptr(grow2), ptr(ws), wsz, stream_ptr())
        torch.cuda.synchronize()
        assert rc == MVML_ERR_INVALID and "gR must be" in L.mvml_last_error().decode(), L.mvml_last_error()
        assert bool((gY2.whole == FILL).all()) and bool((gR2.whole == FILL).all())
        assert int(gmx2.item()) == 0 and int(grow2.abs().max().item()) == 0
