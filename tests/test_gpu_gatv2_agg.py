"""mvml_gatv2_agg_fwd / mvml_gatv2_agg_bwd (csrc/gatv2_agg.hip) through the C ABI against float64
(tests/_gatv2_ref.gatv2_agg_ref at the same cut: ZL, ZR, R and the attention vector given).

Inputs, seeded per case: ZL, ZR, R = 0.3 randn, attn_vec = 3 randn / sqrt(F), g_out = randn; ZL and
ZR are column blocks of one row buffer whose pad is NaN, R has a pitch of its own whose pad is NaN.
Every output is a view into a buffer pre-filled with a sentinel that must survive around it and in
the pad columns of gY = [gZL | gZR | pad] and gR.

The LeakyReLU side of every (edge, head, f) is p = ZL[u] + ZR[v] > 0, one IEEE fp32 add of given
inputs, evaluated on the host in fp32 and given to the reference as `branch`; the float64 sum of
the same fp32 inputs has the same sign (asserted), so there is no flip allowance.

Bar: norm-wise rel_err <= max(1e-5, 4 e32) per quantity (out, attn, gZL, gZR, gR, g_attn_vec, each
against its own float64 block); e32 is the reference in float32 against its float64 run.

Kernel instances (the dispatch picks (H, NJ), NJ = 1 / 2 / 3 / 4 / 6 / 8 column slots for H F <= 256 /
512 / 768 / 1024 / 1536 / 2048; the forward also has a head-mean form of each, the backward kernels
take the mode at run time) -> shapes that run them:
  FULL = (H, 256 NJ / H) [last slot full] and PART = (H, 256 NJ / H - 4) [last slot partly masked]
  for every H in {1, 2, 4, 8} and NJ in {1, 2, 3, 4, 6, 8}, in mode 2 and in mode 1 on "mixed"; the
  partly masked one of each on the other three graphs; "big_hub" (one atom with 202 in- and
  out-edges: four 64-edge chunks) runs one shape per slot count NJ = 1, 2, 3, 6, 8.
  The listed shapes: flatten (1,4) (2,12) (8,8) (4,20) -> NJ 1 partial; (4,64) -> (4, NJ 1) full;
  (4,132) -> (4, NJ 3) partial; (8,96) -> (8, NJ 3) full; (4,260) -> (4, NJ 6) partial (fifth slot
  partial, sixth masked); (4,384) -> (4, NJ 6) full; (8,224) -> (8, NJ 8) partial; (8,256) (1,2048)
  -> NJ 8 full.  Mean (1,4) (2,24) -> NJ 1; (8,64) -> (8, NJ 2) full; (4,132) -> NJ 3; (2,516) ->
  (2, NJ 6) partial; (4,388) -> (4, NJ 8) partial; (8,256) (2,1024) -> NJ 8 full.
"""
import ctypes
import functools

import pytest
import torch

from _gatv2_ref import gatv2_agg_ref
from _util import batch_of_sizes
from conftest import rel_err
from mvml_gat import batch, bigraph_from_bonds
from mvml_gat._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
FILL = -7777.0
GUARD = 64
MVML_ERR_INVALID = 1
SLOPE = 0.2

FLATTEN = [(1, 4), (2, 12), (8, 8), (4, 20), (4, 64), (4, 132), (8, 96), (4, 260), (8, 256), (4, 384),
           (8, 224), (1, 2048)]
MEAN = [(1, 4), (2, 24), (8, 64), (4, 132), (4, 388), (2, 516), (8, 256), (2, 1024)]
FULL = [(H, 256 * NJ // H) for H in (1, 2, 4, 8) for NJ in (1, 2, 3, 4, 6, 8)]
PART = [(H, 256 * NJ // H - 4) for H in (1, 2, 4, 8) for NJ in (1, 2, 3, 4, 6, 8)]


def _dedupe(seq):
    return list(dict.fromkeys(seq))


SHAPES = _dedupe([(H, F, m) for m in (0, 2) for H, F in FLATTEN] + [(H, F, 1) for H, F in MEAN]
                 + [(H, F, m) for m in (2, 1) for H, F in FULL + PART])
SUBSET = [(H, F, m) for m in (2, 1) for H, F in PART] + [(4, 20, 0), (4, 132, 0)]


def _no_self_loops():
    """Two molecules without self-loops: atom 3 of the first has no edge at all, so it is a
    destination without in-edges (and a source without out-edges)."""
    return batch([bigraph_from_bonds(4, [(0, 1), (1, 2)], add_self_loop=False),
                  bigraph_from_bonds(5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)], add_self_loop=False)])


GRAPHS = {"mixed": lambda: batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1).to_graph(),
          "one_atom": lambda: batch_of_sizes([1], seed=2).to_graph(),
          "hubs": lambda: batch_of_sizes([150, 90], seed=7, hubs=True).to_graph(),
          # one hub bonded to 200 atoms: four 64-edge chunks by destination and by source, the
          # ordered sums carried across them
          "big_hub": lambda: batch_of_sizes([220, 30], seed=8, hubs=True, partners=200).to_graph(),
          "zero_in_degree": _no_self_loops}


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = GRAPHS[name]().to(DEV)
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    assert torch.equal(g.in_eid.cpu().long(), torch.argsort(dst, stable=True))
    if name == "zero_in_degree":
        assert g.has_zero_in_degree and int(torch.bincount(dst, minlength=g.num_nodes())[3]) == 0
    if name == "big_hub":
        assert int(torch.bincount(dst).max()) > 192 and int(torch.bincount(src).max()) > 192
    if name == "hubs":
        assert int(torch.bincount(dst).max()) > 64  # past one 64-edge chunk: the spill path
    return g, src, dst


class _Guarded:
    """A [rows, ld] float32 device buffer between two sentinel guards, all pre-filled."""

    def __init__(self, rows, ld):
        self.whole = torch.full((rows * ld + 2 * GUARD,), FILL, dtype=torch.float32, device=DEV)
        self.t = self.whole[GUARD:GUARD + rows * ld].view(rows, ld)

    def guards_intact(self):
        return bool((self.whole[:GUARD] == FILL).all()) and bool((self.whole[-GUARD:] == FILL).all())


def _host_inputs(N, H, F, mode, seed):
    HF, RW = H * F, (F if mode == 1 else H * F)
    gen = torch.Generator().manual_seed(seed)
    ldy = (2 * HF // 64 + 1) * 64  # [ZL | ZR | NaN pad]
    Y = torch.full((N, ldy), float("nan"))
    Y[:, :2 * HF] = torch.randn((N, 2 * HF), generator=gen) * 0.3
    R = torch.full((N, RW + 12), float("nan"))
    R[:, :RW] = torch.randn((N, RW), generator=gen) * 0.3
    return {"Y": Y, "R": R, "av": 3 * torch.randn(HF, generator=gen) / F ** 0.5,
            "g_out": torch.randn((N, F if mode == 1 else HF), generator=gen)}


def _reference(src, dst, inp, H, F, mode, branch, dtype, shared=False, with_r=True):
    HF, RW = H * F, (F if mode == 1 else H * F)
    ZL = inp["Y"][:, :HF].to(dtype).clone().requires_grad_()
    ZR = ZL if shared else inp["Y"][:, HF:2 * HF].to(dtype).clone().requires_grad_()
    R = inp["R"][:, :RW].to(dtype).clone().requires_grad_() if with_r else None
    av = inp["av"].to(dtype).clone().requires_grad_()
    if shared:  # gZL and gZR apart, as the kernels write them: two leaves with equal values
        ZR = ZL.detach().clone().requires_grad_()
    out, a = gatv2_agg_ref(src, dst, ZL, ZR, R, av, H, F, mode, SLOPE, branch)
    out.backward(inp["g_out"].to(dtype))
    ref = {"out": out.detach(), "attn": a.detach(), "gZL": ZL.grad, "gZR": ZR.grad, "g_attn_vec": av.grad}
    if with_r:
        ref["gR"] = R.grad
    return ref


def _branch(src, dst, inp, H, F, shared=False):
    """The kernels' own fp32 side of every (edge, head, f); the float64 sum agrees in sign."""
    HF = H * F
    N = inp["Y"].shape[0]
    ZL = inp["Y"][:, :HF]
    ZR = ZL if shared else inp["Y"][:, HF:2 * HF]
    p32 = ZL[src] + ZR[dst]
    p64 = ZL.double()[src] + ZR.double()[dst]
    # (an exact zero — equal and opposite inputs — is on the `slope` side in both)
    assert torch.equal(p32 > 0, p64 > 0)
    return (p32 > 0).view(-1, H, F)


def _call(g, H, F, mode, dev, shared=False, R=None, ldr=0, form_gr=True, bufs=None):
    """One mvml_gatv2_agg_fwd + mvml_gatv2_agg_bwd on guarded, sentinel-filled outputs."""
    L = lib()
    N, E, HF = g.num_nodes(), g.num_edges(), H * F
    oc, RW = (F if mode == 1 else HF), (F if mode == 1 else HF)
    ldg = (2 * HF // 64 + 1) * 64
    ldgr = RW + 8
    b = bufs or {"out": _Guarded(N, oc), "attn": _Guarded(E, H), "gY": _Guarded(N, ldg), "gR": _Guarded(N, ldgr),
                 "g_attn_vec": _Guarded(1, HF)}
    st = stream_ptr()
    Y = dev["Y"]
    ldy = Y.shape[1]
    zr = ptr(Y) if shared else ctypes.c_void_p(Y.data_ptr() + 4 * HF)
    rc_f = L.mvml_gatv2_agg_fwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(Y), ldy, zr, ldy, H, F, ptr(dev["av"]),
                                R, ldr, SLOPE, mode, ptr(b["out"].t), ptr(b["attn"].t), st)
    err = L.mvml_last_error().decode(errors="replace") if rc_f else ""
    rc_b = None
    if rc_f == 0:
        wsz = L.mvml_gatv2_agg_bwd_workspace_size(N, E, H, F)
        ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=DEV)
        gy = b["gY"].t
        rc_b = L.mvml_gatv2_agg_bwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
                                    ptr(g.out_inslot), E, ptr(Y), ldy, zr, ldy, H, F, ptr(dev["av"]),
                                    ptr(b["attn"].t), ptr(b["out"].t), ptr(dev["g_out"]), SLOPE, mode,
                                    ptr(gy), ldg, ctypes.c_void_p(gy.data_ptr() + 4 * HF), ldg,
                                    ptr(b["gR"].t) if form_gr else None, ldgr if form_gr else 0,
                                    ptr(b["g_attn_vec"].t), ptr(ws), wsz, st)
        err = L.mvml_last_error().decode(errors="replace") if rc_b else ""
    torch.cuda.synchronize()
    return b, {"rc_fwd": rc_f, "rc_bwd": rc_b, "error": err}


def _got(b, H, F, mode, with_r=True):
    HF, RW = H * F, (F if mode == 1 else H * F)
    got = {"out": b["out"].t, "attn": b["attn"].t, "gZL": b["gY"].t[:, :HF], "gZR": b["gY"].t[:, HF:2 * HF],
           "g_attn_vec": b["g_attn_vec"].t.view(-1)}
    if with_r:
        got["gR"] = b["gR"].t[:, :RW]
    return got


def _check(g, src, dst, H, F, mode, seed, shared=False, with_r=True, tag=""):
    N, HF, RW = g.num_nodes(), H * F, (F if mode == 1 else H * F)
    inp = _host_inputs(N, H, F, mode, seed)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    branch = _branch(src, dst, inp, H, F, shared)
    ref = _reference(src, dst, inp, H, F, mode, branch, torch.float64, shared, with_r)
    r32 = _reference(src, dst, inp, H, F, mode, branch, torch.float32, shared, with_r)
    budget = {k: max(TOL, 4 * rel_err(r32[k], ref[k])) for k in ref}
    b, info = _call(g, H, F, mode, dev, shared, R=ptr(dev["R"]) if with_r else None,
                    ldr=dev["R"].shape[1] if with_r else 0, form_gr=with_r)
    assert info["rc_fwd"] == 0 and info["rc_bwd"] == 0, info["error"]
    worst = (0.0, None)
    for k, v in _got(b, H, F, mode, with_r).items():
        assert torch.isfinite(v).all(), (k, "NaN / inf: a masked lane read a pad")
        err = rel_err(v, ref[k])
        if err / budget[k] > worst[0]:
            worst = (err / budget[k], k)
        print(f"GATV2_AGG{tag} H={H} F={F} mode={mode} {k}: err {err:.3e} budget {budget[k]:.3e}")
        assert err <= budget[k], (k, err, budget[k])
    for k, buf in b.items():
        assert buf.guards_intact(), (k, "written outside the buffer")
    assert bool((b["gY"].t[:, 2 * HF:] == FILL).all()), "gY's pad columns written"
    if with_r:
        assert bool((b["gR"].t[:, RW:] == FILL).all()), "gR's row pad written"
    else:
        assert bool((b["gR"].whole == FILL).all()), "a gR that is not formed was written"
    deg = torch.bincount(dst, minlength=N)
    if bool((deg == 0).any()):  # no in-edges: rst is the residual alone and gZR is zero
        z = (deg == 0).to(DEV)
        assert bool((b["gY"].t[:, HF:2 * HF][z] == 0).all())
        want = dev["R"][:, :RW][z] if with_r else torch.zeros_like(b["out"].t[z])
        if mode == 0:  # (ELU of the residual: expm1 of two libraries, not bitwise)
            want = torch.nn.functional.elu(want)
        assert torch.allclose(b["out"].t[z], want, rtol=1e-6, atol=0)
    print(f"GATV2_AGG{tag} H={H} F={F} mode={mode} worst err/budget {worst[1]}: {worst[0]:.3f}")
    return b, dev


@pytest.mark.parametrize("H,F,mode", SHAPES, ids=[f"H{H}-F{F}-mode{m}" for H, F, m in SHAPES])
def test_agg_against_float64_mixed(H, F, mode):
    g, src, dst = _graph("mixed")
    _check(g, src, dst, H, F, mode, seed=3000 * H + F + mode)


@pytest.mark.parametrize("graph", ["one_atom", "hubs", "zero_in_degree"])
@pytest.mark.parametrize("H,F,mode", SUBSET, ids=[f"H{H}-F{F}-mode{m}" for H, F, m in SUBSET])
def test_agg_against_float64_other_graphs(H, F, mode, graph):
    g, src, dst = _graph(graph)
    _check(g, src, dst, H, F, mode, seed=5000 * H + F + mode, tag=f" graph={graph}")


@pytest.mark.parametrize("H,F,mode", [(4, 20, 0), (2, 160, 2), (4, 132, 1), (8, 96, 2), (4, 384, 1), (8, 256, 2)])
def test_agg_against_float64_four_chunk_hub(H, F, mode):
    g, src, dst = _graph("big_hub")
    _check(g, src, dst, H, F, mode, seed=7000 * H + F + mode, tag=" graph=big_hub")


@pytest.mark.parametrize("graph", ["mixed", "hubs"])
@pytest.mark.parametrize("H,F,mode", [(4, 20, 0), (2, 160, 2), (4, 132, 1), (8, 256, 1)])
def test_shared_weights_and_no_residual(H, F, mode, graph):
    g, src, dst = _graph(graph)
    _check(g, src, dst, H, F, mode, seed=11 + F, shared=True, tag=" ZR==ZL")
    _check(g, src, dst, H, F, mode, seed=12 + F, with_r=False, tag=" R=NULL")
    _check(g, src, dst, H, F, mode, seed=13 + F, shared=True, with_r=False, tag=" ZR==ZL,R=NULL")


@pytest.mark.parametrize("graph", ["mixed", "hubs", "big_hub"])
@pytest.mark.parametrize("H,F,mode", [(4, 48, 0), (8, 96, 2), (4, 388, 1)])
def test_two_runs_are_bitwise_equal(H, F, mode, graph):
    g, src, dst = _graph(graph)
    inp = _host_inputs(g.num_nodes(), H, F, mode, seed=21 + F)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    runs = []
    for _ in range(2):
        b, info = _call(g, H, F, mode, dev, R=ptr(dev["R"]), ldr=dev["R"].shape[1])
        assert info["rc_fwd"] == 0 and info["rc_bwd"] == 0, info["error"]
        runs.append(b)
    for k in runs[0]:
        assert torch.equal(runs[0][k].whole.view(torch.int32), runs[1][k].whole.view(torch.int32)), k


def _untouched(b):
    return all(bool((buf.whole == FILL).all()) for buf in b.values())


@pytest.mark.parametrize("H,F,mode,why", [(3, 8, 0, "num_heads"), (4, 6, 1, "out_feats"), (1, 2052, 2, "H*F")])
def test_entries_refuse_unsupported_shape(H, F, mode, why):
    g, _, _ = _graph("mixed")
    inp = _host_inputs(g.num_nodes(), H, F, mode, seed=0)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    b, info = _call(g, H, F, mode, dev, R=ptr(dev["R"]), ldr=dev["R"].shape[1])
    assert info["rc_fwd"] == MVML_ERR_INVALID and why in info["error"], info
    assert _untouched(b)
    # the backward alone refuses it too
    L = lib()
    N, E, HF = g.num_nodes(), g.num_edges(), H * F
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    Y, gy = dev["Y"], b["gY"].t
    rc = L.mvml_gatv2_agg_bwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
                              ptr(g.out_inslot), E, ptr(Y), Y.shape[1], ptr(Y), Y.shape[1], H, F, ptr(dev["av"]),
                              ptr(b["attn"].t), ptr(b["out"].t), ptr(dev["g_out"]), SLOPE, mode, ptr(gy),
                              gy.shape[1], ctypes.c_void_p(gy.data_ptr() + 4 * (HF // 4 * 4)), gy.shape[1], None, 0,
                              ptr(b["g_attn_vec"].t), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert rc == MVML_ERR_INVALID and why in L.mvml_last_error().decode(), L.mvml_last_error()
    assert _untouched(b)


@pytest.mark.parametrize("mode", [0, 1])
def test_entries_refuse_misaligned_residual(mode):
    H, F = 4, 48
    g, _, _ = _graph("mixed")
    inp = _host_inputs(g.num_nodes(), H, F, mode, seed=1)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    R = dev["R"]
    for rp, ldr in ((ctypes.c_void_p(R.data_ptr() + 4), R.shape[1] - 4), (ptr(R), R.shape[1] - 1),
                    (ptr(R), (F if mode == 1 else H * F) - 4)):
        b, info = _call(g, H, F, mode, dev, R=rp, ldr=ldr)
        assert info["rc_fwd"] == MVML_ERR_INVALID and "R must be" in info["error"], info
        assert _untouched(b)


def test_backward_refuses_overlapping_gzl_gzr():
    """gZL and gZR never alias: equal pointers, column blocks less than H F apart in one row
    buffer and a block that runs past the shared pitch are refused before any launch."""
    H, F, mode = 4, 48, 2
    HF = H * F
    g, _, _ = _graph("mixed")
    N, E = g.num_nodes(), g.num_edges()
    inp = _host_inputs(N, H, F, mode, seed=2)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    b, info = _call(g, H, F, mode, dev, R=ptr(dev["R"]), ldr=dev["R"].shape[1])
    assert info["rc_fwd"] == 0 and info["rc_bwd"] == 0, info["error"]
    L = lib()
    Y = dev["Y"]
    gy = _Guarded(N, (2 * HF // 64 + 1) * 64)
    ldg = gy.t.shape[1]
    gav = _Guarded(1, HF)
    wsz = L.mvml_gatv2_agg_bwd_workspace_size(N, E, H, F)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    for off in (0, HF - 4, ldg - HF + 4):
        rc = L.mvml_gatv2_agg_bwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
                                  ptr(g.out_inslot), E, ptr(Y), Y.shape[1], ctypes.c_void_p(Y.data_ptr() + 4 * HF),
                                  Y.shape[1], H, F, ptr(dev["av"]), ptr(b["attn"].t), ptr(b["out"].t),
                                  ptr(dev["g_out"]), SLOPE, mode, ptr(gy.t), ldg,
                                  ctypes.c_void_p(gy.t.data_ptr() + 4 * off), ldg, None, 0, ptr(gav.t), ptr(ws), wsz,
                                  stream_ptr())
        torch.cuda.synchronize()
        assert rc == MVML_ERR_INVALID and "gZL / gZR" in L.mvml_last_error().decode(), (off, L.mvml_last_error())
        assert bool((gy.whole == FILL).all()) and bool((gav.whole == FILL).all())


def test_empty_batch_returns_without_a_launch():
    L = lib()
    rp = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = torch.zeros(16, device=DEV)
    assert L.mvml_gatv2_agg_fwd(0, ptr(rp), None, ptr(x), 16, ptr(x), 16, 4, 4, ptr(x), None, 0, SLOPE, 2,
                                ptr(x), ptr(x), stream_ptr()) == 0
    assert L.mvml_gatv2_partial_rows(0) == 0 and L.mvml_gatv2_partial_rows(170) == 11
    assert L.mvml_gatv2_partial_rows(1 << 24) == 32768
