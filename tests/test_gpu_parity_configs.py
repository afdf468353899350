"""GPU parity at the BASELINE.json workload shapes: the HIP path (through the C ABI) against the
float64 oracle (oracle/gnn_ref.py) on seeded batches drawn from the SAME generators the bench
uses (mvml_gat.synth.config2 / config3 / config5), forward + backward, every parameter gradient.

Which aggregation kernels each case reaches (csrc/gat_agg_fwd.hip launch_fwd, gat_agg_bwd.hip
launch_bwd; H = 4, so both layers hold 3 float4 column slots per lane).  The Python layer picks the
path per batch (mvml_gat.functional: _fwd_path, flat_src); the tests below that name an option
switch it themselves, and so reach the other kernels:

* config 5 (150-400 atoms, 1-4 hubs of in-degree 32-128): every molecule is larger than the
  128-atom LDS window, a "large" batch: the forward by destination wave with the softmax in the
  wave (dst_fwd = 1), the backward by source atom:
    layer 0 (F = 192, flatten + ELU): gat_agg_fwd_dst_kernel<4, 0, 3, 1, SM, LR>,
                                      gat_flat_bwd_src1_kernel<4, 3, MODE, 1> (flat_src = 2)
    layer 1 (F = 384, mean):          gat_agg_fwd_dst_kernel<4, 1, 3, 1, SM, LR>,
                                      gat_mean_bwd_src_kernel<4, 2> (mean_src = 1)
  each source-atom backward followed by gat_mean_bwd_softmax_kernel<4> and
  gat_mean_bwd_gel_kernel<4>.  With dst_fwd = 0, big_window = 0 and mean_src = 0 the node-group
  plan sends ALL its groups to the fallbacks (gat_agg_fwd_gather_kernel<4, 32, {0,1}>,
  gat_agg_bwd_dst_kernel / gat_agg_bwd_src_kernel<4, 3> and <4, 6>); with big_window = 1 to the big
  windows (gat_agg_fwd_lds_kernel<4, 16, M, 512, 512, 2432, true> and the backward likewise).
* config 3 (KEGG-like 11-80 atoms, GraphNorm groups of 64 molecules, the bench shape): a "small"
  batch: gat_softmax_dst4_kernel, then gat_agg_fwd_dst_kernel<4, {0,1}, 3, 1, !SM> (dst_fwd = 2);
  layer 0's backward on the molecule window gat_agg_bwd_lds_kernel<4, 0, 32> (one or two passes
  per node group) with the per-atom pair for groups that hold an 80-atom molecule next to others
  (> 128 atoms), layer 1's by source atom.  With dst_fwd = 0: gat_agg_fwd_lds_kernel<4, 32,
  {0,1}, 512> and the gather kernel for such groups or an in-degree > 5 atom; with mean_src = 0:
  gat_agg_bwd_lds_kernel<4, 1, 32>.
* config 2 (25 atoms, 27 bonds): single GAT layers 0 and 1, the small-batch kernels.
* hub case at layer 0: flatten + ELU through the fallback kernels at the production width.

Bar (BASELINE.json north_star): outputs within 1e-5 norm-wise relative error of float64.
Gradients: 1e-5, or where the batch's own conditioning makes fp32 arithmetic lose a comparable
amount (measured as the error of the SAME oracle run in fp32 on the CPU, e32), 4 x e32.  The case
that needs it: GraphNorm's upstream gradient is mean-free over each group (column sums ~0.3 % of
column |sums| at config 3), so the Set2Set LSTM bias gradients are sums that cancel ~300-fold;
the CPU fp32 oracle loses 3.5-4e-6 there, the HIP path with split-bf16 GEMMs 1.0-1.07e-5 (3.1x),
with f32-input MFMA GEMMs 6e-6 (tools/diag_set2set_up.py).  Each case prints its worst margin.

LeakyReLU kink: at these sizes some edge has |el[src] + er[dst]| ~ 1e-8 (config 3, 192
molecules: 7e-8 at layer 1), so fp32 rounding decides which side of LeakyReLU's kink it is on,
and the two one-sided derivatives differ by 0.8 — a subgradient choice that moves d el / d er
(and through them attn_l / attn_r / dX) by up to 1e-2 relative, in ANY fp32 implementation.  The
oracle is therefore evaluated on the product's side of the kink for every edge
(oracle.gnn_ref.leaky_relu_branch, sides from the product's own fp32 el + er); the forward
values still equal leaky_relu wherever the sides agree, and the test asserts that the sides
disagree with float64 only on edges within 1e-6 of the kink.
"""
import numpy as np
import pytest
import torch

from _util import batch_of_sizes, graph_dict, model_pair
from conftest import rel_err
from mvml_gat import functional as Fn
from mvml_gat import synth
from mvml_gat._lib import option
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _capture(fn):
    """Run fn() with the product's el / er capture on; return (result, [elr per GAT layer])."""
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        res = fn()
    finally:
        Fn.DEBUG_CAPTURE = None
    return res, [e.cpu() for e in cap.get("elr_fwd", [])]


def _branches(gd, elrs, H=4):
    """The product's LeakyReLU side per (edge, head), original edge order: the kernels' fp32
    test (el[src] + er[dst]) > 0 on its own el / er."""
    src = torch.as_tensor(np.asarray(gd["src"]), dtype=torch.long)
    dst = torch.as_tensor(np.asarray(gd["dst"]), dtype=torch.long)
    return [(e[:, :H][src] + e[:, H:][dst]) > 0 for e in elrs]


def _check_kink_flips(gd, branches, layer_inputs64, layer_params64, H=4):
    """Sides that disagree with float64 must be within 1e-6 (relative to max |el|) of the kink."""
    src = torch.as_tensor(np.asarray(gd["src"]), dtype=torch.long)
    dst = torch.as_tensor(np.asarray(gd["dst"]), dtype=torch.long)
    flips = 0
    for br, Xl, p in zip(branches, layer_inputs64, layer_params64):
        with torch.no_grad():
            Z = (Xl @ p["fc.weight"].t()).view(Xl.shape[0], H, -1)
            el, er = (Z * p["attn_l"]).sum(-1), (Z * p["attn_r"]).sum(-1)
            s = el[src] + er[dst]
        bad = br != (s > 0)
        flips += int(bad.sum())
        if bad.any():
            scale = max(el.abs().max().item(), er.abs().max().item())
            assert s[bad].abs().max().item() <= 1e-6 * scale, s[bad]
    assert flips <= max(2, s.numel() // 10000), flips
    return flips


def _module_case(sb, group_size=None, seed=3, hidden_feats=(192, 384)):
    hidden = list(hidden_feats)
    prod, ref = model_pair(hidden=hidden, seed=seed)
    prod.eval()
    ref.eval()
    ref32 = type(ref)(74, hidden, 0.5, 6, 3).eval()
    ref32.load_state_dict(ref.state_dict())
    ref64 = ref.double()
    gd = graph_dict(sb, group_size=group_size)
    X = torch.as_tensor(sb.feats, dtype=torch.float64)

    prod = prod.to(DEV)
    g = sb.to_graph(group_size=group_size).to(DEV)
    out_p, elrs = _capture(lambda: prod(g, g.ndata["h"]))
    br = _branches(gd, elrs)
    out_r = ref64(gd, X, branches=br)
    gout = torch.randn(out_r.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    out_r.backward(gout)
    out_32 = ref32(gd, X.float(), branches=br)
    out_32.backward(gout.float())
    out_p.backward(gout.float().to(DEV))
    torch.cuda.synchronize()
    with torch.no_grad():
        lp = ref64.layer_params()
        h1 = gnn_ref.gat_layer_ref(gd["src"], gd["dst"], X, lp[0], 4, hidden[0], "flatten",
                                   torch.nn.functional.elu)
    flips = _check_kink_flips(gd, br, [X, h1], lp)

    margins = {}
    e = rel_err(out_p, out_r)
    margins["out"] = (e, TOL)
    p64 = dict(ref64.named_parameters())
    p32 = dict(ref32.named_parameters())
    for n, p in prod.named_parameters():
        e = rel_err(p.grad, p64[n].grad)
        budget = max(TOL, 4 * rel_err(p32[n].grad, p64[n].grad))
        margins[n] = (e, budget)
    worst = max(margins.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"worst err/budget {worst[0]}: {worst[1][0]:.2e} / {worst[1][1]:.2e} = "
          f"{worst[1][0] / worst[1][1]:.3f}; "
          f"{flips} LeakyReLU sides differ from float64 (all at the kink)")
    for n, (e, b) in margins.items():
        assert e < b, (n, e, b)


def test_gnn_module_config5_hub_molecules():
    """BASELINE config 5 molecules (all layer-0 and layer-1 fallback kernels, every group)."""
    sb = synth.config5(3, seed=1)
    assert sb.num_nodes.min() > 128
    _module_case(sb, seed=5)


def test_gnn_module_config5_four():
    sb = synth.config5(4, seed=7)
    _module_case(sb, seed=6)


def test_gnn_module_config3_graphnorm_groups():
    """The bench shape: KEGG-like sizes, three GraphNorm groups of 64 molecules."""
    sb = synth.config3(192, seed=11)
    _module_case(sb, group_size=64, seed=7)


def test_gnn_module_other_widths():
    """GNNModule(74, [20, 260]): the flatten layer on the CW 4 windows, the head-mean layer and
    Set2Set at a width with a partly masked last slot (260 = 256 + 4), GraphNorm / fc at 520."""
    _module_case(batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1), seed=4, hidden_feats=(20, 260))


def _layer_case(layer, sb, seed=0, x_grad=True, shape=None):
    """One GAT layer, forward and every gradient, against float64.  layer 0 / 1: the layer of
    GNNModule's default stack (Fin = 74, H = 4, F = 192, flatten + ELU / Fin = 768, F = 384, head
    mean), bar 1e-5 on everything.  shape = (Fin, H, F, agg_mode): a mvml_gat.nn.GATLayer of that
    shape built directly (flatten + ELU, or mean without activation); bar 1e-5, or 4 x the error
    of the same oracle run in fp32 on the CPU where that is larger; prints and returns the worst
    err / budget.  x_grad=False: layer 0 as GNNModule runs it, on the atom features (no input
    gradient)."""
    n = int(sb.num_nodes.sum())
    g = torch.Generator().manual_seed(seed)
    if shape is None:
        prod, ref = model_pair(seed=seed)
        conv_p = prod.conv.gnn_layers[layer]
        conv_r = ref.conv.gnn_layers[layer].gat_conv
        Fin, H, Fo = (74, 4, 192) if layer == 0 else (768, 4, 384)
        mode = "flatten" if layer == 0 else "mean"
    else:
        from mvml_gat.nn import GATLayer
        from _util import randomize_
        Fin, H, Fo, mode = shape
        torch.manual_seed(seed)
        conv_p = GATLayer(Fin, Fo, H, agg_mode=mode,
                          activation=torch.nn.functional.elu if mode == "flatten" else None)
        randomize_(conv_p, seed)
        conv_r = conv_p.gat_conv
    act = torch.nn.functional.elu if mode == "flatten" else None
    if Fin == 74:
        X = torch.as_tensor(sb.feats, dtype=torch.float64)
    else:
        X = torch.randn(n, Fin, generator=g, dtype=torch.float64)
    gd = graph_dict(sb)
    params = {"fc.weight": conv_r.fc.weight, "res_fc.weight": conv_r.res_fc.weight,
              "attn_l": conv_r.attn_l, "attn_r": conv_r.attn_r, "bias": conv_r.bias}
    p64 = {k: v.detach().double().requires_grad_() for k, v in params.items()}
    p32 = {k: v.detach().cpu().clone().requires_grad_() for k, v in params.items()}
    conv_p = conv_p.to(DEV)
    gdev = sb.to_graph().to(DEV)
    Xp = X.float().to(DEV).requires_grad_(x_grad)
    out_p, elrs = _capture(lambda: conv_p(gdev, Xp))
    br = _branches(gd, elrs, H)
    _check_kink_flips(gd, br, [X], [p64], H)
    Xr = X.clone().requires_grad_()
    out_r = gnn_ref.gat_layer_ref(gd["src"], gd["dst"], Xr, p64, H, Fo, mode, act, branch=br[0])
    gout = torch.randn(out_r.shape, generator=g, dtype=torch.float64)
    out_r.backward(gout)
    out_p.backward(gout.float().to(DEV))
    c = conv_p.gat_conv
    got = {"forward": (out_p, out_r)}
    if x_grad:
        got["dX"] = (Xp.grad, Xr.grad)
    for name, pp in (("fc.weight", c.fc.weight), ("res_fc.weight", c.res_fc.weight),
                     ("attn_l", c.attn_l), ("attn_r", c.attn_r), ("bias", c.bias)):
        got[name] = (pp.grad, p64[name].grad)
    budget = {k: TOL for k in got}
    if shape is not None:
        X32 = X.float().requires_grad_()
        gnn_ref.gat_layer_ref(gd["src"], gd["dst"], X32, p32, H, Fo, mode, act, branch=br[0]).backward(gout.float())
        for k in got:
            if k not in ("forward", "dX"):
                budget[k] = max(TOL, 4 * rel_err(p32[k].grad, p64[k].grad))
        if x_grad:
            budget["dX"] = max(TOL, 4 * rel_err(X32.grad, Xr.grad))
    errs = {k: rel_err(a, b) for k, (a, b) in got.items()}
    worst = max(errs, key=lambda k: errs[k] / budget[k])
    if shape is not None:
        print(f"LAYER {shape} worst err/budget {worst}: {errs[worst]:.2e} / {budget[worst]:.2e} = "
              f"{errs[worst] / budget[worst]:.3f}")
    for k in got:
        assert errs[k] < budget[k], (k, errs[k], budget[k])
    return errs[worst] / budget[worst]


_SHAPE_GRAPHS = {"mixed": lambda: batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1),
                 "hubs": lambda: batch_of_sizes([150, 90], seed=7, hubs=True)}
LAYER_SHAPES = [(74, 1, 4, "flatten"), (74, 2, 12, "flatten"), (74, 8, 8, "flatten"), (30, 4, 72, "flatten"),
                (100, 8, 256, "flatten"), (74, 2, 24, "mean"), (80, 4, 132, "mean"), (64, 8, 64, "mean"),
                (768, 1, 260, "mean"), (288, 4, 388, "mean"),
                # past the destination-wave forward's slots: the window kernels on the default policy
                (96, 2, 1024, "mean")]


@pytest.mark.parametrize("graph", list(_SHAPE_GRAPHS))
@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: f"Fin{s[0]}-H{s[1]}-F{s[2]}-{s[3]}")
def test_gat_layer_other_heads_and_widths(shape, graph):
    """mvml_gat.nn.GATLayer at head counts 1 / 2 / 8 and widths off the defaults, on the default
    kernel policy: mvml_gat_fold_weights / mvml_gat_unfold_grads with the head-mean residual at
    H != 4, the attention-vector gradient, the small-K projection at other column counts and
    Fin % 4 != 0 — forward and every gradient against float64."""
    _layer_case(None, _SHAPE_GRAPHS[graph](), seed=3, shape=shape)


@pytest.mark.parametrize("layer", [0, 1])
def test_gat_layer_config2(layer):
    """BASELINE config 2 molecules (25 atoms, 27 bonds), one GAT layer of each kind."""
    _layer_case(layer, synth.config2(128, seed=0), seed=layer)


@pytest.mark.parametrize("case", ["config2", "config5", "hubs", "table_overflow", "config3"])
def test_gat_layer0_flat_src(case):
    """Option flat_src = 1: the flatten layer's aggregation backward by source atom in one pass
    (gat_flat_bwd_src1_kernel forms each gathered g_rst row in registers) — forward and every
    gradient against float64 on each graph family."""
    sb = {"config2": lambda: synth.config2(128, seed=0),
          "config5": lambda: synth.config5(2, seed=3),
          "hubs": lambda: batch_of_sizes([150, 90, 210], seed=7, hubs=True),
          "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109),
          "config3": lambda: synth.config3(192, seed=4)}[case]()
    with option("flat_src", 1):
        _layer_case(0, sb, seed=8)


_FAMILIES = {"config2": lambda: synth.config2(128, seed=0),
             "config5": lambda: synth.config5(2, seed=3),
             "hubs": lambda: batch_of_sizes([150, 90, 210], seed=7, hubs=True),
             "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109),
             "config3": lambda: synth.config3(192, seed=4)}


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("case", list(_FAMILIES))
@pytest.mark.parametrize("layer", [0, 1])
def test_gat_layer_dst_fwd(case, layer, kind, monkeypatch):
    """The aggregation forward by destination wave (csrc/gat_agg.hip gat_agg_fwd_dst_kernel),
    FORCED to each kind through the layer (GATLayerFunction picks the kind per call from the
    batch, functional._fwd_path, so the option alone is overridden): kind 1 fuses the edge
    softmax, kind 2 runs it first as its own launch (gat_softmax_dst4_kernel).  With, for the
    flatten layer, the one-pass source-atom backward (flat_src = 2): forward and every gradient
    against float64 on each graph family (hubs of in-degree past 64: the softmax's multi-chunk
    path and the logit recomputation past the cached in-edges)."""
    monkeypatch.setattr(Fn, "DST_FWD_POLICY", "all")
    monkeypatch.setattr(Fn, "DST_FWD_KIND", kind)
    sb = _FAMILIES[case]()
    with option("flat_src", 2 if layer == 0 else 0):
        _layer_case(layer, sb, seed=8 + layer)


def _agg_outputs(sb, H, F, mode, seed=0, inputs=None, fill=None, graph=None, full=False):
    """One aggregation forward + backward through the C ABI on seeded projection rows:
    (out, attn, gY[:, :C + 2H], out_amax, out_row_amax, gy_amax, gy_row_amax).

    inputs: dict with device tensors "Y" ([N, ldy], ldy >= C a multiple of 4), "elr" [N, 2H],
    "bias" [H F] and "g_out", used instead of the seeded ones.  fill: value written into out, attn
    and ALL of gY before the calls (default: out / attn uninitialised, gY zeros).  graph: sb's
    device graph, built once by the caller.  full=True appends a dict with the inputs used, the
    whole gY (pad columns included) and the two status codes, and returns instead of raising when
    an entry point refuses the call (status != 0: the later call is not made)."""
    from mvml_gat._lib import call, lib, ptr, stream_ptr
    L = lib()
    g = graph if graph is not None else sb.to_graph().to(DEV)
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator(device=DEV).manual_seed(seed)
    C = L.mvml_gat_proj_cols(H, F, int(mode == 1))
    oc = F if mode == 1 else H * F
    if inputs is None:
        ldy = (C + 63) // 64 * 64
        Y = torch.randn((N, ldy), device=DEV, generator=gen) * 0.3
        elr = torch.randn((N, 2 * H), device=DEV, generator=gen)
        bias = torch.randn(H * F, device=DEV, generator=gen) * 0.1
    else:
        Y, elr, bias = inputs["Y"], inputs["elr"], inputs["bias"]
        ldy = Y.shape[1]
    out = torch.empty((N, oc), device=DEV)
    attn = torch.empty((E, H), device=DEV)
    if fill is not None:
        out.fill_(fill)
        attn.fill_(fill)
    st = stream_ptr()
    orow = torch.zeros(N, dtype=torch.int32, device=DEV)
    omx = torch.zeros(1, dtype=torch.int32, device=DEV)
    fwd_args = ("mvml_gat_agg_fwd", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                ptr(Y), ldy, H, F, ptr(elr), ptr(bias), 0.2, mode, ptr(out), ptr(attn), ptr(omx), ptr(orow), st)
    g_out = torch.randn((N, oc), device=DEV, generator=gen) if inputs is None else inputs["g_out"]
    ldg = (C + 2 * H + 63) // 64 * 64
    gY = torch.zeros((N, ldg), device=DEV) if fill is None else torch.full((N, ldg), fill, device=DEV)
    wsz = L.mvml_gat_agg_bwd_workspace_size(E, H)
    ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device=DEV)
    gmx = torch.zeros(1, dtype=torch.int32, device=DEV)
    grow = torch.zeros(N, dtype=torch.int32, device=DEV)
    bwd_args = ("mvml_gat_agg_bwd", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), ldy, ptr(elr), ptr(attn), ptr(out),
                ptr(g_out), H, F, 0.2, mode, ptr(gY), ldg, ptr(gmx), ptr(grow), ptr(ws), wsz, st)
    res = (out, attn, gY[:, :C + 2 * H], omx, orow, gmx, grow)
    if not full:
        call(*fwd_args)
        call(*bwd_args)
        torch.cuda.synchronize()
        return res
    rc_f = getattr(L, fwd_args[0])(*fwd_args[1:])
    err = L.mvml_last_error().decode(errors="replace") if rc_f else ""
    rc_b = None
    if rc_f == 0:
        rc_b = getattr(L, bwd_args[0])(*bwd_args[1:])
        err = L.mvml_last_error().decode(errors="replace") if rc_b else ""
    torch.cuda.synchronize()
    return res + ({"Y": Y, "elr": elr, "bias": bias, "g_out": g_out, "gY": gY, "C": C,
                   "rc_fwd": rc_f, "rc_bwd": rc_b, "error": err},)


@pytest.mark.parametrize("case", ["config2", "config3"])
@pytest.mark.parametrize("mode", [0, 1])
def test_dst_fwd_bitwise_molecule_windows(case, mode):
    """Without hubs, the destination-wave forward sums every row in edge order from 0 exactly as
    the molecule-window / gather kernels do, with the same softmax arithmetic: out, attn and the
    output maxima are BITWISE equal."""
    sb = _FAMILIES[case]()
    F = 192 if mode == 0 else 384
    with option("dst_fwd", 0):
        a = _agg_outputs(sb, 4, F, mode)
    for kind in (1, 2):  # softmax fused / softmax as its own launch first
        with option("dst_fwd", kind):
            b = _agg_outputs(sb, 4, F, mode)
        for i in (0, 1, 3, 4):
            assert torch.equal(a[i], b[i]), (kind, i, (a[i].double() - b[i].double()).abs().max().item())


@pytest.mark.parametrize("case", ["hubs", "table_overflow", "config5"])
@pytest.mark.parametrize("mode", [0, 1])
def test_dst_fwd_kinds_bitwise_hubs(case, mode):
    """On hub molecules (in-degrees past the 6 cached in-edges and past 64: the softmax kernel's
    logit recomputation and the gather kernel's SM = false path over long rows) the two
    destination-wave kinds give BITWISE the same out, attn and output maxima: the softmax as its
    own launch (kind 2) follows the fused softmax's (kind 1) arithmetic and edge order."""
    sb = _FAMILIES[case]()
    F = 192 if mode == 0 else 384
    with option("dst_fwd", 1):
        a = _agg_outputs(sb, 4, F, mode)
    with option("dst_fwd", 2):
        b = _agg_outputs(sb, 4, F, mode)
    for i in (0, 1, 3, 4):
        assert torch.equal(a[i], b[i]), (i, (a[i].double() - b[i].double()).abs().max().item())


@pytest.mark.parametrize("flat_src", [0, 2])
@pytest.mark.parametrize("case", ["config2", "config5"])
def test_gat_bwd_gy_row_maxima_flat(case, flat_src):
    """Per-row max |gY| of the flatten layer's backward, both paths (see the layer-1 test)."""
    if Fn.GEMM_ALGO != "f16x2" or not Fn.ROW_SCALES:
        pytest.skip("per-row maxima feed the per-row split-fp16 GEMM only")
    sb = {"config2": lambda: synth.config2(64, seed=0), "config5": lambda: synth.config5(2, seed=3)}[case]()
    prev = Fn.FLAT_SRC_AUTO
    Fn.FLAT_SRC_AUTO = False
    try:
        with option("flat_src", flat_src):
            cap = _gy_max_case(0, sb)
    finally:
        Fn.FLAT_SRC_AUTO = prev
    (gY, _), = cap["gy_amax"]
    rows, = cap["gy_rows"]
    want = gY.abs().max(dim=1).values
    got = rows.view(torch.float32)[:gY.shape[0]]
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("case", ["config2", "config3"])
def test_gat_layer1_molecule_window_backward(case):
    """Option mean_src = 0: the head-mean layer's backward on the molecule-window LDS kernel (the
    default path is the source-atom kernel, tested by every other layer-1 case)."""
    sb = {"config2": lambda: synth.config2(128, seed=0), "config3": lambda: synth.config3(192, seed=4)}[case]()
    with option("mean_src", 0):
        _layer_case(1, sb, seed=7)


def test_gat_layer0_hubs_flatten_elu(monkeypatch):
    """Layer 0 (F = 192, flatten + ELU) on hub molecules > 128 atoms: the big-window kernels
    (kind bit 2) with their hub segments, at the production width (the source-atom backward
    that such batches take by default turned off; it has its own cases)."""
    monkeypatch.setattr(Fn, "FLAT_SRC_AUTO", False)
    _layer_case(0, batch_of_sizes([150, 90, 210], seed=7, hubs=True), seed=2)


@pytest.mark.parametrize("case", ["config2", "hubs", "config5", "config5_three", "table_overflow",
                                  "config3"])
def test_gat_layer0_no_input_grad(case):
    """The first layer as GNNModule runs it (no input gradient: the dX product is skipped) —
    every output and gradient against float64 on each graph family."""
    sb = {"config2": lambda: synth.config2(128, seed=0),
          "hubs": lambda: batch_of_sizes([150, 90, 210], seed=7, hubs=True),
          "config5": lambda: synth.config5(2, seed=3),
          "config5_three": lambda: synth.config5(3, seed=5),
          "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109),
          "config3": lambda: synth.config3(192, seed=4)}[case]()
    _layer_case(0, sb, seed=11, x_grad=False)


@pytest.mark.parametrize("mean_src", [1, 0])
def test_gat_layer1_config5(mean_src):
    """The head-mean layer on config 5: backward by source atom (default) and by big windows."""
    with option("mean_src", mean_src):
        _layer_case(1, synth.config5(2, seed=3), seed=4)


@pytest.mark.parametrize("layer", [0, 1])
def test_gat_layer_config5_fallback_kernels(layer, monkeypatch):
    """Option big_window = 0: config-5 groups through the per-atom fallbacks (forward gather
    with its hub pass, dst / src backward pair) — the path of groups past the big window's caps
    (the head-mean layer's source-atom backward, picked for such batches, turned off)."""
    monkeypatch.setattr(Fn, "FLAT_SRC_AUTO", False)
    with option("big_window", 0), option("mean_src", 0):
        _layer_case(layer, synth.config5(2, seed=3), seed=4 + layer)


@pytest.mark.parametrize("layer", [0, 1])
def test_gat_layer_big_window_table_overflow(layer, monkeypatch):
    """A 300-atom molecule with 7 hubs of 109 partners (2428 edges, at the big window's edge
    cap): the backward's staged out-edges (640) and out-edge segments (48) overflow, so the
    last hubs walk their out-edges from global memory on their own lanes."""
    sb = batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109)
    assert int(sb.num_edges[0]) <= 2432
    monkeypatch.setattr(Fn, "FLAT_SRC_AUTO", False)
    with option("mean_src", 0):  # the big-window backward itself
        _layer_case(layer, sb, seed=5 + layer)


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("case", ["config2", "config5_big", "config5_fallback", "table_overflow",
                                  "atomwise"])
def test_gat_bwd_fused_gy_max(layer, case, monkeypatch):
    """mvml_gat_agg_bwd folds max |gY| (the split-fp16 scale of the dL/dW and dL/dX GEMMs) into
    its stores: it must equal the max over every column the GEMMs read, [dZ | dR | d el | d er],
    on every kernel path that writes gY (LDS windows, big windows, the dst / src fallback pair
    with and without node groups)."""
    if Fn.GEMM_ALGO != "f16x2":
        pytest.skip("the fused max feeds the split-fp16 GEMMs only")
    sb = {"config2": lambda: synth.config2(64, seed=0),
          "config5_big": lambda: synth.config5(2, seed=3),
          "config5_fallback": lambda: synth.config5(2, seed=3),
          "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109),
          "atomwise": lambda: synth.config3(128, seed=2)}[case]()
    opts = {"config5_fallback": ("big_window", 0), "atomwise": ("bwd_atomwise", 1)}
    monkeypatch.setattr(Fn, "FLAT_SRC_AUTO", False)
    with option(*opts.get(case, ("big_window", 1))), option("mean_src", 0):  # the named path
        _gy_max_case(layer, sb)


@pytest.mark.parametrize("case", ["config2", "config5", "hubs", "table_overflow", "config3"])
def test_gat_layer1_mean_src(case):
    """Option mean_src = 1: the head-mean layer's aggregation backward by SOURCE atom
    (gat_mean_bwd_src_kernel: one wave per atom reads its projection row once and gathers the
    F-wide g_out rows of its out-edges; softmax / d el passes per atom) — forward and every
    gradient against float64 on each graph family, hubs and the 2,428-edge molecule included."""
    sb = {"config2": lambda: synth.config2(128, seed=0),
          "config5": lambda: synth.config5(2, seed=3),
          "hubs": lambda: batch_of_sizes([150, 90, 210], seed=7, hubs=True),
          "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109),
          "config3": lambda: synth.config3(192, seed=4)}[case]()
    with option("mean_src", 1):
        _layer_case(1, sb, seed=6)


@pytest.mark.parametrize("mean_src", [0, 1])
@pytest.mark.parametrize("case", ["config2", "config5"])
def test_gat_bwd_gy_row_maxima(case, mean_src):
    """The per-row max |gY| the aggregation backward folds into its stores (the dL/dX GEMM's
    per-row split-fp16 scales) equals each row's max over [dZ | dR | d el | d er]."""
    if Fn.GEMM_ALGO != "f16x2" or not Fn.ROW_SCALES:
        pytest.skip("per-row maxima feed the per-row split-fp16 GEMM only")
    sb = {"config2": lambda: synth.config2(64, seed=0), "config5": lambda: synth.config5(2, seed=3)}[case]()
    with option("mean_src", mean_src):
        cap = _gy_max_case(1, sb)
    (gY, _), = cap["gy_amax"]
    rows, = cap["gy_rows"]
    want = gY.abs().max(dim=1).values
    got = rows.view(torch.float32)[:gY.shape[0]]
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("case", ["config2", "config5", "table_overflow"])
def test_gat_bwd_fused_gy_max_mean_src(case):
    sb = {"config2": lambda: synth.config2(64, seed=0), "config5": lambda: synth.config5(2, seed=3),
          "table_overflow": lambda: batch_of_sizes([300, 40], seed=9, hubs=True, n_hubs=7, partners=109)}[case]()
    if Fn.GEMM_ALGO != "f16x2":
        pytest.skip("the fused max feeds the split-fp16 GEMMs only")
    with option("mean_src", 1):
        _gy_max_case(1, sb)


def _gy_max_case(layer, sb):
    prod, _ = model_pair(seed=layer)
    conv = prod.conv.gnn_layers[layer].to(DEV)
    g = sb.to_graph().to(DEV)
    n = int(sb.num_nodes.sum())
    X = (torch.as_tensor(sb.feats, dtype=torch.float32) if layer == 0
         else torch.randn(n, 768, generator=torch.Generator().manual_seed(1))).to(DEV).requires_grad_()
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        out = conv(g, X)
        out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).to(DEV))
        torch.cuda.synchronize()
    finally:
        Fn.DEBUG_CAPTURE = None
    (gY, amx), = cap["gy_amax"]
    want = gY.abs().max().item()
    got = amx.cpu().view(torch.float32).item()
    assert got == want and want > 0, (got, want)
    # and max |out| folded into the forward aggregation's stores (the next GEMMs' operand max)
    t, i = out._mvml_amax[:2]
    got_o = t[i:i + 1].cpu().view(torch.float32).item()
    assert got_o == out.detach().abs().max().item(), (got_o, out.detach().abs().max().item())
    return cap
