"""mvml_gat_layer_bwd: a GATConv's whole backward as ONE C call, called
through the ctypes handle of libmvml_gat.so with the forward's saved tensors, is BITWISE the
gradient the Python layer (GATLayerFunction.backward: the same launches) gives — for the
flatten + ELU layer on the 74 atom features and the head-mean layer on 768-wide rows, and for
one layer of each kind at other head counts (H = 8 and H = 1 flatten, H = 2 and H = 1 head mean).
With g_X == NULL (a first layer: the per-row maxima of gY, Wcat's interleaved image and the
data-gradient product are not formed) the other five gradients are bitwise those of the call with
g_X, and nothing is written where g_X would be."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import contextlib

from mvml_gat import functional as Fn
from mvml_gat import synth
from mvml_gat._lib import lib, option, ptr, stream_ptr
from mvml_gat.nn import GATLayer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# layer 0 / 1: GNNModule's default layers; the others: head counts off the default, one of each kind
LAYERS = {0: (74, 4, 192, 0), 1: (768, 4, 384, 1), "flatten-H8-F8": (74, 8, 8, 0), "mean-H2-F24": (74, 2, 24, 1),
          "flatten-H1-F24": (74, 1, 24, 0), "mean-H1-F24": (74, 1, 24, 1)}
POISON_BITS = 0x7FC5A5A5   # (_gemm_cases.POISON_BITS)


def _run(layer, case, with_gx=True):
    """The Python layer's backward and the one C call on the same saved tensors: (module, X, the
    call's outputs by name, the poisoned arena they are views of)."""
    sb = synth.config2(96, seed=3) if case == "config2" else synth.config5(2, seed=4)
    g = sb.to_graph().to(DEV)
    N, E = g.num_nodes(), g.num_edges()
    torch.manual_seed(layer if isinstance(layer, int) else 2)
    Fin, H, Fo, mean = LAYERS[layer]
    layer = mean  # (below: 0 = flatten + ELU, 1 = head mean)
    if layer == 0:
        m = GATLayer(Fin, Fo, H, agg_mode="flatten", activation=F.elu).to(DEV)
    else:
        m = GATLayer(Fin, Fo, H, agg_mode="mean").to(DEV)
    if Fin == 74:
        X = torch.as_tensor(sb.feats, dtype=torch.float32, device=DEV)
    else:
        X = torch.randn(N, Fin, device=DEV)
    X = X.clone().requires_grad_()
    out = m(g, X)
    Xp, Wcat, Y, attn, elr, outs, attn_l, attn_r, attn_lr = out.grad_fn.saved_tensors
    gout = torch.randn(out.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    out.backward(gout)
    torch.cuda.synchronize()

    L = lib()
    HF = H * Fo
    wsz = L.mvml_gat_layer_bwd_workspace_size(N, E, H, Fo, Fin, layer)
    ws = torch.empty(max(wsz, 256), dtype=torch.uint8, device=DEV)
    # every output inside one poisoned arena, 64 floats of poison between them
    sizes = {"g_X": N * Fin, "g_fc": HF * Fin, "g_res": HF * Fin, "g_attn": 2 * HF, "g_bias": HF}
    shapes = {"g_X": (N, Fin), "g_fc": (HF, Fin), "g_res": (HF, Fin), "g_attn": (2, HF), "g_bias": (HF,)}
    arena = torch.full((sum(-(-n // 64) * 64 + 64 for n in sizes.values()) + 64,), POISON_BITS, dtype=torch.int32,
                       device=DEV).view(torch.float32)
    o, off = {}, 64
    for k, n in sizes.items():
        o[k] = arena[off:off + n].view(shapes[k])
        off += -(-n // 64) * 64 + 64
    # the aggregation backward's kernel choice is a process option (mvml_set_option), as for
    # mvml_gat_agg_bwd: set it the way the Python layer did for this batch
    flat_src = Fn.FLAT_SRC_AUTO and layer == 0 and Fn._large_batch(g)
    with option("flat_src", 2) if flat_src else contextlib.nullcontext():
        rc = L.mvml_gat_layer_bwd(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                  ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), E, H, Fo, Fin, layer,
                                  ctypes.c_float(0.2), ptr(Xp), ptr(Wcat), ptr(attn_lr), ptr(Y), Y.stride(0),
                                  ptr(elr), ptr(attn), ptr(outs), ptr(gout.contiguous()),
                                  ptr(o["g_X"]) if with_gx else None, ptr(o["g_fc"]),
                                  ptr(o["g_res"]), ptr(o["g_attn"]), ptr(o["g_bias"]), ptr(ws), ws.numel(), stream_ptr())
    assert rc == 0, L.mvml_last_error().decode()
    torch.cuda.synchronize()
    return m, X, o, arena


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("case", ["config2", "config5"])
def test_gat_layer_bwd_one_call_bitwise(layer, case):
    m, X, o, arena = _run(layer, case)
    conv = m.gat_conv
    assert torch.equal(o["g_X"], X.grad)
    assert torch.equal(o["g_fc"], conv.fc.weight.grad)
    assert torch.equal(o["g_res"], conv.res_fc.weight.grad)
    assert torch.equal(o["g_attn"][0], conv.attn_l.grad.reshape(-1))
    assert torch.equal(o["g_attn"][1], conv.attn_r.grad.reshape(-1))
    assert torch.equal(o["g_bias"], conv.bias.grad)
    written = torch.zeros(arena.numel(), dtype=torch.bool, device=DEV)
    for t in o.values():
        start = (t.data_ptr() - arena.data_ptr()) // 4
        written[start:start + t.numel()] = True
    assert bool((arena.view(torch.int32)[~written] == POISON_BITS).all()), "written outside an output"


@pytest.mark.parametrize("layer", ["flatten-H8-F8", "mean-H2-F24", "flatten-H1-F24", "mean-H1-F24"])
def test_gat_layer_bwd_without_g_x(layer):
    """g_X == NULL: the first layer's branch.  The parameter gradients are bitwise those of the call
    that also forms g_X (and so the Python backward's), and g_X's place stays poison."""
    m, X, o, arena = _run(layer, "config2", with_gx=False)
    _, _, full, _ = _run(layer, "config2")
    for k in ("g_fc", "g_res", "g_attn", "g_bias"):
        assert torch.equal(o[k].view(torch.int32), full[k].view(torch.int32)), k
    conv = m.gat_conv
    assert torch.equal(o["g_fc"], conv.fc.weight.grad) and torch.equal(o["g_res"], conv.res_fc.weight.grad)
    assert torch.equal(o["g_attn"][0], conv.attn_l.grad.reshape(-1)) and torch.equal(o["g_bias"], conv.bias.grad)
    assert bool((o["g_X"].view(torch.int32) == POISON_BITS).all()), "g_X's place written with g_X == NULL"
    assert bool(torch.isfinite(full["g_X"]).all())


def test_gat_layer_bwd_workspace_checked():
    """A workspace below mvml_gat_layer_bwd_workspace_size is refused (no device work)."""
    L = lib()
    need = L.mvml_gat_layer_bwd_workspace_size(100, 300, 4, 192, 74, 0)
    assert need > 0
    z = torch.zeros(1, device=DEV)
    rc = L.mvml_gat_layer_bwd(100, ptr(z), 1, ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), 300, 4, 192, 74, 0,
                              ctypes.c_float(0.2), ptr(z), ptr(z), ptr(z), ptr(z), 1600, ptr(z), ptr(z), ptr(z),
                              ptr(z), None, ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), need - 1, stream_ptr())
    assert rc == 3, rc
    assert b"workspace too small" in L.mvml_last_error()
