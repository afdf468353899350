"""oracle.gnn_ref.gat_agg_ref (the float64 reference of mvml_gat_agg_fwd / _bwd at the ABI's own
cut: Z, R and [el | er] given) against gat_layer_ref (the whole GATConv from X), in float64 on the
CPU: the two must be the same function, so the GPU tests that compare the aggregation kernels with
gat_agg_ref compare them with the GATConv the rest of the suite is pinned to."""
import pytest
import torch

from _util import batch_of_sizes, graph_dict
from conftest import rel_err
from oracle import gnn_ref

SIZES = [25, 1, 40, 7, 23, 3, 64, 2, 5]


@pytest.mark.parametrize("kind", ["flatten_elu", "flatten", "mean"])
@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_gat_agg_ref_equals_gat_layer_ref(H, kind):
    F, Fin = 12, 30
    sb = batch_of_sizes(SIZES, seed=H)
    gd = graph_dict(sb)
    n = int(sb.num_nodes.sum())
    g = torch.Generator().manual_seed(10 * H + len(kind))

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).requires_grad_()

    p = {"fc.weight": leaf(H * F, Fin, scale=0.3), "res_fc.weight": leaf(H * F, Fin, scale=0.3),
         "attn_l": leaf(1, H, F), "attn_r": leaf(1, H, F), "bias": leaf(H * F, scale=0.1)}
    X = leaf(n, Fin)
    mode = {"flatten_elu": 0, "mean": 1, "flatten": 2}[kind]
    agg_mode = "mean" if mode == 1 else "flatten"
    act = torch.nn.functional.elu if mode == 0 else None
    want = gnn_ref.gat_layer_ref(gd["src"], gd["dst"], X, p, H, F, agg_mode, act)
    gout = torch.randn(want.shape, generator=g, dtype=torch.float64)
    want.backward(gout)
    grads = {k: v.grad.clone() for k, v in p.items()}
    gX = X.grad.clone()
    for t in (X, *p.values()):
        t.grad = None

    # the projection as the product forms it (mvml_gat_fold_weights / mvml_gat_proj_fwd), float64
    Z = (X @ p["fc.weight"].t()).view(n, H, F)
    Wr = p["res_fc.weight"].view(H, F, Fin).mean(0) if mode == 1 else p["res_fc.weight"]
    R = X @ Wr.t()
    elr = torch.cat([(Z * p["attn_l"]).sum(-1), (Z * p["attn_r"]).sum(-1)], 1)
    got, attn = gnn_ref.gat_agg_ref(gd["src"], gd["dst"], Z, R, elr, p["bias"], H, F, mode, 0.2, None)
    got.backward(gout)

    assert rel_err(got, want) < 1e-12
    assert rel_err(X.grad, gX) < 1e-12
    for k, v in p.items():
        assert rel_err(v.grad, grads[k]) < 1e-12, k

    # attn: in-CSR slot order = the edges stably sorted by dst; each destination's slots sum to 1
    dst = torch.as_tensor(gd["dst"], dtype=torch.long)
    _, a = gnn_ref.gatconv_ref(gd["src"], gd["dst"], X, p["fc.weight"], p["res_fc.weight"], p["attn_l"],
                               p["attn_r"], p["bias"], H, F, return_attention=True)
    order = torch.argsort(dst, stable=True)
    assert attn.shape == (len(dst), H)
    assert rel_err(attn, a[order]) < 1e-12
    sums = torch.zeros(n, H, dtype=torch.float64).index_add(0, dst[order], attn.detach())
    assert rel_err(sums, torch.ones(n, H, dtype=torch.float64)) < 1e-12


def test_gat_agg_ref_branch_is_leaky_relu_on_its_own_side():
    """With the sides of its own logits, the branch form is the plain one."""
    H, F = 2, 8
    sb = batch_of_sizes(SIZES, seed=1)
    gd = graph_dict(sb)
    n = int(sb.num_nodes.sum())
    g = torch.Generator().manual_seed(0)
    Z = torch.randn(n, H, F, generator=g, dtype=torch.float64)
    R = torch.randn(n, H * F, generator=g, dtype=torch.float64)
    elr = torch.randn(n, 2 * H, generator=g, dtype=torch.float64)
    bias = torch.randn(H * F, generator=g, dtype=torch.float64)
    src = torch.as_tensor(gd["src"], dtype=torch.long)
    dst = torch.as_tensor(gd["dst"], dtype=torch.long)
    br = (elr[:, :H][src] + elr[:, H:][dst]) > 0
    a = gnn_ref.gat_agg_ref(src, dst, Z, R, elr, bias, H, F, 2, 0.2, None)
    b = gnn_ref.gat_agg_ref(src, dst, Z, R, elr, bias, H, F, 2, 0.2, br)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("H,F", [(3, 8), (4, 6), (4, 516), (8, 260), (16, 4), (4, 0)])
def test_gatlayer_refuses_unsupported_shape_at_construction(H, F):
    """Head counts and widths outside the aggregation kernels' range are refused by the
    constructor, with the limit in the message — not by the first forward."""
    from mvml_gat.nn import GATLayer
    with pytest.raises(ValueError, match="num_heads must be 1, 2, 4 or 8"):
        GATLayer(30, F, H)
    GATLayer(30, 1024, 2, agg_mode="mean")  # the widest head-mean layer of two heads constructs


@pytest.mark.parametrize("D", [0, 6, 1028])
def test_set2set_refuses_unsupported_width_at_construction(D):
    from mvml_gat.nn import Set2Set
    with pytest.raises(ValueError, match="multiple of 4 <= 1024"):
        Set2Set(D, 6, 3)
