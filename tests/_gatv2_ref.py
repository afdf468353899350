"""GATv2 restated in plain torch on the CPU (dgl 0.9.1 GATv2Conv, dgllife 0.3.0 GATv2Layer /
GATv2): the reference of the GATv2 tests.  TEST INFRASTRUCTURE ONLY; dgl and dgllife are not
available here, so parity with them is unpinned ("GATv2").

Every function runs in the dtype of its inputs (float64 for parity, float32 for the reference's
own error) and is differentiable with torch autograd, which supplies the reference backward.
"""
import torch
import torch.nn.functional as F

from oracle.gnn_ref import edge_softmax_ref, leaky_relu_branch


def _long(a):
    return torch.as_tensor(a).to(torch.long)


def gatv2_agg_ref(src, dst, ZL, ZR, R, attn, H, F_, mode, slope=0.2, branch=None):
    """GATv2Conv from apply_edges to the layer output, at the cut of mvml_gatv2_agg_fwd: ZL, ZR
    [N, H F], R ([N, H F], [N, F] = its head mean in mode 1, or None) and attn [H F] are inputs
    (leaves).  branch: optional bool [E, H, F] side of LeakyReLU per element (edge-id order).
    mode 0 flatten + ELU, 1 head mean, 2 flatten.  Returns (out, a in in-CSR slot order)."""
    src, dst = _long(src), _long(dst)
    n = ZL.shape[0]
    zl = ZL.view(n, H, F_)
    p = zl[src] + ZR.view(n, H, F_)[dst]
    e = F.leaky_relu(p, slope) if branch is None else leaky_relu_branch(p, slope, branch)
    s = (e * attn.view(1, H, F_)).sum(-1)
    a = edge_softmax_ref(s, dst, n)
    rst = torch.zeros((n, H, F_), dtype=ZL.dtype).index_add(0, dst, a.unsqueeze(-1) * zl[src])
    if mode == 1:
        out = rst.mean(1)
        if R is not None:
            out = out + R
    else:
        if R is not None:
            rst = rst + R.view(n, H, F_)
        out = rst.flatten(1)
        if mode == 0:
            out = F.elu(out)
    return out, a[torch.argsort(dst, stable=True)]


def gatv2_layer_ref(src, dst, X, p, H, F_, agg_mode, activation, slope=0.2, branch=None, return_attention=False):
    """dgllife GATv2Layer.forward.  p: the conv's parameters by state_dict key (fc_src.weight,
    fc_src.bias, fc_dst.*, attn, res_fc.*; absent keys: no such parameter; res_fc "identity" via
    p["res_identity"] = True).  The activation is the conv's, applied per head before the
    flatten / mean."""
    src, dst = _long(src), _long(dst)
    n = X.shape[0]

    def lin(name):
        y = X @ p[name + ".weight"].t()
        b = p.get(name + ".bias")
        return y if b is None else y + b

    zl = lin("fc_src").view(n, H, F_)
    zr = lin("fc_dst").view(n, H, F_)
    pe = zl[src] + zr[dst]
    e = F.leaky_relu(pe, slope) if branch is None else leaky_relu_branch(pe, slope, branch)
    s = (e * p["attn"].view(1, H, F_)).sum(-1)
    a = edge_softmax_ref(s, dst, n)
    rst = torch.zeros((n, H, F_), dtype=X.dtype).index_add(0, dst, a.unsqueeze(-1) * zl[src])
    if "res_fc.weight" in p:
        rst = rst + lin("res_fc").view(n, H, F_)
    elif p.get("res_identity"):
        rst = rst + X.view(n, H, F_)
    if activation is not None:
        rst = activation(rst)
    out = rst.flatten(1) if agg_mode == "flatten" else rst.mean(1)
    return (out, a, pe) if return_attention else out


def gatv2_ref(src, dst, X, layer_params, hidden_feats, num_heads=None, branches=None):
    """dgllife GATv2 with its defaults: 'flatten' + ELU for all but the last layer, 'mean' last."""
    n = len(hidden_feats)
    num_heads = num_heads or [4] * n
    h = X
    for i in range(n):
        last = i == n - 1
        h = gatv2_layer_ref(src, dst, h, layer_params[i], num_heads[i], hidden_feats[i],
                            "mean" if last else "flatten", None if last else F.elu,
                            branch=None if branches is None else branches[i])
    return h


def conv_params(conv, dtype=torch.float64):
    """A GATv2Conv's parameters as gatv2_layer_ref's dict: detached leaves of `dtype` on the CPU."""
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_() for k, v in conv.state_dict().items()}
    if getattr(conv, "share_weights", False):
        for k in ("weight", "bias"):
            if "fc_src." + k in p:
                p["fc_dst." + k] = p["fc_src." + k]
    if isinstance(conv.res_fc, torch.nn.Identity):
        p["res_identity"] = True
    return p
