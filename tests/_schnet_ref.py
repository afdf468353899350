"""SchNet in plain torch on the CPU, edge-list form, with the [E, K] radial-basis expansion materialised
and index_add_ for the sums: the reference of tests/test_gpu_schnet.py.  Formulas of dgl 0.9.1 CFConv
and dgllife 0.3.0 SchNetGNN / MLPNodeReadout as restated in DESIGN.md "SchNet" (parity with dgllife is
unpinned).  Every function works in the dtype of its tensors; `sd` is a SchNetPredictor state_dict."""
import math

import torch
import torch.nn.functional as F


def ssp(x):
    return F.softplus(x) - math.log(2.0)


def filter(d, centers, gamma, W1, b1, W2, b2):
    """he [E, H] from the distances d [E]."""
    rbf = torch.exp(-gamma * (d[:, None] - centers[None, :]) ** 2)
    return ssp(F.linear(ssp(F.linear(rbf, W1, b1)), W2, b2))


def cfconv(src, dst, N, hv, he):
    """a_v = sum over the edges u -> v of hv[u] * he_e."""
    return torch.zeros((N, hv.shape[1]), dtype=hv.dtype).index_add_(0, dst, hv[src] * he)


def predictor(sd, src, dst, gid, B, types, d, gamma):
    dt = sd["readout.out_project.bias"].dtype
    x, centers = sd["gnn.embed.weight"][types], sd["gnn.rbf.centers"].to(dt)
    for i in range(sum(k.endswith("conv.project_node.weight") for k in sd)):
        p = f"gnn.gnn_layers.{i}."
        lin = lambda t, name: F.linear(t, sd[p + name + ".weight"], sd[p + name + ".bias"])
        he = filter(d, centers, gamma, *(sd[f"{p}conv.project_edge.{j}.{w}"] for j in (0, 2) for w in ("weight", "bias")))
        a = cfconv(src, dst, x.shape[0], lin(x, "conv.project_node"), he)
        x = lin(ssp(lin(a, "conv.project_out.0")), "project_out")
    h = ssp(F.linear(x, sd["readout.in_project.weight"], sd["readout.in_project.bias"]))
    h = F.linear(h, sd["readout.out_project.weight"], sd["readout.out_project.bias"])
    return torch.zeros((B, h.shape[1]), dtype=dt).index_add_(0, gid, h)
