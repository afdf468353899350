"""MPNN in plain torch on the CPU, edge-list form with the per-edge [D, D] matrices materialised as
dgl does (NNConv's bmm, index_add_), Set2Set written out: the reference of tests/test_gpu_mpnn.py and
tests/test_mpnn_cpu.py.  Formulas of dgl 0.9.1 NNConv / Set2Set and dgllife 0.3.0 gnn/mpnn.py and
model_zoo/mpnn_predictor.py as restated in DESIGN.md "MPNN" (parity with dgllife is unpinned).  Every
function works in the dtype of its tensors; `sd` is an MPNNPredictor state_dict of that dtype.  The
*_reassociated functions are the kernels' formulas (csrc/nnconv.hip), for the CPU test."""
import torch
import torch.nn.functional as F

from _afp_ref import gru_gates, seg_softmax, seg_sum


def nnconv(src, dst, N, h, z, W2, b2, bias):
    """out_v = sum_{e: u -> v} h_u view(z_e W2^T + b2, [D, D]) + bias; z in edge-id order."""
    D = h.shape[1]
    W = (z @ W2.T + b2).view(-1, D, D)
    return seg_sum(torch.bmm(h[src].unsqueeze(1), W).squeeze(1), dst, N) + bias


def nnconv_reassociated(src, dst, N, h, z, W2):
    """The z W2^T part as mvml_nnconv_fwd forms it: sum_i h_u[i] (z_e W2_i), W2_i = W2[i D:(i + 1) D]."""
    D = h.shape[1]
    m = sum(h[src, i:i + 1] * (z @ W2[i * D:(i + 1) * D].T) for i in range(D))
    return seg_sum(m, dst, N)


def nnconv_grads_reassociated(src, dst, N, h, z, W2, g):
    """(dz, dH, dW2) of nnconv_reassociated from g = dL/d out, by the formulas of mvml_nnconv_bwd_data
    (C'_i = dM W2_i: dz += h[:, i] C'_i, dh_edge[:, i] = <z, C'_i>) and mvml_nnconv_bwd_weight."""
    D = h.shape[1]
    dM, hs = g[dst], h[src]
    C = [dM @ W2[i * D:(i + 1) * D] for i in range(D)]
    dz = sum(hs[:, i:i + 1] * C[i] for i in range(D))
    dH = seg_sum(torch.stack([(z * C[i]).sum(1) for i in range(D)], 1), src, N)
    dW2 = torch.cat([(hs[:, i:i + 1] * dM).T @ z for i in range(D)])
    return dz, dH, dW2


def set2set(gid, B, x, sd, pre, n_iters, n_layers):
    D = x.shape[1]
    hs = [x.new_zeros(B, D) for _ in range(n_layers)]
    cs = [x.new_zeros(B, D) for _ in range(n_layers)]
    q_star = x.new_zeros(B, 2 * D)
    for _ in range(n_iters):
        inp = q_star
        for l in range(n_layers):
            w_ih, w_hh, b_ih, b_hh = (sd[f"{pre}lstm.{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            i, f, c, o = (inp @ w_ih.T + b_ih + hs[l] @ w_hh.T + b_hh).chunk(4, 1)
            cs[l] = torch.sigmoid(f) * cs[l] + torch.sigmoid(i) * torch.tanh(c)
            inp = hs[l] = torch.sigmoid(o) * torch.tanh(cs[l])
        a = seg_softmax((x * inp[gid]).sum(1), gid, B)
        q_star = torch.cat([inp, seg_sum(a[:, None] * x, gid, B)], 1)
    return q_star


def predictor(sd, src, dst, gid, B, x, e, steps, n_iters, n_layers):
    N = x.shape[0]
    h = F.relu(F.linear(x, sd["gnn.project_node_feats.0.weight"], sd["gnn.project_node_feats.0.bias"]))
    p = "gnn.gnn_layer."
    z = F.relu(F.linear(e, sd[p + "edge_func.0.weight"], sd[p + "edge_func.0.bias"]))
    gru = [sd["gnn.gru." + k] for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    for _ in range(steps):
        m = F.relu(nnconv(src, dst, N, h, z, sd[p + "edge_func.2.weight"], sd[p + "edge_func.2.bias"], sd[p + "bias"]))
        h = gru_gates(m @ gru[0].T, h @ gru[1].T, gru[2], gru[3], h)
    r = set2set(gid, B, h, sd, "readout.", n_iters, n_layers)
    return F.linear(F.relu(F.linear(r, sd["predict.0.weight"], sd["predict.0.bias"])), sd["predict.2.weight"], sd["predict.2.bias"])
