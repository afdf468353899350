"""AttentiveFP in plain torch on the CPU, edge-list form (index_add_, a scatter softmax), with the
un-re-associated [E, G] rows: the reference of tests/test_gpu_afp.py and tests/test_afp_cpu.py.
Formulas of dgllife 0.3.0 gnn/attentivefp.py and readout/attentivefp_readout.py as restated in
DESIGN.md "AttentiveFP" (parity with dgllife is unpinned).  Every function works in the dtype of
its tensors; `sd` is an AttentiveFPPredictor state_dict (tensors of that dtype)."""
import torch
import torch.nn.functional as F


def seg_softmax(logit, idx, n):
    """softmax of logit [E] over the entries that share idx."""
    m = torch.full((n,), -float("inf"), dtype=logit.dtype).scatter_reduce(0, idx, logit.detach(), "amax")
    p = torch.exp(logit - m[idx])
    return p / torch.zeros(n, dtype=logit.dtype).index_add_(0, idx, p)[idx]


def seg_sum(rows, idx, n):
    return torch.zeros((n, rows.shape[1]), dtype=rows.dtype).index_add_(0, idx, rows)


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    return gru_gates(x @ w_ih.T, h @ w_hh.T, b_ih, b_hh, h)


def gru_gates(gi, gh, b_ih, b_hh, h):
    ir, iz, i_n = (gi + b_ih).chunk(3, 1)
    hr, hz, hn = (gh + b_hh).chunk(3, 1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(i_n + r * hn)
    return (1 - z) * n + z * h


def context_sum(src, dst, N, P, e, W1e, b1, w2e, t):
    """(s, a): the re-associated edge part of GetContext from node-level P and t (the kernel's contract)."""
    he = F.leaky_relu(P[src] + e @ W1e.T + b1)
    a = seg_softmax(F.leaky_relu(t[dst] + he @ w2e), dst, N)
    return seg_sum(a[:, None] * he, dst, N), a


def get_context(sd, pre, src, dst, x, e):
    N = x.shape[0]
    hv_new = F.leaky_relu(F.linear(x, sd[pre + "project_node.0.weight"], sd[pre + "project_node.0.bias"]))
    he1 = F.leaky_relu(F.linear(torch.cat([x[src], e], 1), sd[pre + "project_edge1.0.weight"], sd[pre + "project_edge1.0.bias"]))
    logit = F.leaky_relu(F.linear(torch.cat([hv_new[dst], he1], 1), sd[pre + "project_edge2.1.weight"],
                                  sd[pre + "project_edge2.1.bias"])).squeeze(1)
    a = seg_softmax(logit, dst, N)
    g = pre + "attentive_gru."
    msg = a[:, None] * F.linear(he1, sd[g + "edge_transform.1.weight"], sd[g + "edge_transform.1.bias"])
    c = F.elu(seg_sum(msg, dst, N))
    return F.relu(gru_cell(c, hv_new, *[sd[g + "gru." + k] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]))


def gnn_layer(sd, pre, src, dst, h, eps=1e-5):
    N = h.shape[0]
    logit = F.leaky_relu(F.linear(torch.cat([h[dst], h[src]], 1), sd[pre + "project_edge.1.weight"],
                                  sd[pre + "project_edge.1.bias"])).squeeze(1)
    a = seg_softmax(logit, dst, N)
    g = pre + "attentive_gru."
    hv = F.linear(h, sd[g + "project_node.1.weight"], sd[g + "project_node.1.bias"])
    c = F.elu(seg_sum(a[:, None] * hv[src], dst, N))
    out = F.relu(gru_cell(c, h, *[sd[g + "gru." + k] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]))
    mean, var = out.mean(0), out.var(0, unbiased=False)  # BatchNorm1d in training mode
    return (out - mean) / torch.sqrt(var + eps) * sd[pre + "bn_layer.weight"] + sd[pre + "bn_layer.bias"]


def attn_pool(gid, B, h, w_node, u, slope=0.01):
    """(r, a) of one readout step's weighted sum from the per-graph u (the kernel's contract)."""
    a = seg_softmax(F.leaky_relu(h @ w_node + u[gid], slope), gid, B)
    return seg_sum(a[:, None] * h, gid, B), a


def readout(sd, pre, gid, B, h, T):
    gf = seg_sum(h, gid, B)
    for t in range(T):
        p = f"{pre}readouts.{t}."
        z = F.leaky_relu(F.linear(torch.cat([F.relu(gf)[gid], h], 1), sd[p + "compute_logits.0.weight"],
                                  sd[p + "compute_logits.0.bias"])).squeeze(1)
        a = seg_softmax(z, gid, B)
        hp = F.linear(h, sd[p + "project_nodes.1.weight"], sd[p + "project_nodes.1.bias"])  # per atom, as dgllife
        ctx = F.elu(seg_sum(a[:, None] * hp, gid, B))
        gf = gru_cell(ctx, gf, *[sd[p + "gru." + k] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])
    return gf


def predictor(sd, src, dst, gid, B, x, e, num_layers, T):
    h = get_context(sd, "gnn.init_context.", src, dst, x, e)
    for i in range(num_layers - 1):
        h = gnn_layer(sd, f"gnn.gnn_layers.{i}.", src, dst, h)
    return F.linear(readout(sd, "readout.", gid, B, h, T), sd["predict.1.weight"], sd["predict.1.bias"])


def molecules():
    """Three hand-written molecules (+ the shapes the kernels must hold): local bond lists, both
    directions.  A single atom (no in-edge), a two-atom molecule, a six-ring, and a 12-atom
    molecule whose atom 0 has 70 in- and 70 out-edges (parallel bonds), past one 64-entry chunk."""
    ring = [(i, (i + 1) % 6) for i in range(6)]
    hub = [(i, i + 1) for i in range(11)] + [(1 + k % 11, 0) for k in range(69)]
    chain = [(i, i + 1) for i in range(18)] + [(0, 9), (4, 15)]
    mols = [(1, []), (2, [(0, 1)]), (6, ring), (12, hub), (19, chain)]
    nn_, ne, src, dst = [], [], [], []
    for n, bonds in mols:
        nn_.append(n)
        ne.append(2 * len(bonds))
        src += [a for a, b in bonds] + [b for a, b in bonds]
        dst += [b for a, b in bonds] + [a for a, b in bonds]
    return nn_, ne, src, dst


def global_ids(nn_, ne, src, dst):
    """(src, dst, gid) as global int64 tensors."""
    off = torch.tensor([0] + nn_).cumsum(0)[:-1]
    shift = torch.repeat_interleave(off, torch.tensor(ne))
    gid = torch.repeat_interleave(torch.arange(len(nn_)), torch.tensor(nn_))
    return torch.tensor(src) + shift, torch.tensor(dst) + shift, gid
