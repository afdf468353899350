"""D-MPNN in plain torch on the CPU over edge-id order (index_add_ for the sums, a Python loop for
the reverse map): the reference of tests/test_gpu_dmpnn.py and tests/test_dmpnn_cpu.py.  Formulas of
Chemprop v1's MPNEncoder (bond messages, directed, ReLU) as restated in DESIGN.md "D-MPNN" (parity
with Chemprop is unpinned), in the dtype of its tensors; `sd` is a DMPNNPredictor state_dict.

THE REVERSE MAP: for s = (u -> v), the k-th edge u -> v in edge-id order, rev(s) is the k-th edge
v -> u in edge-id order.  A self-loop is its own reverse.  An edge without such a partner has none
(-1), and nothing is subtracted for it."""
import torch
import torch.nn.functional as F

from _afp_ref import seg_sum


def rev_map(src, dst):
    """rev as a list over edge ids (global atom ids in src / dst)."""
    pairs = [(int(u), int(v)) for u, v in zip(src, dst)]
    ids = {}
    for s, p in enumerate(pairs):
        ids.setdefault(p, []).append(s)
    rev = []
    for s, (u, v) in enumerate(pairs):
        k, back = ids[(u, v)].index(s), ids.get((v, u), [])
        rev.append(back[k] if k < len(back) else -1)
    return rev


def _reverse_rows(M, rev):
    rev = torch.as_tensor(rev)
    return M[rev.clamp(min=0)] * (rev >= 0).to(M.dtype)[:, None]


def init(src, x, e, W_i, b_i=None):
    """(input, M0): input_s = W_i [x_u ; e_s] (+ b_i), M0 = relu(input)."""
    inp = F.linear(torch.cat([x[src], e], 1), W_i, b_i)
    return inp, F.relu(inp)


def update(src, dst, rev, N, inp, R, b_h=None):
    """The update kernel's contract, from R = M W_h^T: relu(input + b_h + Q[u] - R[rev]), Q_v = sum_{k -> v} R_k."""
    pre = inp + seg_sum(R, dst, N)[src] - _reverse_rows(R, rev)
    return F.relu(pre if b_h is None else pre + b_h)


def step(src, dst, rev, N, inp, M, W_h, b_h=None):
    """M^t from M^{t-1} as the model states it: W_h applied to the summed messages."""
    return F.relu(inp + F.linear(seg_sum(M, dst, N)[src] - _reverse_rows(M, rev), W_h, b_h))


def encoder(sd, pre, src, dst, rev, x, e, depth):
    N = x.shape[0]
    inp, M = init(src, x, e, sd[pre + "W_i.weight"], sd.get(pre + "W_i.bias"))
    for _ in range(depth - 1):
        M = step(src, dst, rev, N, inp, M, sd[pre + "W_h.weight"], sd.get(pre + "W_h.bias"))
    return F.relu(F.linear(torch.cat([x, seg_sum(M, dst, N)], 1), sd[pre + "W_o.weight"], sd[pre + "W_o.bias"]))


def predictor(sd, src, dst, rev, gid, B, x, e, depth, aggregation):
    h = encoder(sd, "gnn.", src, dst, rev, x, e, depth)
    r = seg_sum(h, gid, B)
    if aggregation == "mean":
        r = r / torch.bincount(gid, minlength=B).to(h.dtype)[:, None]
    return F.linear(F.relu(F.linear(r, sd["predict.0.weight"], sd["predict.0.bias"])), sd["predict.2.weight"], sd["predict.2.bias"])
