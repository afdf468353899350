"""Reference of the weighted-sum-and-max readout in plain torch on the CPU (float64 for parity,
float32 for the reference's own error), restated from dgllife 0.3.0 WeightAndSum /
WeightedSumAndMax and dgl 0.9.1 sum_nodes / max_nodes (parity with them unpinned, like oracle/).

Per molecule g with atoms n in [offsets[g], offsets[g + 1]):
    s_n = sigmoid(<W, x_n> + b);  out[g] = [ sum_n s_n x_n | max_n x_n ]
The max is a gather at the FIRST atom index attaining the segment maximum, so autograd routes the
max gradient to that atom alone (amax's backward would split it among ties).  A molecule without
atoms gives a zero row, argmax -1 and no gradient."""
import numpy as np
import torch


def wsum_max_ref(node_offsets, X, W, b, argmax=None):
    """X [N, D], W [1, D] or [D], b [1] -> (out [B, 2 D], argmax int64 [B, D] of global atom
    indices).  argmax given (int [B, D], -1 for a molecule without atoms): the max half gathers
    at those atoms instead of at the first maximum."""
    offs = [int(o) for o in np.asarray(node_offsets).reshape(-1)]
    D = X.shape[1]
    s = torch.sigmoid(X @ W.reshape(-1) + b.reshape(()))
    rows, ams = [], []
    for g, (n0, n1) in enumerate(zip(offs[:-1], offs[1:])):
        if n1 == n0:
            rows.append(X.new_zeros(2 * D))
            ams.append(torch.full((D,), -1, dtype=torch.long))
            continue
        xs = X[n0:n1]
        if argmax is None:
            xd = xs.detach()
            top = xd.max(0).values
            idx = torch.arange(n1 - n0).unsqueeze(1).expand(-1, D)
            am = torch.where(xd == top, idx, torch.full_like(idx, n1 - n0)).min(0).values
        else:
            am = torch.as_tensor(argmax[g]).long().cpu() - n0
        rows.append(torch.cat([(s[n0:n1].unsqueeze(1) * xs).sum(0), xs.gather(0, am.unsqueeze(0))[0]]))
        ams.append(am + n0)
    if not rows:
        return X.new_zeros((0, 2 * D)), torch.zeros((0, D), dtype=torch.long)
    return torch.stack(rows), torch.stack(ams)


def gate_ref(X, W, b):
    return torch.sigmoid(X @ W.reshape(-1) + b.reshape(()))
