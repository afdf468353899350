"""Weave's readout (dgllife 0.3.0 WeaveGather, restated) in plain torch, dtype-generic, with the
[N, F K] histogram materialised."""
import torch
import torch.nn.functional as F


def histogram(x, means, stds):
    """[N, F] -> [N, F K], column f K + k: q_k = exp(-(x - mu_k)^2 / (2 sigma_k^2)) + 1e-7, p = q / sum q."""
    mu, sd = (torch.as_tensor(v, dtype=x.dtype) for v in (means, stds))
    q = torch.exp(-(x[..., None] - mu) ** 2 / (2 * sd ** 2)) + 1e-7
    return (q / q.sum(-1, keepdim=True)).flatten(1)


def sum_nodes(x, gid, B):
    return torch.zeros((B, x.shape[1]), dtype=x.dtype).index_add_(0, gid, x)


def gather(x, gid, B, means=None, stds=None, W=None, b=None, tanh=True):
    """WeaveGather.forward: without memberships the plain node sum."""
    if means is None:
        return sum_nodes(x, gid, B)
    y = F.linear(sum_nodes(histogram(x, means, stds), gid, B), W, b)
    return torch.tanh(y) if tanh else y
