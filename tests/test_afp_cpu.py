"""The re-associations behind the AttentiveFP kernels (DESIGN.md "AttentiveFP") reproduce the
un-re-associated [E, G] formulas of tests/_afp_ref.py at float64 on its hand-written molecules, so
a GPU mismatch can be pinned on a kernel rather than on the algebra."""
import pytest
import torch
import torch.nn.functional as F

import _afp_ref as R

Fn_, De, G = 7, 3, 8
TOL = 1e-12


@pytest.fixture(scope="module")
def case():
    nn_, ne, src, dst = R.molecules()
    src, dst, gid = R.global_ids(nn_, ne, src, dst)
    gen = torch.Generator().manual_seed(0)
    N, E = sum(nn_), len(src)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    return dict(src=src, dst=dst, gid=gid, N=N, B=len(nn_), x=rnd(N, Fn_), e=rnd(E, De), h=rnd(N, G), rnd=rnd,
                deg=torch.bincount(dst, minlength=N))


def _close(a, b):
    assert float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def test_context_split_and_masked_bias(case):
    c, rnd = case, case["rnd"]
    src, dst, N, x, e = c["src"], c["dst"], c["N"], c["x"], c["e"]
    Wn, bn, W1, b1, W2, b2, We, be = rnd(G, Fn_), rnd(G), rnd(G, Fn_ + De), rnd(G), rnd(1, 2 * G), rnd(1), rnd(G, G), rnd(G)
    hv_new = F.leaky_relu(x @ Wn.T + bn)
    he1 = F.leaky_relu(torch.cat([x[src], e], 1) @ W1.T + b1)
    a = R.seg_softmax(F.leaky_relu(torch.cat([hv_new[dst], he1], 1) @ W2.T + b2).squeeze(1), dst, N)
    want = R.seg_sum(a[:, None] * (he1 @ We.T + be), dst, N)
    # P = x W1n^T, t = w2n . hv_new + b2, he1 = leaky(P[u] + W1e e + b1), logit = leaky(t_v + w2e . he1)
    s, a2 = R.context_sum(src, dst, N, x @ W1[:, :Fn_].T, e, W1[:, Fn_:], b1, W2[0, G:], hv_new @ W2[0, :G] + b2)
    _close(a2, a)
    _close(s, R.seg_sum(a[:, None] * he1, dst, N))
    assert int((c["deg"] == 0).sum()) == 1  # the single atom: no bias there
    _close(s @ We.T + be * (c["deg"] > 0)[:, None], want)


def test_readout_projects_at_graph_level(case):
    c, rnd = case, case["rnd"]
    gid, B, h = c["gid"], c["B"], c["h"]
    wn, u, Wp, bp = rnd(G), rnd(B), rnd(G, G), rnd(G)
    r, a = R.attn_pool(gid, B, h, wn, u)
    _close(r @ Wp.T + bp, R.seg_sum(a[:, None] * (h @ Wp.T + bp), gid, B))


def test_gnn_layer_logits_are_a_one_head_gat_pair(case):
    c, rnd = case, case["rnd"]
    src, dst, h = c["src"], c["dst"], c["h"]
    w, b = rnd(1, 2 * G), rnd(1)
    want = F.leaky_relu(torch.cat([h[dst], h[src]], 1) @ w.T + b).squeeze(1)
    el, er = h @ w[0, G:], h @ w[0, :G] + b  # el: the source term, er: the destination term with the bias
    _close(F.leaky_relu(el[src] + er[dst]), want)
