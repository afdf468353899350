"""The re-association csrc/nnconv.hip rests on, in float64 on the CPU: summing h_u[i] (z_e W2_i) over the
rows i of the per-edge matrix equals NNConv with that matrix materialised, and the three gradient
formulas of the kernels equal autograd's through the materialised form.  1e-12 ("MPNN")."""
import torch

import _mpnn_ref as R
from conftest import rel_err

SRC = torch.tensor([0, 1, 1, 2, 2, 0, 3, 3, 1, 2])  # 10 edges on 5 atoms: atom 4 has no edge, 1 -> 2 twice
DST = torch.tensor([1, 0, 2, 1, 0, 2, 2, 1, 2, 3])


def test_reassociated_nnconv_and_its_gradients_equal_the_materialised_ones():
    N, D, H = 5, 4, 6
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    h, z, W2, g = rnd(N, D).requires_grad_(), rnd(10, H).requires_grad_(), rnd(D * D, H).requires_grad_(), rnd(N, D)
    zero = torch.zeros(D * D, dtype=torch.float64)
    out = R.nnconv(SRC, DST, N, h, z, W2, zero, zero[:D])
    assert rel_err(R.nnconv_reassociated(SRC, DST, N, h, z, W2), out) <= 1e-12
    assert float(out[4].detach().abs().max()) == 0.0
    want = torch.autograd.grad(out, (z, h, W2), g)
    got = R.nnconv_grads_reassociated(SRC, DST, N, h.detach(), z.detach(), W2.detach(), g)
    for name, a, b in zip(("dz", "dH", "dW2"), got, want):
        assert rel_err(a, b) <= 1e-12, name
