"""Dropout that does not follow a ReLU (functional.DropoutFunction / functional.dropout: the
Dropout MLPPredictor opens with).  It is mvml_dropout_fwd out of place, and its backward is the
same kernel on g_y with the saved (p, seed): the mask is a function of (seed, element index) alone.

Inputs are |randn| + 1, so no element is 0 and a dropped element is recognised by reading 0."""
import pytest
import torch

from mvml_gat import functional as Fn
from mvml_gat._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (4099, 61)  # 250,039 elements: odd, so the scalar tail of the float4 kernel runs


def _x(seed=1):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(seed)).abs().add(1).to(DEV)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_forward_values_fraction_and_mask_of_the_in_place_kernel(p):
    x = _x().requires_grad_()
    y = Fn.DropoutFunction.apply(x, p, 4242)
    assert y.shape == x.shape and y.data_ptr() != x.data_ptr()  # out of place: x is intact
    assert torch.equal(x.detach(), _x())
    kept = y.detach() != 0
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device=DEV)  # float32(1 / (1 - p))
    assert torch.equal(y.detach()[kept], (x.detach() * scale)[kept])
    n = x.numel()
    frac = kept.double().mean().item()
    assert abs(frac - (1 - p)) < 6 * (p * (1 - p) / n) ** 0.5, (frac, 1 - p)
    # the same (seed, i) gives the in-place mvml_dropout_fwd's mask
    z = x.detach().clone()
    call("mvml_dropout_fwd", n, ptr(z), ptr(z), float(p), 4242, stream_ptr())
    assert torch.equal(z, y.detach())
    # backward: g_x = g_y * mask * scale, bitwise, the mask read off the forward
    g_y = torch.randn(SHAPE, generator=torch.Generator().manual_seed(2)).to(DEV)
    y.backward(g_y)
    assert torch.equal(x.grad, torch.where(kept, g_y * scale, torch.zeros_like(g_y)))


def test_seed_comes_from_torch_manual_seed():
    x = _x()
    torch.manual_seed(11)
    a = Fn.dropout(x, 0.5)
    b = Fn.dropout(x, 0.5)
    torch.manual_seed(11)
    a2 = Fn.dropout(x, 0.5)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    torch.manual_seed(11)
    assert torch.equal(Fn.DropoutFunction.apply(x, 0.5), a)  # no seed given: one dropout_seed() draw


def test_p0_and_eval_mode_are_the_identity_with_no_launch():
    x = _x().requires_grad_()
    assert Fn.dropout(x, 0.0) is x
    mod = torch.nn.Dropout(0.5).eval()
    assert Fn.dropout_p(mod) == 0.0 and Fn.dropout(x, Fn.dropout_p(mod)) is x
    state = torch.get_rng_state()
    y = Fn.DropoutFunction.apply(x, 0.0)
    assert torch.equal(torch.get_rng_state(), state)  # no seed drawn
    assert y.data_ptr() == x.data_ptr() and torch.equal(y.detach(), x.detach())  # x's own values: nothing written
    g = torch.ones_like(y)
    y.backward(g)
    assert torch.equal(x.grad, g)
    with pytest.raises(ValueError, match="< 1"):
        Fn.dropout(x, 1.0)
    with pytest.raises(ValueError, match="< 1"):
        Fn.DropoutFunction.apply(x, 1.0)
