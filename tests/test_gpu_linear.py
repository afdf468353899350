"""nn.Linear on the HIP path is one function whichever autograd Function carries it:
fusion.LinearFunction and LinearReLUFunction (p = 0, every pre-activation positive, so its ReLU
and ReLU backward are the identity) return bitwise the same output and gradients, each within
the 1e-5 norm-wise bar of the float64 products, with and without an input gradient, under
per-row and per-operand split-fp16 scales.  K = 6 has no 16-B weight image (split_il4 is None)."""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-5


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _run(function, x, w, b, g, need_gx, *extra):
    xd = x.float().to(DEV).requires_grad_(need_gx)
    wd, bd = w.float().to(DEV).requires_grad_(), b.float().to(DEV).requires_grad_()
    y = function.apply(xd, wd, bd, *extra)
    y.backward(g.float().to(DEV))
    return y.detach(), xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("row_scales", [None, False], ids=["default", "operand_scales"])
@pytest.mark.parametrize("Nout", [1, 12])
@pytest.mark.parametrize("K", [6, 8, 76])
@pytest.mark.parametrize("M", [1, 5, 257])
def test_linear_is_one_function_in_both_carriers(M, K, Nout, row_scales):
    from mvml_gat import functional as Fn
    from mvml_gat.fusion import LinearFunction
    gen = torch.Generator().manual_seed(1000 * M + 10 * K + Nout)
    # non-negative entries and a bias of +1: every pre-activation is >= 1
    x = torch.rand(M, K, generator=gen, dtype=torch.float64)
    w = torch.rand(Nout, K, generator=gen, dtype=torch.float64)
    b = torch.ones(Nout, dtype=torch.float64)
    # the upstream gradient: both signs, mean 1/4, so that no column sum over the M rows cancels
    # (sum |g| / |sum g| is about 1.25) and the norm-wise bar measures the arithmetic
    g = torch.rand(M, Nout, generator=gen, dtype=torch.float64) - 0.25
    x, w, g = x.float().double(), w.float().double(), g.float().double()  # what the device is given
    ref = (x @ w.t() + b, g @ w, g.t() @ x, g.sum(0))
    prev = Fn.ROW_SCALES
    try:
        if row_scales is not None:
            Fn.ROW_SCALES = row_scales
        plain = _run(LinearFunction, x, w, b, g, True)
        relu = _run(Fn.LinearReLUFunction, x, w, b, g, True, 0.0)
        plain_nogx = _run(LinearFunction, x, w, b, g, False)
        relu_nogx = _run(Fn.LinearReLUFunction, x, w, b, g, False, 0.0)
    finally:
        Fn.ROW_SCALES = prev
    names = ("y", "gx", "gw", "gb")
    for n, a, c, r in zip(names, plain, relu, ref):
        ea, ec = rel_err(a, r), rel_err(c, r)
        print(f"linear M={M} K={K} Nout={Nout} {n}: rel err {ea:.2e} / {ec:.2e}")
        assert _bits_equal(a, c), n
        assert ea <= TOL and ec <= TOL, (n, ea, ec)
    for with_gx, without in ((plain, plain_nogx), (relu, relu_nogx)):
        assert without[1] is None
        assert _bits_equal(with_gx[0], without[0])
        assert _bits_equal(with_gx[2], without[2]) and _bits_equal(with_gx[3], without[3])
