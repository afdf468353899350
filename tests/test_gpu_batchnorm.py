"""mvml_batchnorm1d_fwd / _bwd (csrc/batchnorm.hip) at the C ABI against torch.nn.functional.
batch_norm in float64 on the CPU, in training and eval mode.

Every buffer is row-pitched with NaN pad columns on the inputs and sentinels in the pads, a guard
row and the tails of the outputs; the workspace carries a sentinel tail past
mvml_batchnorm1d_workspace_size.  Pads, guards and tails must come back untouched.

The kernels run CT column lanes x RT = 256 / CT rows in flight per workgroup (CT = the power of
two >= the row's float4 count on the float4 path, its float count on the scalar path, at most 64),
one workgroup per (column tile, stripe), R = mvml_batchnorm1d_part_rows(M) = min(ceil(M / 64),
1024) stripes of ceil(M / R) rows; each CASE names the path it reaches.

Bar: a flat 1e-5 (conftest.rel_err, norm-wise) on y, running_mean, running_var, g_x, g_weight and
g_bias for every pattern and both modes — fp64 internals leave only the final fp32 rounding
(2^-24 = 6e-8 per element, and the same on the fp32 running statistics).  It is NOT relative to
the float32 reference's error: on `offset` fp32 torch itself is off by 2e-5 .. 4e-5 on y and up to
4.7e-4 on g_weight, and the kernel has to beat it.  One exception, M = 2 in training: g_x cancels
to ~eps / var of its terms, so its error is measured against max |g_y weight invstd| (the
un-cancelled scale, from the float64 reference) and held to 1e-5.
Each case prints its worst err / budget."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from mvml_gat._lib import MvmlError, call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
EPS, MOM = 1e-5, 0.1
SENT = 7.0
NAN = float("nan")

# (M, C, pad columns, element offset of the x / y / g_y / g_x bases, the path)
CASES = [
    (2, 1, 0, 0, "scalar, CT = 1: 256 rows in flight; M = 2"),
    (2, 128, 0, 0, "float4, CT = 32; M = 2"),
    (3, 3, 0, 0, "scalar, CT = 4 with a masked lane"),
    (3, 4, 0, 0, "float4, CT = 1"),
    (63, 64, 0, 0, "float4, CT = 16: one stripe, the 4-row unrolled loop and its tail"),
    (63, 64, 0, 1, "C % 4 == 0 on bases 4 bytes off 16-byte alignment: scalar path"),
    (63, 65, 0, 0, "scalar, CT = 64: two column tiles, the second with one live lane"),
    (65, 4, 4, 0, "float4 at pitch C + 4; two stripes (33 + 32 rows)"),
    (65, 128, 3, 0, "C % 4 == 0 at pitch C + 3: scalar path, two column tiles, two stripes"),
    (65, 130, 0, 0, "scalar, three column tiles, the last with two live lanes"),
    (257, 1, 0, 0, "scalar, CT = 1; five stripes of 52 rows, the last of 49"),
    (257, 260, 0, 0, "float4, 65 quads: two column tiles, the second with one live lane; five stripes"),
    (4099, 64, 0, 0, "65 stripes of 64 rows and a ragged one of 3: the stripe sum's unrolled loop and tail"),
    (4099, 3, 3, 0, "scalar at pitch C + 3, 65 stripes"),
    (65537, 4, 0, 0, "the stripe cap: 1024 stripes of 65 rows, the last 15 of them empty"),
]
PATTERNS = ["normal", "offset", "relu", "const"]


def _inputs(M, C, pattern):
    gen = torch.Generator().manual_seed(7919 * M + 31 * C + len(pattern))
    x = torch.randn((M, C), generator=gen)
    if pattern == "offset":
        x = x + 1000
    elif pattern == "relu":
        x = torch.relu(x)
    elif pattern == "const":
        x[:, C // 2] = 0.7
    return dict(x=x, w=1 + 0.5 * torch.randn(C, generator=gen), b=torch.randn(C, generator=gen),
                rm=0.1 * torch.randn(C, generator=gen), rv=0.5 + torch.rand(C, generator=gen),
                gy=torch.randn((M, C), generator=gen))


def _padded(t, pad, off, fill, guard_rows=1):
    """t's rows at a pitch of C + pad inside a flat buffer filled with `fill`, `off` elements past
    the buffer's (256-byte aligned) start, followed by guard rows.  Returns (flat, view)."""
    M, C = t.shape
    ld = C + pad
    flat = torch.full((off + (M + guard_rows) * ld + 4,), fill, dtype=torch.float32)
    flat[off:off + M * ld].view(M, ld)[:, :C] = t
    return flat.to(DEV), ld


def _view(flat, M, C, ld, off):
    return flat[off:off + M * ld].view(M, ld)[:, :C]


def _untouched(flat, M, C, ld, off, what):
    """Everything of an output buffer outside its M x C block still holds the sentinel."""
    f = flat.clone()
    _view(f, M, C, ld, off).fill_(SENT)
    assert bool((f == SENT).all()), f"{what}: a pad column, the guard row or the tail was written"


def _run(M, C, inp, training, pad=0, off=0, rm=None, rv=None, nbt=None, check=True):
    """One forward and backward at the C ABI.  rm / rv / nbt: device tensors, updated in place in
    training mode."""
    L = lib()
    st = stream_ptr()
    xf, ld = _padded(inp["x"], pad, off, NAN)
    gyf, _ = _padded(inp["gy"], pad, off, NAN)
    yf, _ = _padded(torch.full((M, C), SENT), pad, off, SENT)
    gxf, _ = _padded(torch.full((M, C), SENT), pad, off, SENT)
    w, b = inp["w"].to(DEV), inp["b"].to(DEV)
    save = torch.full((2, C + 4), SENT, dtype=torch.float64, device=DEV)
    gwb = torch.full((2, C + 4), SENT, device=DEV)
    wsz = L.mvml_batchnorm1d_workspace_size(M, C)
    assert wsz >= 2 * L.mvml_batchnorm1d_part_rows(M) * C * 8
    ws = torch.full((wsz + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    p4 = lambda t: ptr(t[off:])
    call("mvml_batchnorm1d_fwd", M, C, p4(xf), ld, ptr(w), ptr(b), int(training), MOM, EPS, ptr(rm), ptr(rv),
         ptr(nbt), p4(yf), ld, ptr(save[0]), ptr(save[1]), ptr(ws), wsz, st)
    call("mvml_batchnorm1d_bwd", M, C, p4(xf), ld, ptr(w), int(training), ptr(save[0]), ptr(save[1]), p4(gyf), ld,
         p4(gxf), ld, ptr(gwb[0]), ptr(gwb[1]), ptr(ws), wsz, st)
    torch.cuda.synchronize()
    if check:
        _untouched(yf, M, C, ld, off, "y")
        _untouched(gxf, M, C, ld, off, "g_x")
        assert bool((save[:, C:] == SENT).all()) and bool((gwb[:, C:] == SENT).all()), "a [C] output's tail written"
        assert bool((ws[wsz:] == 0xA5).all()), "workspace written past mvml_batchnorm1d_workspace_size"
        assert bool(torch.isnan(xf).sum() == xf.numel() - M * C), "an input was written"
    return dict(y=_view(yf, M, C, ld, off).clone(), gx=_view(gxf, M, C, ld, off).clone(), gw=gwb[0, :C].clone(),
                gb=gwb[1, :C].clone(), mean=save[0, :C].clone(), invstd=save[1, :C].clone())


def _ref64(inp, training, rm, rv):
    """float64 torch on the CPU: outputs, gradients and (training) the updated running statistics."""
    x, w, b = (inp[k].double().clone().requires_grad_() for k in ("x", "w", "b"))
    rm, rv = rm.double().cpu().clone(), rv.double().cpu().clone()
    y = F.batch_norm(x, rm, rv, w, b, training, MOM, EPS)
    y.backward(inp["gy"].double())
    return dict(y=y.detach(), gx=x.grad, gw=w.grad, gb=b.grad, rm=rm, rv=rv)


def _margins(got, ref, keys, gx_scale=None):
    m = {}
    for k in keys:
        assert bool(torch.isfinite(got[k]).all()), k
        if k == "gx" and gx_scale is not None:  # M = 2, training: against the un-cancelled scale
            m[k] = (float((got[k].double().cpu() - ref[k]).abs().max()) / gx_scale, TOL)
        else:
            m[k] = (rel_err(got[k], ref[k]), TOL)
    return m


def _report(tag, m):
    worst = max(m, key=lambda k: m[k][0] / m[k][1])
    print(f"batchnorm1d {tag}: worst err/budget {worst}: {m[worst][0]:.2e} / {m[worst][1]:.0e} = "
          f"{m[worst][0] / m[worst][1]:.3f}")
    for k, (e, budget) in m.items():
        assert e < budget, (tag, k, e, budget)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", CASES, ids=[f"M{c[0]}-C{c[1]}-pad{c[2]}-off{c[3]}" for c in CASES])
def test_against_float64(case, pattern):
    M, C, pad, off, path = case
    inp = _inputs(M, C, pattern)
    rm, rv = inp["rm"].to(DEV), inp["rv"].to(DEV)
    nbt = torch.tensor([5, -1], dtype=torch.int64, device=DEV)  # [1]: a guard
    # training: batch statistics, the running statistics and the counter updated by the kernel
    ref = _ref64(inp, True, inp["rm"], inp["rv"])
    got = _run(M, C, inp, True, pad, off, rm, rv, nbt)
    got.update(rm=rm.clone(), rv=rv.clone())
    assert nbt.tolist() == [6, -1]
    scale = None
    if M == 2:
        var = inp["x"].double().var(0, unbiased=False)
        scale = float((inp["gy"].double() * inp["w"].double() / (var + EPS).sqrt()).abs().max())
    m = _margins(got, ref, ("y", "rm", "rv", "gx", "gw", "gb"), scale)
    if pattern == "const":  # var = 0 exactly: invstd = 1 / sqrt(eps), y = bias
        c = C // 2
        assert float(got["invstd"][c]) == pytest.approx(EPS ** -0.5, rel=1e-12)
        assert rel_err(got["y"][:, c], inp["b"][c].expand(M)) < 1e-6
    _report(f"M={M} C={C} pad={pad} off={off} {pattern} train [{path}]", m)
    # eval: the running statistics the training call left (fp32), nothing updated
    rm0, rv0 = rm.clone(), rv.clone()
    ref = _ref64(inp, False, rm0, rv0)
    got = _run(M, C, inp, False, pad, off, rm, rv, nbt)
    assert nbt.tolist() == [6, -1], "num_batches_tracked advanced in eval mode"
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0), "running statistics changed in eval mode"
    _report(f"M={M} C={C} pad={pad} off={off} {pattern} eval", _margins(got, ref, ("y", "gx", "gw", "gb")))


def test_second_training_call_counts_and_blends_again():
    M, C = 65, 128
    inp = _inputs(M, C, "normal")
    rm, rv = inp["rm"].to(DEV), inp["rv"].to(DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    rm64, rv64 = inp["rm"].double(), inp["rv"].double()
    for step in (1, 2, 3):
        _run(M, C, inp, True, rm=rm, rv=rv, nbt=nbt)
        F.batch_norm(inp["x"].double(), rm64, rv64, None, None, True, MOM, EPS)
        assert int(nbt) == step
    assert rel_err(rm, rm64) < TOL and rel_err(rv, rv64) < TOL
    _run(M, C, inp, True, rm=rm, rv=rv, nbt=None)  # a NULL counter is allowed
    assert int(nbt) == 3


def test_one_row_in_eval_mode_and_bitwise_alone_or_in_a_batch():
    M, C = 65, 128
    inp = _inputs(M, C, "normal")
    rm, rv = inp["rm"].to(DEV), inp["rv"].to(DEV)
    full = _run(M, C, inp, False, rm=rm, rv=rv)
    ref = _ref64(inp, False, inp["rm"], inp["rv"])
    _report("M=65 C=128 eval", _margins(full, ref, ("y", "gx", "gw", "gb")))
    for r, pad in ((0, 0), (31, 0), (64, 3)):  # pad 3: the row alone on the scalar path
        one = {k: (v[r:r + 1] if v.dim() == 2 else v) for k, v in inp.items()}
        alone = _run(1, C, one, False, pad=pad, rm=rm, rv=rv)
        assert torch.equal(alone["y"][0], full["y"][r]), f"row {r}: y differs alone and in the batch"
        assert torch.equal(alone["gx"][0], full["gx"][r])
    ref1 = _ref64(one, False, inp["rm"], inp["rv"])
    _report("M=1 C=128 eval", _margins(alone, ref1, ("y", "gx", "gw", "gb")))
    with pytest.raises(MvmlError, match="batchnorm1d_fwd: training needs more than 1 value"):
        _run(1, C, one, True, rm=rm, rv=rv)


@pytest.mark.parametrize("M, C, pad", [(257, 260, 0), (65, 130, 0), (4099, 64, 4)])
def test_bitwise_repeatable_and_column_permutation_invariant(M, C, pad):
    inp = _inputs(M, C, "offset")
    perm = torch.randperm(C, generator=torch.Generator().manual_seed(C))
    pin = {k: (v[:, perm] if v.dim() == 2 else v[perm]).contiguous() for k, v in inp.items()}
    for training in (True, False):
        runs = []
        for which in (inp, inp, pin):
            rm, rv = which["rm"].to(DEV), which["rv"].to(DEV)
            out = _run(M, C, which, training, pad=pad, rm=rm, rv=rv, check=False)
            out.update(rm=rm, rv=rv)
            runs.append(out)
        a, b, p = runs
        pd = perm.to(DEV)
        for k in a:
            assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
            want = a[k][:, pd] if a[k].dim() == 2 else a[k][pd]
            assert torch.equal(p[k], want), f"{k}: permuting the columns changes a column's bits"
