"""The fusion head at widths other than the default 384: D = hidden_feats[-1] a multiple of 4
in [16, 384] (the masked instances of mvml_token_attn_* / mvml_attn_conv_*), held to the bar of
test_gpu_fusion.py — fp32 outputs and gradients within 1e-5 of the float64 oracle
oracle/fusion_ref.py MVFusionRef(D, 12, 11) on identical seeded weights and inputs.

Widths: 16 (one partial 64-column group, 14 output columns, all in wave 0's conv tile), 20 (no
multiple of 8), 64 (exactly one full group), 100 (a partial second group, the conv tiles end
inside wave 3), 192 (the reference's other layer size), 380 (six groups, the last partial); and
every group boundary 128, 256, 320 with the width just above each of the five (68 .. 324), so that
every <kMask, kV> instance is launched and a width mapped to the wrong one fails.
Batches: 300 gives the fused kernels (256 workgroups) more than one molecule per workgroup with a
short last run."""
import math

import pytest
import torch

from conftest import rel_err
from test_gpu_fusion import _check_relu_flips, _pair, _relu_sides

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
WIDTHS = [16, 20, 64, 100, 192, 380]
# every 64-column group boundary and the width just above it: with WIDTHS these launch the masked
# instances of all six group counts (kV = 4 at 196 and 256, kV = 5 at 260 and 320) and sit on both
# sides of every step of the width dispatch.  Two small batches: they are here to reach the
# instance, not the molecule loop.
BOUNDARY_WIDTHS = [68, 128, 132, 196, 256, 260, 320, 324]
WIDTH_BATCHES = ([(D, B) for D in WIDTHS for B in (1, 5, 67, 300)] +
                 [(D, B) for D in BOUNDARY_WIDTHS for B in (1, 5)])


@pytest.mark.parametrize("path", ["fused", "fold", "qkv"])
@pytest.mark.parametrize("D,B", WIDTH_BATCHES)
def test_fusion_width_parity(D, B, path, monkeypatch):
    """test_fusion_forward_backward_parity at width D: natural biases, the oracle on the
    product's own ReLU sides; logits, the three input gradients and every parameter gradient
    within 1e-5 (no cancellation exception at these sizes: the same oracle in fp32 is within
    3.1e-6 of float64 over all (D, B) pairs)."""
    import mvml_gat.fusion as fu
    monkeypatch.setattr(fu, "FOLD_QK", path != "qkv")
    monkeypatch.setattr(fu, "FUSE_ATTN_CONV", path == "fused")
    ref, mod, xs = _pair(B, seed=B, dim=D)
    xr = [x.clone().requires_grad_(True) for x in xs]
    xd = [x.float().to(DEV).requires_grad_(True) for x in xs]
    zd, conv, mlp = _relu_sides(mod, xd)
    assert conv.shape == (B, 12, 1, D - 2)
    _check_relu_flips(ref, [x.detach() for x in xr], conv, mlp)
    zr = ref(*xr, conv_branch=conv, mlp_branch=mlp)
    assert rel_err(zd, zr) < TOL
    up = torch.randn(zr.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (zr * up).sum().backward()
    (zd * up.float().to(DEV)).sum().backward()
    for a, b in zip(xd, xr):
        assert rel_err(a.grad, b.grad) < TOL
    pr = dict(ref.named_parameters())
    for name, p in mod.named_parameters():
        if name.startswith("norm_layer."):
            assert p.grad is None  # constructed but unused, as in the reference
            continue
        assert rel_err(p.grad, pr[name].grad) < TOL, name


@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("D", [16, 100, 256, 260, 380])
def test_attn_conv_fused_matches_unfused_at_width(D, B, monkeypatch):
    """test_attn_conv_fused_matches_unfused at width D: logits, input gradients and the Q / K / V
    weight gradients bit-identical; the Conv2d weight / bias gradients within 1e-5."""
    import mvml_gat.fusion as fu
    _, mod, xs = _pair(B, seed=5, dim=D)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(fu, "FUSE_ATTN_CONV", fused)
        mod.zero_grad()
        xd = [x.float().to(DEV).requires_grad_(True) for x in xs]
        z = mod(*xd)
        (z * torch.linspace(-1, 1, z.numel(), device=DEV).view(z.shape)).sum().backward()
        res[fused] = (z.detach().clone(), [x.grad.clone() for x in xd],
                      {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None})
    (z1, gx1, gp1), (z0, gx0, gp0) = res[True], res[False]
    assert torch.equal(z1, z0)
    for a, b in zip(gx1, gx0):
        assert torch.equal(a, b)
    for n in gp0:
        if n.startswith("conv."):
            assert rel_err(gp1[n], gp0[n]) < 1e-5, n
        else:
            assert torch.equal(gp1[n], gp0[n]), n


SENTINEL = -12345.0


class _Guarded:
    """A (rows, cols) view with leading dimension ld >= cols inside a larger allocation filled
    with a sentinel: `front` floats before the first row, the pad columns [cols, ld) of every
    row, and `back` floats after the last row must still hold the sentinel after the kernels."""

    def __init__(self, rows, cols, ld, front=64, back=512):
        self.rows, self.cols, self.ld, self.front = rows, cols, ld, front
        self.buf = torch.full((front + rows * ld + back,), SENTINEL, device=DEV)
        self.mat = self.buf[front:front + rows * ld].view(rows, ld)

    @property
    def view(self):
        return self.mat[:, :self.cols]

    def check(self, name):
        assert torch.all(self.buf[:self.front] == SENTINEL), name + ": written before the buffer"
        assert torch.all(self.buf[self.front + self.rows * self.ld:] == SENTINEL), name + ": written past the buffer"
        if self.ld > self.cols:
            assert torch.all(self.mat[:, self.cols:] == SENTINEL), name + ": pad columns written"
        assert not torch.any(self.view == SENTINEL), name + ": elements left unwritten"


@pytest.mark.parametrize("D", [16, 100, 196, 260])
def test_width_abi_stores_stay_inside_rows(D):
    """mvml_token_attn_fold_fwd / _bwd and mvml_attn_conv_fwd / _bwd called directly: every
    output lives in a sentinel-filled allocation (g_pv with ldg > 2 * 12 * D, g_k with ldgk > D)
    and the sentinel survives around it; the fused and separate entries agree as
    test_attn_conv_abi_matches_separate_kernels requires (P, out, g_pv, g_k, max |g_pv| and the
    folded g_pv row maxima bit-identical; Conv2d weight / bias gradients within 1e-5)."""
    from mvml_gat._lib import call, lib, ptr, ws_ptr_size
    B, H = 7, 12
    g = torch.Generator(device=DEV).manual_seed(D)
    HD = H * D
    PV = torch.randn(3 * B, 2 * HD, device=DEV, generator=g)
    Xn = torch.randn(3 * B, D, device=DEV, generator=g)
    w = torch.randn(12, 12, 3, 3, device=DEV, generator=g) * 0.1
    bias = torch.randn(12, device=DEV, generator=g) * 0.1
    gout = torch.randn(B, 12, D - 2, device=DEV, generator=g)
    sc = 1.0 / math.sqrt(D)
    st = torch.cuda.current_stream().cuda_stream
    L = lib()
    ldg, ldgk = 2 * HD + 12, D + 4
    res = {}
    for fused in (True, False):
        P = _Guarded(B, H * 9, H * 9)
        out = _Guarded(B, 12 * (D - 2), 12 * (D - 2))
        gPV = _Guarded(3 * B, 2 * HD, ldg)
        gk = _Guarded(3 * B, D, ldgk)
        gw, gb = torch.empty_like(w), torch.empty_like(bias)
        amx = torch.zeros(1, dtype=torch.int32, device=DEV)
        guards = dict(P=P, out=out, gPV=gPV, gk=gk)
        if fused:
            call("mvml_attn_conv_fwd", B, H, D, ptr(PV), 2 * HD, ptr(Xn), D, sc, ptr(w), ptr(bias),
                 ptr(P.mat), ptr(out.mat), 0.0, 0, st)
            wp, wn = ws_ptr_size(L.mvml_attn_conv_bwd_workspace_size(B), DEV)
            rows = torch.zeros(3 * B, dtype=torch.int32, device=DEV)
            call("mvml_attn_conv_bwd", B, H, D, ptr(PV), 2 * HD, ptr(Xn), D, sc, ptr(P.mat), ptr(w),
                 ptr(out.mat), ptr(gout), 1.0, ptr(gPV.mat), ldg, ptr(gk.mat), ldgk, ptr(amx), ptr(rows),
                 ptr(gw), ptr(gb), wp, wn, st)
            torch.cuda.synchronize()
            assert torch.equal(rows.view(torch.float32), gPV.view.abs().amax(1))
        else:
            att = _Guarded(B, H * 3 * D, H * 3 * D)
            guards["att"] = att
            call("mvml_token_attn_fold_fwd", B, H, D, ptr(PV), 2 * HD, ptr(Xn), D, sc, ptr(att.mat),
                 ptr(P.mat), st)
            call("mvml_conv3_fwd", B, 12, 12, D, ptr(att.mat), ptr(w), ptr(bias), ptr(out.mat), st)
            gatt = torch.empty(B, H, 3, D, device=DEV)
            wp, wn = ws_ptr_size(L.mvml_conv3_bwd_workspace_size(B), DEV)
            call("mvml_conv3_bwd", B, 12, 12, D, ptr(att.mat), ptr(w), ptr(out.mat), ptr(gout), ptr(gatt),
                 ptr(gw), ptr(gb), wp, wn, st)
            call("mvml_token_attn_fold_bwd", B, H, D, ptr(PV), 2 * HD, ptr(Xn), D, sc, ptr(P.mat),
                 ptr(gatt), ptr(gPV.mat), ldg, ptr(gk.mat), ldgk, ptr(amx), st)
        torch.cuda.synchronize()
        for name, gd in guards.items():
            gd.check(f"{name} (fused={fused})")
        res[fused] = dict(P=P.view.clone(), out=out.view.clone(), gPV=gPV.view.clone(), gk=gk.view.clone(),
                          amx=amx, gw=gw, gb=gb)
    diff = {k: (res[True][k].double() - res[False][k].double()).abs().max().item()
            for k in ("P", "out", "gPV", "gk", "amx")}
    assert all(v == 0 for v in diff.values()), diff
    assert res[True]["amx"].view(torch.float32).item() == res[True]["gPV"].abs().max().item()
    assert rel_err(res[True]["gw"], res[False]["gw"]) < 1e-5
    assert rel_err(res[True]["gb"], res[False]["gb"]) < 1e-5


def test_attn_conv_dropout_at_width(monkeypatch):
    """MVFusion(100, 12, 11, dropout=0.3) in train mode: the fused kernel's Dropout-in-the-store
    against the separate launches (in-place mvml_dropout_fwd) for the same seed — output and
    every gradient bit-identical (Conv2d weight / bias: another column-sum order, 1e-5) — and
    what test_attn_conv_dropout_gradient_is_masked_scaled asserts at 384: kept elements are the
    p = 0 output times 1 / (1 - p), and the gradients are those of p = 0 with the upstream
    gradient masked and scaled."""
    import mvml_gat.fusion as fu
    from mvml_gat import MVFusion
    from mvml_gat.fusion import FusionAttnConvFunction
    torch.manual_seed(0)
    B, D = 160, 100
    mod = MVFusion(D, 12, 11, dropout=0.3).to(DEV).train()
    ln = mod.norm_layer_module
    xs = [torch.randn(B, D, device=DEV) for _ in range(3)]
    args = (ln.weight, ln.bias, mod.linear_q.weight, mod.linear_k.weight, mod.linear_v.weight,
            mod.conv[0].weight, mod.conv[0].bias, ln.eps)

    def run(p, g, fused=True, seed=11):
        monkeypatch.setattr(fu, "FUSE_ATTN_CONV", fused)
        for t in mod.parameters():
            t.grad = None
        torch.manual_seed(seed)
        out = FusionAttnConvFunction.apply(*xs, *args, p)
        out.backward(g)
        return out.detach().clone(), {n: t.grad.clone() for n, t in mod.named_parameters() if t.grad is not None}

    g = torch.randn(B, 12 * (D - 2), device=DEV)
    out_p, grads_p = run(0.3, g)
    out_s, grads_s = run(0.3, g, fused=False)
    assert torch.equal(out_p, out_s)
    assert grads_p.keys() == grads_s.keys() and grads_p
    for n in grads_p:
        if n.startswith("conv."):
            assert rel_err(grads_p[n], grads_s[n]) < 1e-5, n
        else:
            assert torch.equal(grads_p[n], grads_s[n]), n
    out_0, _ = run(0.0, g)
    s = torch.tensor(1.0 / (1.0 - 0.3), dtype=torch.float32, device=DEV)
    kept = out_p != 0
    assert torch.equal(out_p[kept], out_0[kept] * s)
    assert torch.all(out_0[~kept] >= 0)
    pos = out_0 > 0
    frac = (kept & pos).sum().item() / pos.sum().item()
    assert abs(frac - 0.7) < 0.02, frac
    _, grads_ref = run(0.0, g * kept.float() * s)
    assert grads_p.keys() == grads_ref.keys()
    for n in grads_p:
        assert torch.equal(grads_p[n], grads_ref[n]), n


def test_fusion_width_deterministic_bitwise():
    _, mod, xs = _pair(33, seed=11, dim=100)
    outs = []
    for _ in range(2):
        xd = [x.float().to(DEV).requires_grad_(True) for x in xs]
        mod.zero_grad()
        z = mod(*xd)
        z.sum().backward()
        outs.append([z.detach().clone()] + [x.grad.clone() for x in xd] +
                    [p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
