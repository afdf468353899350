"""NNConv's split-fp16 weight gradient (csrc/nnconv_wgrad.hip): mvml_nnconv_bwd_weight_f16x2 through the
C ABI against the float64 formulas of tests/_mpnn_ref.py, then MPNNPredictor(weight_grad="split_fp16").

Bar (the project's rule, as tests/test_gpu_mpnn.py): norm-wise rel_err <= max(1e-5, 4 e32), e32 the
same formulas in float32 on the CPU against their float64 run."""
import pytest
import torch

import _mpnn_ref as R
from conftest import rel_err
from mvml_gat import MPNNPredictor
from mvml_gat._lib import lib, ptr, stream_ptr
from test_gpu_mpnn import _batch, _predictor_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 40  # atoms; every fourth one has no in-edge


def _case(D, H, E, seed, g_scale=None):
    """Edge arrays in in-CSR slot order, NaN-padded pitched h, z, g on the device, and dW2 at float64 / float32."""
    gen = torch.Generator().manual_seed(seed)
    with_in = torch.tensor([v for v in range(N) if v % 4 != 3])
    dst = with_in[torch.randint(len(with_in), (E,), generator=gen)].sort().values
    src = torch.randint(N, (E,), generator=gen)
    h, z, g = (torch.randn(s, generator=gen) for s in ((N, D), (E, H), (N, D)))
    if g_scale is not None:
        g = g * g_scale[:, None]
    refs = [R.nnconv_grads_reassociated(src, dst, N, h.to(dt), z.to(dt), torch.zeros(D * D, H, dtype=dt), g.to(dt))[2]
            for dt in (torch.float64, torch.float32)]

    def pitched(x, pad):
        buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
        buf[:, :x.shape[1]] = x.to(DEV)
        return buf[:, :x.shape[1]]
    return (src.int().to(DEV), dst.int().to(DEV), pitched(h, 8), pitched(z, 4), pitched(g, 12)), refs


def _wgrad(D, H, E, dev, accumulate, dW2):
    src, dst, h, z, g = dev
    L, st = lib(), stream_ptr()
    img = torch.empty(L.mvml_nnconv_z_image_bytes(E, H), dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.mvml_nnconv_bwd_weight_f16x2_workspace_size(E, D, H), dtype=torch.uint8, device=DEV)
    assert img.numel() > 0 and ws.numel() > 0
    rc = L.mvml_nnconv_split_z(E, H, ptr(z), z.stride(0), ptr(img), st)
    rc = rc or L.mvml_nnconv_bwd_weight_f16x2(E, ptr(src), ptr(dst), ptr(h), h.stride(0), D, ptr(z), z.stride(0), H, ptr(g),
                                              g.stride(0), accumulate, ptr(dW2), ptr(ws), ws.numel(), st, ptr(img))
    torch.cuda.synchronize()
    assert rc == 0, L.mvml_last_error()
    return dW2


def _check(what, got, r64, r32):
    e, b = rel_err(got, r64), max(1e-5, 4 * rel_err(r32, r64))
    print(f"nnconv wgrad f16x2 {what}: {e:.2e} / {b:.2e}")
    assert bool(torch.isfinite(got).all()) and e <= b, (what, e, b)


# E: 21 is one partial chunk of 32.  The large one has more chunks than the launch wants ranges
# (min(64, ceil(256 / (D / IB))): 64, 43, 32, 4), so the ranges hold three chunks (the double buffer
# turns over), there are 44, 32, 22 and 4 of them, and the last chunk is partial (8, 24, 20, 12 edges).
@pytest.mark.parametrize("D,H,E_big", [(16, 16, 4200), (48, 80, 3000), (64, 128, 2100), (128, 256, 300)])
def test_weight_gradient_against_float64(D, H, E_big):
    for E in (21, E_big):
        assert E % 32
        dev, (r64, r32) = _case(D, H, E, 1000 * D + H + E)
        fresh = lambda: torch.full((D * D, H), float("nan"), device=DEV)
        got = _wgrad(D, H, E, dev, 0, fresh())
        _check(f"D={D} H={H} E={E}", got, r64, r32)
        assert torch.equal(got.view(torch.int32), _wgrad(D, H, E, dev, 0, fresh()).view(torch.int32))
        base = torch.randn(D * D, H, generator=torch.Generator().manual_seed(E))
        got = _wgrad(D, H, E, dev, 1, base.to(DEV))
        _check(f"D={D} H={H} E={E} accumulate", got, r64 + base.double(), r32 + base)
    # no edges: zeroed, or left alone when accumulating
    dev = tuple(x[:0] for x in dev[:2]) + (dev[2], dev[3][:0], dev[4])
    assert float(_wgrad(D, H, 0, dev, 0, fresh()).abs().max()) == 0.0
    assert torch.equal(_wgrad(D, H, 0, dev, 1, base.to(DEV)).cpu(), base)


def test_weight_gradient_over_a_wide_dynamic_range():
    """Whole molecules' g rows scaled by 2^-8 .. 2^8: what the global scales must survive."""
    D, H, E = 64, 128, 2100
    scale = 2.0 ** (torch.arange(N) * 17 // N - 8).float()
    assert scale.min() == 2.0 ** -8 and scale.max() == 2.0 ** 8
    dev, (r64, r32) = _case(D, H, E, 5, scale)
    _check("wide range", _wgrad(D, H, E, dev, 0, torch.empty((D * D, H), device=DEV)), r64, r32)


@pytest.mark.parametrize("D,H,steps,T,L", [(16, 16, 1, 2, 2), (64, 128, 3, 6, 3)])
def test_predictor_with_split_fp16_weight_gradient(D, H, steps, T, L):
    g, src, dst, gid, _, _ = _batch()
    torch.manual_seed(D + steps)
    kw = {} if L == 3 else dict(num_step_set2set=T, num_layer_set2set=L)
    model = MPNNPredictor(39, 10, node_out_feats=D, edge_hidden_feats=H, n_tasks=3, num_step_message_passing=steps,
                          weight_grad="split_fp16", **kw)
    _predictor_case(model, g, src, dst, gid, steps, T, L, f"predictor split_fp16 D={D} H={H} steps={steps}")
    with pytest.raises(ValueError, match="weight_grad"):
        MPNNPredictor(39, 10, node_out_feats=D, edge_hidden_feats=H, weight_grad="bf16")
