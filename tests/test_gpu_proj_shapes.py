"""mvml_gat_proj_fwd (the projection GEMM with GATConv's attention logits in its epilogue) at the
ABI, at every partial width of the epilogue: the logits are per-W-column partial dots of the fp32 Z
tile, W = the largest power of two <= 32 dividing F (common.h proj_logw), summed per head in fixed
order by gat_logits_finalize_kernel<H>.  F = 4 / 24 / 48 / 96 give W = 4 / 8 / 16 / 32; the head
counts 1 / 2 / 4 / 8 and both residual layouts ride along.  Y and [el | er] against float64, on
the fp32-MFMA and the split-bf16 (x3) kernels, 1e-5 norm-wise (BASELINE.json north_star)."""
import pytest
import torch

from conftest import rel_err
from mvml_gat._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
ALGO = {"f32": 0, "x3": 1}  # MVML_GEMM_F32 / MVML_GEMM_F32X3


@pytest.mark.parametrize("algo", list(ALGO))
@pytest.mark.parametrize("H,F,mean", [(4, 4, 0), (1, 4, 1), (2, 24, 1), (4, 24, 0), (4, 48, 0), (8, 48, 1),
                                      (8, 96, 0), (4, 96, 1)])
def test_proj_fwd_logit_epilogue(H, F, mean, algo):
    L = lib()
    N, K = 301, 76  # more than one 128- / 256-row tile, rows not a multiple of 4
    HF = H * F
    C = L.mvml_gat_proj_cols(H, F, mean)
    assert C == HF + (F if mean else HF)
    gen = torch.Generator().manual_seed(100 * H + F + mean)
    X = torch.randn((N, K), generator=gen)
    W = torch.randn((C, K), generator=gen) / K ** 0.5
    attn = torch.randn((2, HF), generator=gen)
    ldy = C + 4
    Y = torch.full((N, ldy), -7777.0, device=DEV)
    elr = torch.full((N, 2 * H), -7777.0, device=DEV)
    wsz = L.mvml_gat_proj_fwd_workspace_size(N, H, F)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    dX, dW, dA = X.to(DEV), W.to(DEV), attn.to(DEV)
    call("mvml_gat_proj_fwd", N, ptr(dX), K, K, ptr(dW), K, ptr(dA), H, F, mean, ALGO[algo], ptr(Y), ldy,
         ptr(elr), None, None, None, 0, ptr(ws), wsz, stream_ptr())
    torch.cuda.synchronize()
    Y64 = X.double() @ W.double().t()
    Z = Y64[:, :HF].view(N, H, F)
    a = attn.double().view(2, H, F)
    elr64 = torch.cat([(Z * a[0]).sum(-1), (Z * a[1]).sum(-1)], 1)
    e_y, e_l = rel_err(Y[:, :C], Y64), rel_err(elr, elr64)
    print(f"PROJ H={H} F={F} mean={mean} {algo}: Y {e_y / TOL:.3f} elr {e_l / TOL:.3f} of the budget")
    assert e_y < TOL and e_l < TOL, (e_y, e_l)
    assert bool((Y[:, C:] == -7777.0).all()), "columns past C written"
