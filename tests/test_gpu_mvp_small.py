"""The whole MVP model at a non-default configuration — hidden_feats [32, 64], rnn_embed_dim 32,
blstm_dim 48, fp_2_dim 64 — where the three views meet the fusion head at width 64 instead of
384: one training step against the composed float64 oracle MVPRef on the 64-molecule KEGG batch
of test_gpu_mvp.py (that file's method and bars), then a two-epoch fit as test_gpu_fit.py runs
at the default sizes.

Bars: logits / loss within 1e-5 of float64; every parameter gradient within 1e-5 or 4x the fp32
oracle's own error; after one Adam step the parameters within 1e-5."""
import os

import numpy as np
import pytest
import torch

from _util import randomize_
from conftest import rel_err
from test_gpu_mvp import _kegg_batch
from test_gpu_parity_configs import _branches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = dict(hidden_feats=(32, 64), rnn_embed_dim=32, blstm_dim=48, fp_2_dim=64)


def _mvp(device="cpu"):
    from mvml_gat.mvp import MVP
    return MVP(11, 74, [32, 64], 6, 3, 32, 48, 2, 64, 12, 0.5, device=device)


def _models(seed=0):
    from oracle.fusion_ref import MVPRef
    torch.manual_seed(seed)
    mod = _mvp()
    randomize_(mod.gnn, seed)
    with torch.no_grad():
        mod.norm_layer_module.weight.uniform_(0.5, 1.5)
    ref64 = MVPRef(**SIZES).double().eval()
    ref64.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    ref32 = MVPRef(**SIZES).eval()
    ref32.load_state_dict(mod.state_dict())
    return mod.to(DEV).eval(), ref64, ref32


def test_mvp_small_train_step_parity():
    from mvml_gat import bce_with_logits
    from mvml_gat import functional as Fn
    from oracle.fusion_ref import bce_logits_ref
    bg, gd, x, smiles, fp, y = _kegg_batch()
    mod, ref64, ref32 = _models()
    g = bg.to(DEV)
    sm_d = {"smiles": smiles["smiles"].to(DEV), "seq_len": smiles["seq_len"]}
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad()
    cap = {}
    Fn.DEBUG_CAPTURE = cap
    try:
        z_d = mod(sm_d, g, g.ndata["h"].to(DEV), fp.float().to(DEV))
    finally:
        Fn.DEBUG_CAPTURE = None
    assert z_d.shape == (64, 11)
    br = _branches(gd, [e.cpu() for e in cap["elr_fwd"]])
    conv = (cap["conv_out"] > 0).unsqueeze(2).cpu()
    mlp = (cap["relu_out"][-1] > 0).cpu()
    assert conv.shape == (64, 12, 1, 62)
    loss_d = bce_with_logits(z_d, y.float().to(DEV))
    loss_d.backward()

    z_r = ref64(smiles, gd, x, fp, branches=br, conv_branch=conv, mlp_branch=mlp)
    loss_r = bce_logits_ref(z_r, y)
    loss_r.backward()
    loss_32 = bce_logits_ref(ref32({"smiles": smiles["smiles"], "seq_len": smiles["seq_len"]}, gd,
                                   x.float(), fp.float(), branches=br, conv_branch=conv,
                                   mlp_branch=mlp), y.float())
    loss_32.backward()
    print(f"MVP [32, 64]: logits {rel_err(z_d, z_r):.2e}, loss {loss_d.item():.6f} vs {loss_r.item():.6f}")
    assert rel_err(z_d, z_r) < TOL
    assert abs(loss_d.item() - loss_r.item()) / abs(loss_r.item()) < TOL
    p64, p32 = dict(ref64.named_parameters()), dict(ref32.named_parameters())
    worst = (0.0, None)
    for n, p in mod.named_parameters():
        if p64[n].grad is None:  # unused LayerNorms (model.py:39, 120): no gradient anywhere
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        e = rel_err(p.grad, p64[n].grad)
        budget = max(TOL, 4 * rel_err(p32[n].grad, p64[n].grad))
        worst = max(worst, (e / budget, n))
        assert e < budget, (n, e, budget)
    print(f"MVP [32, 64]: worst grad err/budget {worst[0]:.2f} ({worst[1]})")
    opt_r = torch.optim.Adam(ref64.parameters(), lr=1e-3, weight_decay=1e-4)
    with torch.no_grad():
        for n, p in mod.named_parameters():  # same gradients on both sides: compare the update
            if p.grad is not None and p64[n].grad is not None:
                p64[n].grad.copy_(p.grad.double().cpu())
    opt.step()
    opt_r.step()
    for n, p in mod.named_parameters():
        assert rel_err(p, p64[n]) < TOL, n


def test_mvp_small_fit_two_epochs_and_checkpoint(tmp_path):
    """48 molecules train, 16 validate, batch size 16: the driver runs, the losses are finite and
    the checkpoint round-trips through EarlyStopping.load_checkpoint."""
    from torch.utils.data import DataLoader, Subset
    from mvml_gat import FlatAdam, MultiLabelMeter
    from mvml_gat.fingerprints import kegg_pool
    from mvml_gat.train import EarlyStopping, MVPDataSet, collate_mvp, evaluate_loader, fit
    ds = MVPDataSet(os.path.join(HERE, "golden", "kegg_test_split.csv"), fps=kegg_pool())
    train = DataLoader(Subset(ds, range(48)), batch_size=16, collate_fn=collate_mvp)
    val = DataLoader(Subset(ds, range(48, 64)), batch_size=16, collate_fn=collate_mvp)
    torch.manual_seed(1)
    model = _mvp(DEV).to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
    stopper = EarlyStopping(mode='higher', patience=15, filename=str(tmp_path / "net_0.pkl"))
    history = fit(model, opt, sched, stopper, train, val, 2, DEV, log=None)
    assert len(history) == 2
    for e, h in enumerate(history):
        assert h["epoch"] == e and np.isfinite(h["loss"]) and h["loss"] > 0
        assert h["train"]["n_samples"] == 48 and h["val"]["n_samples"] == 16
    assert history[0]["saved"]
    best = [h for h in history if h["saved"]][-1]
    torch.manual_seed(7)
    fresh = _mvp(DEV).to(DEV)
    ckpt = torch.load(stopper.filename, map_location="cpu")
    assert list(ckpt["model_state_dict"].keys()) == list(fresh.state_dict().keys())
    assert ckpt["model_state_dict"]["linear_q.weight"].shape == (12 * 64, 64)
    stopper.load_checkpoint(fresh)
    again = evaluate_loader(fresh, val, MultiLabelMeter(11, DEV))
    assert again == best["val"]  # eval mode is deterministic: the recorded metrics, exactly
