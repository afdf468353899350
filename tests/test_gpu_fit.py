"""The training driver (mvml_gat.train, main.py:18-61) on the GPU: the first 128 molecules of the
KEGG test split train, the next 64 validate, batch size 64 (config.py:21)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
LR0 = 1e-3


@pytest.fixture(scope="module")
def loaders():
    from torch.utils.data import DataLoader, Subset
    from mvml_gat.fingerprints import kegg_pool
    from mvml_gat.train import MVPDataSet, collate_mvp
    # kegg_pool(): fingerprints() of exactly these rows, stored (tests/test_fingerprints.py)
    ds = MVPDataSet(os.path.join(HERE, "golden", "kegg_test_split.csv"), fps=kegg_pool())
    train = DataLoader(Subset(ds, range(128)), batch_size=64, collate_fn=collate_mvp)
    val = DataLoader(Subset(ds, range(128, 192)), batch_size=64, collate_fn=collate_mvp)
    return train, val


def _model(seed=0):
    from mvml_gat.mvp import MVP
    torch.manual_seed(seed)
    return MVP(11, 74, [192, 384], 6, 3, 128, 384, 2, 512, 12, 0.5, device=DEV).to(DEV)


def test_train_step_with_meter_is_bitwise_the_step_without(loaders):
    """meter=None is the old path; a meter adds one kernel between the forward and the loss and
    changes nothing else: loss and every parameter bitwise equal after two steps (dropout on)."""
    from mvml_gat import FlatAdam, MultiLabelMeter
    from mvml_gat.mvp import train_step
    from mvml_gat.train import to_device
    batches = [to_device(b, DEV) for b in loaders[0]]
    assert len(batches) == 2
    runs = []
    for meter in (None, MultiLabelMeter(11, DEV)):
        model = _model(0).train()
        opt = FlatAdam(model.parameters(), lr=LR0, weight_decay=1e-4)
        torch.manual_seed(123)
        losses = [train_step(model, opt, b, meter=meter).detach().clone() for b in batches]
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in model.parameters()], meter))
    (l0, p0, _), (l1, p1, meter) = runs
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    r = meter.compute()
    assert r["n_batches"] == 2 and r["n_samples"] == 128 and 0.0 <= r["f1_score"] <= 1.0


def test_fit_two_epochs_checkpoint_reproduces_validation(loaders, tmp_path):
    from mvml_gat import FlatAdam, MultiLabelMeter
    from mvml_gat.train import EarlyStopping, evaluate_loader, fit
    train, val = loaders
    model = _model(1)
    opt = FlatAdam(model.parameters(), lr=LR0, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
    stopper = EarlyStopping(mode='higher', patience=15, filename=str(tmp_path / "net_0.pkl"))
    lines = []
    history = fit(model, opt, sched, stopper, train, val, 2, DEV, log=lines.append)
    assert len(history) == 2 and len(lines) == 2
    for e, h in enumerate(history):
        assert h["epoch"] == e and np.isfinite(h["loss"]) and h["loss"] > 0
        for phase, rows, nb in (("train", 128, 2), ("val", 64, 1)):
            assert h[phase]["n_samples"] == rows and h[phase]["n_batches"] == nb
            for k in ("acc", "precision", "recall", "f1_score"):
                assert np.isfinite(h[phase][k]) and 0.0 <= h[phase][k] <= 1.0, (e, phase, k)
    # ExponentialLR: one multiplication by gamma per epoch
    assert history[0]["lr"] == LR0 and history[1]["lr"] == LR0 * 0.95
    assert opt.param_groups[0]["lr"] == LR0 * 0.95 * 0.95
    assert history[0]["saved"] and stopper.timestep == 2
    best = [h for h in history if h["saved"]][-1]
    assert stopper.best_score == best["val"]["f1_score"] == max(h["val"]["f1_score"] for h in history)

    fresh = _model(7)
    ckpt = torch.load(stopper.filename, map_location="cpu")
    assert list(ckpt) == ["model_state_dict"]
    assert list(ckpt["model_state_dict"].keys()) == list(fresh.state_dict().keys())
    stopper.load_checkpoint(fresh)
    again = evaluate_loader(fresh, val, MultiLabelMeter(11, DEV))
    assert again == best["val"]  # eval mode is deterministic: the recorded metrics, exactly
