"""What the GCN tests share beside the reference (tests/_gcn_ref.py): the batch, weight-tied
(product, float64 reference, float32 reference) stacks, and the choice of the Adam test's weight
seeds from the reference alone.  No GPU is needed to import or run anything here but
stack(..., device="cuda:0")."""
import torch
import torch.nn.functional as F

from _gcn_ref import GCNPredictorRef, GCNRef
from _util import batch_of_sizes, graph_dict, randomize_
from conftest import rel_err
from mvml_gat import GCN, GCNPredictor

# Weight seeds of the three-Adam-step test: adam_e32(kind, seed) <= 2.5e-6 (at seed 3: 7e-5 / 1e-5)
ADAM_SEEDS = {"gcn": 4, "predictor": 5}


def mixed_batch():
    """The 170-atom `mixed` batch (tests/test_gpu_agg_shapes.py GRAPHS, restated for the CPU tests;
    tests/test_gpu_gcn.py asserts that the two are the same)."""
    return batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1)


def features(sb, width, seed=0):
    if width == 74:
        return torch.as_tensor(sb.feats, dtype=torch.float32)
    return torch.randn((int(sb.num_nodes.sum()), width), generator=torch.Generator().manual_seed(seed))


def perturb_bn(model, seed):
    """BatchNorm's weight and buffers off their initial 1 / 0 / 1."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
                m.running_mean.add_(0.1 * torch.randn(m.weight.shape, generator=gen))
                m.running_var.add_(0.3 * torch.rand(m.weight.shape, generator=gen))
    return model


def stack(kind, seed=3, device="cpu"):
    """(product on `device`, [float64 reference, float32 reference]) of kind "gcn": GCN(74, [64, 64])
    or "predictor": GCNPredictor(74, [64, 20], n_tasks=11), weight-tied."""
    torch.manual_seed(seed)
    if kind == "gcn":
        m = GCN(74, [64, 64], gnn_norm=["both", "none"])
        mk = lambda: GCNRef(74, [64, 64], ["both", "none"])
    else:
        m = GCNPredictor(74, [64, 20], gnn_norm=["both", "right"], n_tasks=11, predictor_hidden_feats=32)
        mk = lambda: GCNPredictorRef(74, [64, 20], ["both", "right"], predictor_hidden_feats=32, n_tasks=11)
    randomize_(m, seed)
    perturb_bn(m, seed)
    refs = []
    for dt in (torch.float64, torch.float32):
        r = mk()
        r.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
        refs.append(r.to(dt))
    return m.to(device), refs


def adam_labels(kind, sb):
    shape = (int(sb.num_nodes.sum()), 64) if kind == "gcn" else (len(sb.num_nodes), 11)
    return (torch.rand(shape, generator=torch.Generator().manual_seed(8)) > 0.5).float()


def adam_e32(kind, seed):
    """Worst rel_err over the state_dict of the float32 reference against the float64 one after
    three Adam steps at this weight seed, each on its own ReLU sides; CPU only."""
    sb = mixed_batch()
    gd, X = graph_dict(sb), features(sb, 74)
    _, refs = stack(kind, seed)
    y = adam_labels(kind, sb)
    for ref, dt in zip(refs, (torch.float64, torch.float32)):
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-4)
        ref.train()
        for _ in range(3):
            opt.zero_grad()
            F.binary_cross_entropy_with_logits(ref(gd, X.to(dt)), y.to(dt)).backward()
            opt.step()
    s64, s32 = refs[0].state_dict(), refs[1].state_dict()
    return max(rel_err(s32[k], s64[k]) for k in s64 if not k.endswith("num_batches_tracked"))
