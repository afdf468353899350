"""What the GIN tests share beside the reference (tests/_gin_ref.py): the seeded categorical
features of the 170-atom `mixed` batch, weight-tied (product, float64 reference, float32 reference)
stacks, the sides protocol (ReLU sides and the max readout's argmax taken from one arithmetic and
given to the float64 reference, under check_sides' cap) and the choice of the weight seeds from the
reference alone.  No GPU is needed to import or run anything here but stack(..., device="cuda:0")."""
import torch
import torch.nn.functional as F

from _gcn_cases import mixed_batch, perturb_bn
from _gin_ref import GINPredictorRef, GINRef
from _util import graph_dict, randomize_
from conftest import rel_err
from mvml_gat import GIN, GINPredictor

NODE_TABLES, EDGE_TABLES = [13, 3], [6, 3]
KINDS = {"last": dict(JK="last", emb=64), "concat": dict(JK="concat", emb=64), "sum": dict(JK="sum", emb=64),
         "wide": dict(JK="last", emb=300), "pred_sum": dict(JK="last", emb=64, readout="sum"),
         "pred_mean": dict(JK="concat", emb=64, readout="mean"), "pred_max": dict(JK="sum", emb=64, readout="max")}
LAYERS, TASKS = 3, 11
# Weight seeds, decided from the reference alone (float32 against float64 on the CPU;
# tests/test_gin_cpu.py recomputes both conditions without a GPU):
#   STACK_SEEDS: the forward + backward test; the float64 reference run on the float32 one's sides
#                and argmax stays inside check_sides' cap (flips: the differing elements seen);
#   ADAM_SEEDS:  the three-Adam-step test; the same at every step, and adam_e32 <= 2.5e-6, so that
#                test's bar is the 1e-5 floor.
# Seen: 0 differing elements at every STACK seed; adam_e32 2.1e-7 / 5.7e-7 / 3.7e-7 / 2.5e-7.
STACK_SEEDS = {"last": 3, "concat": 3, "sum": 3, "wide": 3, "pred_sum": 3, "pred_mean": 3, "pred_max": 3}
ADAM_SEEDS = {"last": 12, "pred_sum": 40, "pred_mean": 16, "pred_max": 16}
# The optimiser of the three-step test.  The weight decay is large on purpose: mlp[2]'s bias feeds
# BatchNorm1d directly, which subtracts the batch mean, so the loss does not depend on it and its
# gradient is rounding noise alone (1e-8 in float32, 1e-17 in float64).  Adam divides a gradient by
# its own magnitude, so with the usual 1e-4 decay the float32 noise moves those biases by up to
# 1e-4 per step where the float64 run moves them by the decay term alone (adam_e32 1e-5 .. 3e-3 at
# every seed tried).  With decay 0.3 the decay term (0.3 |b|, about 1e-2) stands six orders above
# the noise and the update is a function of the parameters again.
ADAM = dict(lr=1e-3, weight_decay=0.3)


def categories(sb=None, seed=5):
    """(node categories, edge categories) of the batch: int64 CPU vectors, one per table."""
    sb = mixed_batch() if sb is None else sb
    gen = torch.Generator().manual_seed(seed)
    n, e = int(sb.num_nodes.sum()), int(sb.num_edges.sum())
    return ([torch.randint(0, s, (n,), generator=gen) for s in NODE_TABLES],
            [torch.randint(0, s, (e,), generator=gen) for s in EDGE_TABLES])


def is_predictor(kind):
    return kind.startswith("pred")


def stack(kind, seed=3, device="cpu", dropout=0.0):
    """(product on `device`, [float64 reference, float32 reference]), weight-tied: GIN(NODE_TABLES,
    EDGE_TABLES, num_layers=3, emb_dim, JK) or GINPredictor(..., readout, n_tasks=11)."""
    k = KINDS[kind]
    torch.manual_seed(seed)
    if is_predictor(kind):
        m = GINPredictor(NODE_TABLES, EDGE_TABLES, LAYERS, k["emb"], k["JK"], dropout, k["readout"], TASKS)
        mk = lambda: GINPredictorRef(NODE_TABLES, EDGE_TABLES, LAYERS, k["emb"], k["JK"], k["readout"], TASKS)
    else:
        m = GIN(NODE_TABLES, EDGE_TABLES, LAYERS, k["emb"], k["JK"], dropout)
        mk = lambda: GINRef(NODE_TABLES, EDGE_TABLES, LAYERS, k["emb"], k["JK"])
    randomize_(m, seed)
    perturb_bn(m, seed)
    refs = []
    for dt in (torch.float64, torch.float32):
        r = mk()
        r.load_state_dict({k_: v.detach().cpu() for k_, v in m.state_dict().items()}, strict=True)
        refs.append(r.to(dt))
    return m.to(device), refs


def out_shape(kind, sb):
    k = KINDS[kind]
    if is_predictor(kind):
        return (len(sb.num_nodes), TASKS)
    return (int(sb.num_nodes.sum()), k["emb"] * (LAYERS + 1 if k["JK"] == "concat" else 1))


def adam_labels(kind, sb):
    return (torch.rand(out_shape(kind, sb), generator=torch.Generator().manual_seed(8)) > 0.5).float()


def sides_of_record(record):
    """The sides a reference run took itself, in the layout its forward accepts."""
    outs = record["out"]
    return {"hidden": [t > 0 for t in record["hidden"]],
            "out": [(t > 0) if i < len(outs) - 1 else None for i, t in enumerate(outs)],  # the last layer has no ReLU
            "argmax": record["argmax"][0] if "argmax" in record else None}


def check_sides(record, sides):
    """The float64 reference's own ReLU sides and argmax (record) differ from the given ones in at
    most 2 elements per tensor; a differing ReLU side has a pre-activation within 1e-6 of the
    tensor's largest; at a differing argmax the two candidates' values are within 1e-6 of the
    tensor's largest value.  Returns the number of differing elements."""
    pairs = list(zip(record["hidden"], sides["hidden"])) + list(zip(record["out"], sides["out"]))
    total = 0
    for pre, side in pairs:
        if side is None:
            continue
        flips = (pre > 0) != side
        total += int(flips.sum())
        assert int(flips.sum()) <= 2, int(flips.sum())
        if flips.any():
            assert float(pre[flips].abs().max()) <= 1e-6 * float(pre.abs().max())
    if sides.get("argmax") is not None:
        own, h = record["argmax"]
        given = sides["argmax"].long()
        assert bool(((own < 0) == (given < 0)).all())
        diff = own != given
        total += int(diff.sum())
        assert int(diff.sum()) <= 2, int(diff.sum())
        if diff.any():
            v_own, v_giv = torch.gather(h, 0, own.clamp(min=0)), torch.gather(h, 0, given.clamp(min=0))
            assert float((v_own - v_giv)[diff].abs().max()) <= 1e-6 * float(h.abs().max())
    return total


def _inputs():
    sb = mixed_batch()
    return sb, graph_dict(sb), categories(sb)


def reference_flips(kind, seed):
    """Forward of the float32 reference on its own sides, then the float64 one on those sides under
    check_sides (raises outside the cap); the number of differing elements.  CPU only."""
    sb, gd, (nc, ec) = _inputs()
    _, (r64, r32) = stack(kind, seed)
    r32.train(), r64.train()
    rec32 = {}
    r32(gd, nc, ec, None, rec32)
    sides = sides_of_record(rec32)
    rec64 = {}
    r64(gd, nc, ec, sides, rec64)
    return check_sides(rec64, sides)


def adam_e32(kind, seed):
    """Worst rel_err over the state_dict of the float32 reference against the float64 one after
    three Adam steps at this weight seed; the float32 run takes its own sides, the float64 run is
    given them under check_sides, as the GPU test gives it the product's.  CPU only."""
    sb, gd, (nc, ec) = _inputs()
    _, (r64, r32) = stack(kind, seed)
    y = adam_labels(kind, sb)
    o64 = torch.optim.Adam(r64.parameters(), **ADAM)
    o32 = torch.optim.Adam(r32.parameters(), **ADAM)
    r64.train(), r32.train()
    for _ in range(3):
        o32.zero_grad()
        rec32 = {}
        F.binary_cross_entropy_with_logits(r32(gd, nc, ec, None, rec32), y).backward()
        o32.step()
        sides = sides_of_record(rec32)
        o64.zero_grad()
        rec64 = {}
        F.binary_cross_entropy_with_logits(r64(gd, nc, ec, sides, rec64), y.double()).backward()
        check_sides(rec64, sides)
        o64.step()
    s64, s32 = r64.state_dict(), r32.state_dict()
    return max(rel_err(s32[k], s64[k]) for k in s64 if not k.endswith("num_batches_tracked"))
