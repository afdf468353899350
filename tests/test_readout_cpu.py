"""The weighted-sum-and-max readout without a GPU: hand-derivable known answers on the float64
reference (tests/_readout_ref.py) and the module surface (state_dict keys, refused widths, the
GNNModule / MVP / train switches)."""
import pytest
import torch

from _readout_ref import wsum_max_ref


def test_ref_zero_gate_is_half_the_column_sums():
    X = torch.tensor([[1., 2., 3., 4.], [5., 6., 7., 8.], [-1., 0., 1., 2.]], dtype=torch.float64)
    out, am = wsum_max_ref([0, 2, 3], X, torch.zeros(1, 4, dtype=torch.float64),
                           torch.zeros(1, dtype=torch.float64))
    assert out.shape == (2, 8)
    assert torch.equal(out[0, :4], 0.5 * (X[0] + X[1]))  # gate sigmoid(0) = 0.5
    assert torch.equal(out[1, :4], 0.5 * X[2])
    assert torch.equal(out[0, 4:], X[1]) and torch.equal(out[1, 4:], X[2])
    assert am.tolist() == [[1] * 4, [2] * 4]


def test_ref_max_ties_go_to_the_lowest_atom():
    X = torch.tensor([[1., 5.], [3., 5.], [3., 2.]], dtype=torch.float64, requires_grad=True)
    W, b = torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    out, am = wsum_max_ref([0, 3], X, W, b)
    assert out[0, 2:].tolist() == [3., 5.]
    assert am.tolist() == [[1, 0]]
    out[0, 2:].sum().backward()  # the max half alone: exactly one 1 per column
    assert X.grad.tolist() == [[0., 1.], [1., 0.], [0., 0.]]


def test_ref_given_argmax_gathers_there():
    X = torch.tensor([[1., 5.], [3., 5.], [3., 2.]], dtype=torch.float64, requires_grad=True)
    W, b = torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    out, am = wsum_max_ref([0, 3], X, W, b, argmax=torch.tensor([[2, 1]]))
    assert out[0, 2:].tolist() == [3., 5.] and am.tolist() == [[2, 1]]
    out[0, 2:].sum().backward()
    assert X.grad.tolist() == [[0., 0.], [0., 1.], [1., 0.]]


def test_ref_molecule_without_atoms():
    X = torch.randn(3, 4, dtype=torch.float64, requires_grad=True)
    W = torch.randn(1, 4, dtype=torch.float64)
    b = torch.randn(1, dtype=torch.float64)
    out, am = wsum_max_ref([0, 0, 3, 3], X, W, b)
    assert out.shape == (3, 8)
    for g in (0, 2):
        assert bool((out[g] == 0).all()) and am[g].tolist() == [-1] * 4
    (g0,) = torch.autograd.grad(out[0].sum() + out[2].sum(), X, allow_unused=True)
    assert g0 is None or bool((g0 == 0).all())


def test_readout_modules_keys_and_shapes():
    from mvml_gat import WeightAndSum, WeightedSumAndMax
    m = WeightedSumAndMax(260)
    sd = m.state_dict()
    assert list(sd) == ["weight_and_sum.atom_weighting.0.weight", "weight_and_sum.atom_weighting.0.bias"]
    assert sd["weight_and_sum.atom_weighting.0.weight"].shape == (1, 260)
    assert sd["weight_and_sum.atom_weighting.0.bias"].shape == (1,)
    w = WeightAndSum(64)
    assert list(w.state_dict()) == ["atom_weighting.0.weight", "atom_weighting.0.bias"]
    assert isinstance(w.atom_weighting[0], torch.nn.Linear) and isinstance(w.atom_weighting[1], torch.nn.Sigmoid)


@pytest.mark.parametrize("D", [6, 1028, 0])
def test_readout_refuses_bad_width_at_construction(D):
    from mvml_gat import WeightAndSum, WeightedSumAndMax
    with pytest.raises(ValueError, match="multiple of 4"):
        WeightedSumAndMax(D)
    with pytest.raises(ValueError, match="multiple of 4"):
        WeightAndSum(D)


def test_gnn_module_readout_switch():
    from mvml_gat import GNNModule, Set2Set, WeightedSumAndMax
    default = GNNModule(74, [64, 64], 0.5, 6, 3)
    explicit = GNNModule(74, [64, 64], 0.5, 6, 3, readout="set2set")
    assert list(default.state_dict()) == list(explicit.state_dict())  # same keys, same order
    assert isinstance(default.readout, Set2Set)
    assert not any("weight_and_sum" in k for k in default.state_dict())
    ws = GNNModule(74, [64, 64], 0.5, readout="weighted_sum_max")
    assert isinstance(ws.readout, WeightedSumAndMax)
    keys = set(ws.state_dict())
    assert not any(k.startswith("readout.lstm.") for k in keys)
    new = {"readout.weight_and_sum.atom_weighting.0.weight", "readout.weight_and_sum.atom_weighting.0.bias"}
    assert new <= keys
    assert keys - new == {k for k in default.state_dict() if not k.startswith("readout.")}
    assert ws.state_dict()["readout.weight_and_sum.atom_weighting.0.weight"].shape == (1, 64)
    with pytest.raises(ValueError, match="readout"):
        GNNModule(74, [64, 64], 0.5, readout="x")


def test_mvp_and_train_pass_the_readout_through():
    from mvml_gat import MVP
    from mvml_gat import train
    # num_heads = 12: the only head count the fusion head takes
    m = MVP(11, 74, [64, 128], num_heads=12, graph_readout="weighted_sum_max")
    keys = set(m.state_dict())
    assert "gnn.readout.weight_and_sum.atom_weighting.0.weight" in keys
    assert "gnn.readout.weight_and_sum.atom_weighting.0.bias" in keys
    assert m.state_dict()["gnn.readout.weight_and_sum.atom_weighting.0.weight"].shape == (1, 128)
    assert not any(k.startswith("gnn.readout.lstm.") for k in keys)
    assert any(k.startswith("gnn.readout.lstm.") for k in MVP(11, 74, [64, 128], num_heads=12).state_dict())
    base = ["--data", "d.csv", "--index", "i.txt"]
    assert train.parse(base).graph_readout == "set2set"
    assert train.parse(base + ["--graph_readout", "weighted_sum_max"]).graph_readout == "weighted_sum_max"
    with pytest.raises(SystemExit):
        train.parse(base + ["--graph_readout", "x"])
