"""The fusion head's supported sizes, checked without a GPU: MVFusion / MVP construct at any
hidden_feats[-1] that is a multiple of 4 in [16, 384] with the oracle's state_dict layout, and
refuse every other width and every num_heads != 12 with a message that names the set."""
import pytest
import torch

SUPPORTED = "16 <= hidden_feats[-1] <= 384"
# the ends, and every 64-column group boundary of the kernels with the width just above it
ACCEPTED = [16, 68, 128, 132, 196, 256, 260, 320, 324, 384]


@pytest.mark.parametrize("D", ACCEPTED)
def test_mvfusion_constructs_with_oracle_layout(D):
    from mvml_gat import MVFusion
    from oracle.fusion_ref import MVFusionRef
    torch.manual_seed(D)
    mod, ref = MVFusion(D, 12, 11), MVFusionRef(D, 12, 11)
    sd, rd = mod.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys())
    for k in sd:
        assert sd[k].shape == rd[k].shape, k
    mod.load_state_dict(rd, strict=True)
    for k, v in mod.state_dict().items():
        assert torch.equal(v, rd[k]), k
    assert mod.mlp[0].in_features == 12 * (D - 2) and mod.linear_q.out_features == 12 * D


@pytest.mark.parametrize("D", ACCEPTED)
def test_mvp_constructs_with_oracle_layout(D):
    from mvml_gat.mvp import MVP
    from oracle.fusion_ref import MVPRef
    torch.manual_seed(D)
    mod = MVP(11, 74, [64, D], 6, 3, 32, 48, 2, 64, num_heads=12, dropout=0.5)
    ref = MVPRef(hidden_feats=(64, D), rnn_embed_dim=32, blstm_dim=48, fp_2_dim=64)
    sd, rd = mod.state_dict(), ref.state_dict()
    assert sorted(sd.keys()) == sorted(rd.keys())
    for k in sd:
        assert sd[k].shape == rd[k].shape, k
    mod.load_state_dict(rd, strict=True)


def test_mvp_at_the_readme_example_sizes():
    from mvml_gat.mvp import MVP
    from oracle.fusion_ref import MVPRef
    mod = MVP(11, 74, [64, 128], 6, 3, 128, 96, 2, 128, num_heads=12)
    ref = MVPRef(hidden_feats=(64, 128), blstm_dim=96, fp_2_dim=128)
    mod.load_state_dict(ref.state_dict(), strict=True)
    assert mod.final_hidden_feats == 128


@pytest.mark.parametrize("D", [8, 18, 388, 512])
def test_mvfusion_refuses_unsupported_width(D):
    from mvml_gat import MVFusion
    with pytest.raises(ValueError) as e:
        MVFusion(D, 12, 11)
    assert SUPPORTED in str(e.value) and "multiple of 4" in str(e.value) and str(D) in str(e.value)


@pytest.mark.parametrize("heads", [4, 8])
def test_mvfusion_refuses_other_head_counts(heads):
    from mvml_gat import MVFusion
    from mvml_gat.mvp import MVP
    with pytest.raises(ValueError) as e:
        MVFusion(128, heads, 11)
    msg = str(e.value)
    assert SUPPORTED in msg and "Conv2d(12, 12" in msg and "12" in msg
    with pytest.raises(ValueError):
        MVP(11, 74, [64, 128], num_heads=heads)


def test_train_cli_sizes_are_accepted():
    from mvml_gat.mvp import MVP
    from mvml_gat.train import parse
    a = parse(["--data", "x", "--index", "y", "--hidden_feats", "64", "128"])
    assert a.hidden_feats == [64, 128] and a.head == 12
    mod = MVP(num_classes=a.class_num, in_feats=74, hidden_feats=a.hidden_feats,
              rnn_embed_dim=a.rnn_embed_dim, blstm_dim=a.rnn_hidden_dim, blstm_layers=a.rnn_layers,
              fp_2_dim=a.fp_dim, dropout=a.p, num_heads=a.head)
    assert mod.final_hidden_feats == 128
    assert mod.linear_q.weight.shape == (12 * 128, 128)
    b = parse(["--data", "x", "--index", "y", "--hidden_feats", "64", "128", "--rnn_hidden_dim", "96",
               "--fp_dim", "128"])
    MVP(num_classes=b.class_num, in_feats=74, hidden_feats=b.hidden_feats, rnn_embed_dim=b.rnn_embed_dim,
        blstm_dim=b.rnn_hidden_dim, blstm_layers=b.rnn_layers, fp_2_dim=b.fp_dim, dropout=b.p,
        num_heads=b.head)
