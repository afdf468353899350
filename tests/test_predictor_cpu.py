"""GATPredictor / GATv2Predictor / MLPPredictor and the BatchNorm1d entry points without a GPU:
the header and the library agree on the new symbols, every refusal of mvml_batchnorm1d_* returns
before a launch, the stripe rule, the modules' state_dict layout against the reference
composition (tests/_predictor_ref.py), gnn_out_feats, dgllife's classifier_* override rule, the
constructors' refusals, and no CPU fallback."""
import ctypes

import pytest
import torch

import mvml_gat
from _predictor_ref import MLPPredictorRef, PredictorRef
from mvml_gat import GATPredictor, GATv2Predictor, MLPPredictor, _lib
from mvml_gat import functional as Fn

INVALID, WORKSPACE = 1, 3
NEW = ["mvml_batchnorm1d_part_rows", "mvml_batchnorm1d_workspace_size", "mvml_batchnorm1d_fwd",
       "mvml_batchnorm1d_bwd"]
P = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before a launch


def test_header_and_library_agree_on_the_new_symbols():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in NEW:
        assert name in protos and hasattr(L, name), name
    assert [n for n in protos if "batchnorm1d" in n] == NEW  # the exact list, in the header's order
    assert protos["mvml_batchnorm1d_part_rows"] == (ctypes.c_int64, [ctypes.c_int64])
    assert protos["mvml_batchnorm1d_workspace_size"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    assert len(protos["mvml_batchnorm1d_fwd"][1]) == 19 and len(protos["mvml_batchnorm1d_bwd"][1]) == 17


def _fwd(M=8, C=4, ldx=None, ldy=None, training=1, momentum=0.1, eps=1e-5, ws=None):
    L = _lib.lib()
    ws = L.mvml_batchnorm1d_workspace_size(M, C) if ws is None else ws
    rc = L.mvml_batchnorm1d_fwd(M, C, P, C if ldx is None else ldx, P, P, training, momentum, eps, P, P, P, P,
                                C if ldy is None else ldy, P, P, P, ws, None)
    return rc, L.mvml_last_error().decode()


def _bwd(M=8, C=4, ldx=None, ldgy=None, ldgx=None, training=1, ws=None, gx=P):
    L = _lib.lib()
    ws = L.mvml_batchnorm1d_workspace_size(M, C) if ws is None else ws
    rc = L.mvml_batchnorm1d_bwd(M, C, P, C if ldx is None else ldx, P, training, P, P, P,
                                C if ldgy is None else ldgy, gx, C if ldgx is None else ldgx, P, P, P, ws, None)
    return rc, L.mvml_last_error().decode()


@pytest.mark.parametrize("fn, kw, status", [
    (_fwd, dict(M=0), INVALID), (_fwd, dict(C=0), INVALID), (_fwd, dict(M=-3), INVALID),
    (_fwd, dict(C=8, ldx=7), INVALID), (_fwd, dict(C=8, ldy=4), INVALID),
    (_fwd, dict(M=1), INVALID), (_fwd, dict(eps=-1e-9), INVALID),
    (_fwd, dict(momentum=-0.01), INVALID), (_fwd, dict(momentum=1.5), INVALID),
    (_fwd, dict(ws=255), WORKSPACE), (_fwd, dict(M=4099, C=130, ws=2 * 65 * 130 * 8 - 1), WORKSPACE),
    (_bwd, dict(M=0), INVALID), (_bwd, dict(C=0), INVALID),
    (_bwd, dict(C=8, ldx=7), INVALID), (_bwd, dict(C=8, ldgy=7), INVALID), (_bwd, dict(C=8, ldgx=7), INVALID),
    (_bwd, dict(M=1), INVALID), (_bwd, dict(ws=0), WORKSPACE), (_bwd, dict(training=0, ws=100), WORKSPACE),
])
def test_refusals_before_any_launch(fn, kw, status):
    rc, msg = fn(**kw)
    assert rc == status, (rc, msg)
    assert "batchnorm1d" in msg


def test_part_rows_rule():
    L = _lib.lib()
    R = L.mvml_batchnorm1d_part_rows
    assert R(1) == 1 and R(0) == 0
    ms = list(range(1, 300)) + [4095, 4096, 4097, 4099, 65535, 65536, 65537, 10 ** 6, 1_750_000, 2 ** 31 + 5]
    rs = [R(m) for m in ms]
    assert all(a <= b for a, b in zip(rs, rs[1:]))  # monotone in M
    assert all(1 <= r <= min(m, 1024) for m, r in zip(ms, rs))
    assert R(64) == 1 and R(65) == 2 and R(4099) == 65  # 64 full stripes of 64 rows and a ragged one of 3
    assert R(1_750_000) == 1024
    W = L.mvml_batchnorm1d_workspace_size
    assert W(65536, 128) >= 2 * 1024 * 128 * 8 + 2 * 128 * 8
    assert W(1_750_000, 768) < 16 * 2 ** 20  # tall inputs stay small


MLP_KEYS = ["predict.1.weight", "predict.1.bias", "predict.3.weight", "predict.3.bias", "predict.3.running_mean",
            "predict.3.running_var", "predict.3.num_batches_tracked", "predict.4.weight", "predict.4.bias"]


def _layout(sd):
    return [(k, tuple(v.shape), v.dtype) for k, v in sd.items()]


def test_mlp_predictor_state_dict():
    m = MLPPredictor(24, 20, 3, 0.25)
    assert list(m.state_dict()) == MLP_KEYS
    assert _layout(m.state_dict()) == _layout(MLPPredictorRef(24, 20, 3, 0.25).state_dict())
    assert isinstance(m.predict[0], torch.nn.Dropout) and m.predict[0].p == 0.25
    assert isinstance(m.predict[3], torch.nn.BatchNorm1d) and m.predict[3].momentum == 0.1
    MLPPredictorRef(24, 20, 3).load_state_dict(m.state_dict(), strict=True)


@pytest.mark.parametrize("kind", ["gat", "gatv2"])
@pytest.mark.parametrize("modes", [None, ["flatten", "flatten"]])
def test_predictor_state_dict_equals_the_reference_compositions(kind, modes):
    if kind == "gat":
        m = GATPredictor(74, [8, 12], [2, 4], agg_modes=modes)
    else:
        m = GATv2Predictor(74, [8, 12], [2, 4], agg_modes=modes)
    ref = PredictorRef(kind, 74, [8, 12], [2, 4], agg_modes=modes)
    assert _layout(m.state_dict()) == _layout(ref.state_dict())
    assert list(m.state_dict())[-9:] == ["predict." + k for k in MLP_KEYS]
    ref.load_state_dict(m.state_dict(), strict=True)
    want = 48 if modes else 12  # flatten: hidden * heads; mean: hidden
    assert m.gnn_out_feats == want == ref.gnn_out_feats
    assert m.readout.weight_and_sum.in_feats == want
    assert m.predict.predict[1].in_features == 2 * want
    assert m.predict.predict[1].out_features == 128 and m.predict.predict[4].out_features == 1  # dgllife's defaults


def test_classifier_arguments_override_only_default_predictor_arguments():
    def hd(**kw):
        m = GATPredictor(74, [8], [2], **kw)
        return m.predict.predict[1].out_features, m.predict.predict[0].p

    assert hd() == (128, 0.0)
    assert hd(classifier_hidden_feats=64, classifier_dropout=0.3) == (64, 0.3)
    assert hd(predictor_hidden_feats=32, predictor_dropout=0.2) == (32, 0.2)
    assert hd(classifier_hidden_feats=64, predictor_hidden_feats=32) == (32, 0.0)
    assert hd(classifier_dropout=0.3, predictor_dropout=0.2) == (128, 0.2)
    assert hd(classifier_hidden_feats=64, predictor_dropout=0.2) == (64, 0.2)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="WeightAndSum"):
        GATPredictor(74, [8, 1028], [2, 1], agg_modes=["flatten", "flatten"])  # readout width 1028
    with pytest.raises(ValueError, match="WeightAndSum"):
        GATv2Predictor(74, [8, 1028], [2, 1])  # the same width from a head-mean last layer
    GATPredictor(74, [8, 256], [2, 4], agg_modes=["flatten", "flatten"])  # 1024: the widest
    with pytest.raises(NotImplementedError, match="feat_drop"):
        GATPredictor(74, [8, 12], [2, 4], feat_drops=[0.1, 0.1])
    with pytest.raises(NotImplementedError, match="feat_drop"):
        GATv2Predictor(74, [8, 12], [2, 4], attn_drops=[0.1, 0.0])
    with pytest.raises(ValueError):
        MLPPredictor(8, 8, 1, dropout=1.0)


def test_momentum_none_is_refused():
    m = MLPPredictor(8, 8, 1)
    m.predict[3].momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        m(torch.zeros(4, 8))
    with pytest.raises(ValueError, match="momentum=None"):
        Fn.batch_norm1d(torch.zeros(4, 8), torch.nn.BatchNorm1d(8, momentum=None))


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MLPPredictor(8, 8, 1)(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.batch_norm1d(torch.zeros(4, 8), torch.nn.BatchNorm1d(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.dropout(torch.ones(8), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.DropoutFunction.apply(torch.ones(8), 0.5)
    with pytest.raises(ValueError, match="< 1"):
        Fn.dropout(torch.ones(8), 1.0)
    sb_model = GATPredictor(74, [8, 12], [2, 4])
    with pytest.raises(TypeError, match="BatchedMolGraph"):
        sb_model(None, torch.zeros(3, 74))
    assert "GATPredictor" in mvml_gat.__all__ and "GATv2Predictor" in mvml_gat.__all__


def test_gpu_test_weight_seeds_follow_the_conditioning_rule():
    """tests/test_gpu_predictor.py takes, per model, the first weight seed at which the float64
    reference is well enough conditioned (its docstring); the choice is recomputed here from the
    reference alone."""
    import test_gpu_predictor as T
    for name, seed in T.SEEDS.items():
        assert T.pick_seed(name) == seed, name
        ratio, amp = T.conditioning(name, seed)
        assert ratio <= 32 and amp <= 1024
