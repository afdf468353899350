"""WeaveGather without a GPU: state_dict layout, the constructor's refusals, the refusals of
mvml_weave_gather_* / mvml_tanh_* before any launch, and the reference's own closed-form cases."""
import ctypes

import pytest
import torch
import torch.nn as nn

import _weave_ref as R
import mvml_gat
from mvml_gat import WeaveGather, _lib
from mvml_gat import functional as Fn

INVALID = 1
P = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before a launch


def test_state_dict_and_exports():
    m = WeaveGather(128)
    want = {**{f"means.{k}": () for k in range(11)}, **{f"stds.{k}": () for k in range(11)},
            "to_out.weight": (128, 11 * 128), "to_out.bias": (128,)}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert [float(p) for p in m.means] == pytest.approx([mu for mu, _ in Fn.WEAVE_MEMBERSHIPS])
    assert not any(p.requires_grad for p in (*m.means, *m.stds))
    assert WeaveGather(128, gaussian_expand=False).state_dict() == {}
    assert WeaveGather(8, gaussian_memberships=[(0., 1.), (1., 2.)], activation=None).to_out.in_features == 16
    assert "WeaveGather" in mvml_gat.__all__
    for name in ("mvml_weave_gather_fwd", "mvml_weave_gather_bwd", "mvml_tanh_fwd", "mvml_tanh_bwd"):
        assert name in _lib.parse_header() and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("kw, match", [
    (dict(node_in_feats=6), "multiple of 4"), (dict(node_in_feats=1028), "multiple of 4"),
    (dict(node_in_feats=6, gaussian_expand=False), "multiple of 4"),
    (dict(node_in_feats=8, gaussian_memberships=[(0., 0.)]), "std > 0"),
    (dict(node_in_feats=8, gaussian_memberships=[(0., -1.)]), "std > 0"),
    (dict(node_in_feats=8, gaussian_memberships=[(float("nan"), 1.)]), "finite mean"),
    (dict(node_in_feats=8, gaussian_memberships=[(0.1 * k, 1.) for k in range(17)]), "1 to 16"),
    (dict(node_in_feats=8, gaussian_memberships=[]), "1 to 16"),
    (dict(node_in_feats=8, activation=nn.ReLU()), "Tanh"), (dict(node_in_feats=8, activation=torch.tanh), "Tanh")])
def test_constructor_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        WeaveGather(**kw)


@pytest.mark.parametrize("kw", [dict(F=6), dict(F=0), dict(F=1028), dict(K=0), dict(K=17), dict(stds=[0.1, 0.0]),
                                dict(stds=[0.1, 1e-30]), dict(means=[0.0, float("inf")]), dict(B=-1), dict(N=2 ** 31),
                                dict(ldx=4), dict(ldx=10), dict(ldo=12), dict(null="means"), dict(null="offsets")])
def test_entry_points_refuse_before_any_launch(kw):
    L = _lib.lib()
    F, K, B, N = kw.get("F", 8), kw.get("K", 2), kw.get("B", 3), kw.get("N", 5)
    mu = (ctypes.c_float * 17)(*(kw.get("means", [0.0, 1.0]) + [0.0] * 15))
    sd = (ctypes.c_float * 17)(*(kw.get("stds", [0.5, 0.5]) + [1.0] * 15))
    mu = None if kw.get("null") == "means" else mu
    off = None if kw.get("null") == "offsets" else P
    ldx, ldo = kw.get("ldx", F), kw.get("ldo", F * K)
    for rc in (L.mvml_weave_gather_fwd(B, N, F, K, mu, sd, off, P, ldx, P, ldo, None),
               L.mvml_weave_gather_bwd(B, N, F, K, mu, sd, off, P, ldx, P, ldo, P, ldx, None)):
        assert rc == INVALID and b"weave_gather" in L.mvml_last_error()
    assert L.mvml_tanh_fwd(-1, P, P, None) == L.mvml_tanh_fwd(4, None, P, None) == INVALID
    assert L.mvml_tanh_bwd(-1, P, P, P, None) == L.mvml_tanh_bwd(4, P, None, P, None) == INVALID


def test_reference_closed_forms():
    """One membership: p = 1, so the readout counts the atoms; K equal memberships: p = 1 / K."""
    x = torch.linspace(-3, 3, 28, dtype=torch.float64).view(7, 4)
    gid = torch.tensor([0, 0, 0, 2, 2, 2, 2])
    one = R.sum_nodes(R.histogram(x, [0.3], [0.2]), gid, 3)
    assert torch.equal(one, torch.tensor([3., 0., 4.], dtype=torch.float64)[:, None].expand(3, 4))
    same = R.histogram(x, [0.3] * 5, [0.2] * 5)
    assert same.shape == (7, 20) and torch.allclose(same, torch.full_like(same, 0.2), rtol=0, atol=1e-15)
