"""mvml_nnconv_bwd_weight_f16x2's refusals and the z image's size, without a GPU: every refusal comes
before any launch, so the pointers are never followed."""
import pytest

from mvml_gat._lib import lib

P = 0x10000  # a 16-byte aligned address that is never dereferenced


def _call(D=64, H=128, E=100, dW2=P, image=P, ws_short=0):
    L = lib()
    need = L.mvml_nnconv_bwd_weight_f16x2_workspace_size(E, 64, 128)
    return L.mvml_nnconv_bwd_weight_f16x2(E, P, P, P, D, D, P, H, H, P, D, 0, dW2, P, need - ws_short, None, image)


@pytest.mark.parametrize("kw,rc", [(dict(D=20), 1), (dict(H=272), 1), (dict(dW2=P + 4), 1), (dict(image=None), 1),
                                   (dict(ws_short=1), 3)])
def test_refused_before_any_launch(kw, rc):
    assert _call(**kw) == rc and b"nnconv_bwd_weight_f16x2" in lib().mvml_last_error()


def test_z_image_bytes():
    L = lib()
    assert L.mvml_nnconv_z_image_bytes(100, 272) == 0 and L.mvml_nnconv_z_image_bytes(100, 20) == 0
    assert L.mvml_nnconv_z_image_bytes(-1, 128) == 0
    head = L.mvml_nnconv_z_image_bytes(0, 128)
    assert [L.mvml_nnconv_z_image_bytes(E, 128) - head for E in (1, 32, 33, 64)] == [c * 32 * 4 * 128 for c in (1, 1, 2, 2)]
