"""The reverse-bond rule of D-MPNN (include/mvml_gat.h, tests/_dmpnn_ref.py) on the CPU: the reference's
map on the hand-written molecules and on three hand cases, against the expected pairs written out; and
the update kernel's contract (W_h applied first) against the model's statement in float64."""
import torch

import _afp_ref as A
import _dmpnn_ref as R
from conftest import rel_err


def test_reverse_map_on_the_hand_cases():
    assert R.rev_map([0, 1, 2], [0, 2, 1]) == [0, 2, 1]          # a self-loop is its own reverse
    assert R.rev_map([0, 0, 1, 1], [1, 1, 0, 0]) == [2, 3, 0, 1]  # a doubled bond pairs k-th with k-th
    assert R.rev_map([0, 0, 1], [1, 1, 0]) == [2, -1, 0]          # ... and the one left over has none
    assert R.rev_map([0], [1]) == [-1]                            # a one-way edge has none


def test_reverse_map_on_the_molecules():
    nn_, ne, src, dst = A.molecules()
    src, dst, _ = A.global_ids(nn_, ne, src, dst)
    rev = R.rev_map(src, dst)
    # bonds are listed forward then backward per molecule: without parallel bonds b-th pairs with b-th
    e0 = 0
    for i, n in enumerate(ne):
        if i != 3:
            assert rev[e0:e0 + n] == [e0 + n // 2 + b for b in range(n // 2)] + [e0 + b for b in range(n // 2)]
        e0 += n
    # the hub molecule (edges 14..173) has bond (0, 1) once and bond (1, 0) seven times: its first edge
    # 0 -> 1 is the forward edge of (0, 1), its first edge 1 -> 0 the forward edge of the first (1, 0)
    h0 = sum(ne[:3])
    assert [int(t) for t in (src[h0], dst[h0], src[h0 + 11], dst[h0 + 11])] == [9, 10, 10, 9] and rev[h0] == h0 + 11 and rev[h0 + 11] == h0
    assert -1 not in rev and all(int(src[r]) == int(dst[s]) and int(dst[r]) == int(src[s]) and rev[r] == s for s, r in enumerate(rev))


def test_update_from_R_equals_the_model_step():
    nn_, ne, src, dst = A.molecules()
    src, dst, _ = A.global_ids(nn_, ne, src, dst)
    N, E, D = sum(nn_), len(src), 8
    gen = torch.Generator().manual_seed(0)
    inp, M, W, b = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((E, D), (E, D), (D, D), (D,)))
    rev = R.rev_map(src, dst)
    rev[3] = -1  # (an edge treated as one-way)
    assert rel_err(R.update(src, dst, rev, N, inp, M @ W.T, b), R.step(src, dst, rev, N, inp, M, W, b)) <= 1e-12
