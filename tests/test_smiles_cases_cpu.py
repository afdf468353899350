"""Conditions on the INPUTS and RESTATEMENTS of test_gpu_smiles_shapes.py (no GPU): the length
catalogue has the batch-size profiles its names promise, and every numpy restatement in
_smiles_cases.py is pinned to torch (pack_padded_sequence, the oracle's select-last indexing,
nn.Embedding's float64 gradient) and to the product's own host-side Packing."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import _smiles_cases as C


def test_catalogue_profiles():
    bs = {n: C.packed_order(C.lengths(n))[2] for n in C.NAMES}
    assert bs["one"] == [1] and bs["single7"] == [1] * 7
    assert bs["eq16"] == [16] * 6 and bs["eq17"] == [17] * 3
    assert bs["stair17"] == list(range(17, 0, -1))  # crosses the 16-row block edge one row a step
    assert bs["cliff33"] == [33, 16, 1]
    assert bs["blocks48"] == [48, 32, 32, 16, 16]
    for name, B in (("b512", C.SEQ_MAX_B), ("b513", C.SEQ_MAX_B + 1)):
        lens = C.lengths(name)
        assert len(lens) == B and sorted(set(lens)) == [1, 2, 3, 4, 5, 6]
    for name, B, T in (("r5x9", 5, 9), ("r140x12", 140, 12)):
        lens = C.lengths(name)
        assert len(lens) == B and min(lens) == 1 and max(lens) == T and len(set(lens)) > 2
    assert C.STEP_ROWS == 16
    for name in ("eq16", "cliff33", "blocks48"):  # a step with exactly one / two / three full blocks
        assert any(b % C.STEP_ROWS == 0 for b in bs[name])
    for name in ("eq17", "stair17", "cliff33"):   # and one row past a block edge
        assert any(b % C.STEP_ROWS == 1 for b in bs[name])


@pytest.mark.parametrize("name", C.NAMES)
def test_catalogue_is_shuffled(name):
    lens = C.lengths(name)
    perm, pos, _, _ = C.packed_order(lens)
    assert sorted(perm.tolist()) == list(range(len(lens)))
    assert np.array_equal(perm[pos], np.arange(len(lens)))
    if len(set(lens)) > 1:
        assert not np.array_equal(perm, np.arange(len(lens))), "perm is the identity"
        assert not np.array_equal(pos, np.arange(len(lens)))


@pytest.mark.parametrize("name", C.NAMES)
def test_packed_order_matches_torch_and_product(name):
    from mvml_gat.smiles import Packing
    lens = C.lengths(name)
    B, T = len(lens), max(lens)
    perm, pos, batch_sizes, offsets = C.packed_order(lens)
    ident = (1000 * torch.arange(B)[:, None] + torch.arange(T)[None, :]).double()[:, :, None]
    ref = pack_padded_sequence(ident, lens, batch_first=True, enforce_sorted=False)
    assert ref.batch_sizes.tolist() == batch_sizes
    assert offsets.tolist() == [0] + np.cumsum(batch_sizes).tolist()
    data = ref.data[:, 0].long()
    lens_a = np.asarray(lens)
    for t, bs in enumerate(batch_sizes):
        rows = data[offsets[t]:offsets[t + 1]]
        assert (rows % 1000 == t).all()
        b_torch = (rows // 1000).numpy()
        # the same sequences alive, the same length at every packed row; inside a run of equal
        # lengths torch's order is only required to be a permutation (its sort need not be stable)
        assert sorted(b_torch.tolist()) == sorted(perm[:bs].tolist())
        assert np.array_equal(lens_a[b_torch], lens_a[perm[:bs]])
    si = ref.sorted_indices.numpy()
    assert sorted(si.tolist()) == list(range(B)) and np.array_equal(lens_a[si], lens_a[perm])
    assert (np.diff(lens_a[perm]) <= 0).all()
    # the product's host-side metadata is this restatement
    pk = Packing(lens, torch.zeros((B, T)), 39)
    assert pk.batch_sizes == batch_sizes
    assert pk.perm.tolist() == perm.tolist() and pk.pos.tolist() == pos.tolist()
    for key in ((0, T), (1, T), (0, T - 1)):
        if key[1] > key[0]:
            o, n = pk.live_offsets(*key)
            assert n == sum(batch_sizes[key[0]:key[1]])
            assert o.tolist() == [0] + np.cumsum(batch_sizes[key[0]:key[1]]).tolist()


@pytest.mark.parametrize("name", ["single7", "stair17", "cliff33", "b513"])
def test_gather_and_packed_tokens_match_torch(name):
    lens = C.lengths(name)
    B, T = len(lens), max(lens)
    perm, pos, batch_sizes, _ = C.packed_order(lens)
    tok = C.tokens_for(lens, 39, 3, ldtok=T + 2)
    assert tok.max() == 38 and (tok[np.arange(T + 2)[None, :] >= np.asarray(lens)[:, None]] == 0).all()
    table = np.random.default_rng(0).standard_normal((39, 8)).astype(np.float32)
    got = C.gather_rows_ref(table, tok, lens, perm, T).reshape(T, B, 8)
    x = torch.from_numpy(table)[torch.from_numpy(tok[:, :T]).long()]
    padded, _ = pad_packed_sequence(pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False))
    assert np.array_equal(got, padded[:, torch.from_numpy(perm)].numpy())
    # sorted input: torch's packed order has no ties to break differently
    ref = pack_padded_sequence(torch.from_numpy(tok[perm][:, :T]), np.asarray(lens)[perm].tolist(),
                               batch_first=True, enforce_sorted=True)
    assert np.array_equal(C.packed_tokens_ref(tok, perm, batch_sizes), ref.data.numpy())
    m = C.live_mask(lens)
    assert m.sum() == sum(lens) and np.array_equal(m, (got != 0).any(axis=2))


@pytest.mark.parametrize("name", ["one", "stair17", "cliff33"])
def test_select_last_matches_oracle_indexing(name):
    lens = C.lengths(name)
    B, T, H = len(lens), max(lens), 3
    perm, pos, _, _ = C.packed_order(lens)
    output = torch.randn(B, T, 2 * H, dtype=torch.float64, requires_grad=True)  # batch_first, original order
    out_forward = output[range(len(output)), np.array(lens) - 1, :H]   # oracle/smiles_ref.py
    out_reverse = output[:, 0, H:]
    want = torch.cat((out_forward, out_reverse), 1)
    out_tm = output.detach().numpy().transpose(1, 0, 2)[:, perm]       # time-major, sorted rows
    assert np.array_equal(C.select_last_gather(out_tm, lens, pos), want.detach().numpy())
    # the scatter is the gather's adjoint
    fea = torch.randn(B, 2 * H, dtype=torch.float64)
    (want * fea).sum().backward()
    g = C.select_last_scatter(np.zeros((T, B, 2 * H)), fea.numpy(), lens, pos)
    assert np.array_equal(g, output.grad.numpy().transpose(1, 0, 2)[:, perm])
    # ... and writes nothing else
    s = C.select_last_scatter(np.full((T, B, 2 * H), -7.0), fea.numpy(), lens, pos)
    assert (s != -7.0).sum() == B * 2 * H


@pytest.mark.parametrize("name", ["single7", "stair17", "cliff33", "blocks48"])
def test_pack_then_unpack_is_identity_on_live_rows(name):
    lens = C.lengths(name)
    B, T = len(lens), max(lens)
    _, _, batch_sizes, _ = C.packed_order(lens)
    live = C.live_mask(lens)
    tm = np.random.default_rng(1).standard_normal((T, B, 4))
    packed = C.pack_rows_ref(tm, batch_sizes, 0, T, 0)
    assert packed.shape == (sum(lens), 4) and np.array_equal(packed, tm[live])
    back = C.unpack_rows_ref(np.full_like(tm, -7.0), packed, batch_sizes, 0, T, 0)
    assert np.array_equal(back[live], tm[live]) and (back[~live] == -7.0).all()
    if T > 1:  # the shifted ranges pair step t with t - 1 (from step 1) and t + 1 (to step T - 1)
        prev = C.pack_rows_ref(tm, batch_sizes, 1, T, -1)
        nxt = C.pack_rows_ref(tm, batch_sizes, 0, T - 1, 1)
        assert prev.shape[0] == sum(batch_sizes[1:]) and nxt.shape[0] == sum(batch_sizes[:-1])
        assert np.array_equal(prev[:batch_sizes[1]], tm[0, :batch_sizes[1]])
        assert np.array_equal(nxt[:batch_sizes[0]], tm[1, :batch_sizes[0]])


@pytest.mark.parametrize("vocab", [39, 64])
def test_token_sums_match_embedding_gradient(vocab):
    lens = C.lengths("stair17")
    perm, _, batch_sizes, _ = C.packed_order(lens)
    tok = C.packed_tokens_ref(C.tokens_for(lens, vocab, 5), perm, batch_sizes)
    tok[tok == 5] = 6  # a token that never occurs: its sum is an exact zero
    g =np.random.default_rng(2).standard_normal((tok.size, 6))
    s, a, n = C.token_sums(g, tok, vocab)
    emb = torch.nn.Embedding(vocab, 6).double()
    (emb(torch.from_numpy(tok).long()) * torch.from_numpy(g)).sum().backward()
    assert np.allclose(s, emb.weight.grad.numpy(), rtol=0, atol=1e-13)
    assert n.sum() == tok.size and np.array_equal(n, np.bincount(tok, minlength=vocab))
    assert (a >= np.abs(s) - 1e-13).all() and (s[n == 0] == 0).all() and (n == 0).any()
    bound = C.token_sum_bound(a, n)
    assert bound.shape == s.shape and (bound[n == 0] == 0).all()


def test_expected_entries_rules():
    assert C.expected_entries(512, 384, "f16x2") == C.SEQ_ENTRIES
    assert C.expected_entries(513, 384, "f16x2") == C.WIDE_ENTRIES
    assert C.expected_entries(1, 384, "f16x2", seq_max_b=0) == C.WIDE_ENTRIES
    assert C.expected_entries(5, 392, "f16x2") == C.WIDE_ENTRIES
    assert C.expected_entries(5, 8, "f16x2") == C.WIDE_ENTRIES
    assert C.expected_entries(5, 8, "x3") == C.CELL_ENTRIES
    assert C.expected_entries(5, 72, "f16x2", wide_step=False) == C.CELL_ENTRIES
    for H in (100, 36, 30):
        assert C.expected_entries(300, H, "f16x2", seq_max_b=0) == C.CELL_ENTRIES
