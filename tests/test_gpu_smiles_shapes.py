"""The SMILES BiLSTM kernels (csrc/smiles_lstm.hip, the wide-step entry points of
csrc/gemm_f32.hip, mvml_gat/smiles.py) at every recurrence path, hidden size and row edge,
against float64 (oracle.smiles_ref.RNNModuleRef, torch's nn.LSTM) and the numpy restatements of
_smiles_cases.py (pinned to torch in test_smiles_cases_cpu.py).

Which recurrence runs, and what each case pins:

* fused step kernels (mvml_bilstm_seq_fwd / _bwd: B <= 512 and H = 384).  A block owns 16 rows
  of a step; it clamps rows past B, skips blocks past the step's batch size, and relies on the
  zeroed out / c / gg / carry for rows that come alive or die between steps.  ``eq16`` is one
  full block, ``eq17`` one row into the second; ``stair17`` loses one row per step across the
  block edge; ``cliff33`` drops 33 -> 16 -> 1 live rows (three blocks, one full block, one row);
  ``blocks48`` retires a whole block at a time; ``one`` / ``single7`` are B = 1 at T = 1 and 7;
  ``b512`` is the widest batch the path takes.
* wide step (mvml_bilstm_wide_fwd / _bwd: every other shape with H % 8 == 0 on the split-fp16
  GEMM): one dual launch per step.  ``b513`` takes it by the default dispatch; the H = 384
  cases force it (SEQ_MAX_B = 0) down to M = 1 row, to T = 1 (only the K = 0 first-step launch;
  a backward with no recurrent product, R = 0) and over the cliff, on the planned 128x128 tile
  and on the 256x256 one (option lstm_tile).  Hidden sizes: H = 8 (K = 8 is no multiple of the
  32-deep k tile: W_hh is not pre-split; the gate matrix is 32 columns, narrower than a tile;
  the backward's split-K chunk rounds up to all of K = 32, so its second half is empty and
  the cell-backward kernel still adds both slabs), 40 (K % 32 != 0, second half short: 64 of
  96 + 64), 72 (ragged last column tile: 288 = 2 x 128 + 32), 128 (aligned), 200 (K % 32 != 0,
  800 columns), 392 (one 8-column step past 384: K % 32 != 0, ragged column tile), each at 5
  rows and at 140 (two row tiles), two layers (the second layer's packed input projection).
  H = 72 also runs the per-step GEMM + cell kernels and the two mixed packings.
* per-step GEMM + cell kernels (mvml_lstm_cell_fwd / _bwd): H % 8 != 0, WIDE_STEP off, or
  another GEMM algorithm.

Every parity case asserts, through a spy on mvml_gat.smiles.call, that exactly the entry points
its path names ran — the expectation comes from the documented rules
(_smiles_cases.expected_entries), not from the product's predicates.

One layer with a dense upstream gradient: BiLSTMLayerFunction against nn.LSTM on the whole
[T, B, 2H] output with a gradient on every live position (the module-level cases feed the last
layer two non-zero positions per sequence), g_x and all eight weight gradients; out and g_x are
exactly 0.0 at padded positions.

Index kernels through the C ABI: destinations pre-filled with a sentinel (nothing outside the
documented rows and columns may change), data movement bitwise equal to the restatement; the
token gradients twice (bitwise equal runs) and within the bound of sequential fp32 summation,
n_v 2^-24 sum|g| over a token's n_v rows.

Bars: 1e-5 norm-wise (conftest.rel_err) on the output and every gradient, the project's flat
bar.  torch's own float32 nn.LSTM on the CPU, on these very batches and weights, stays at or
below 9.1e-7 against the same float64 reference (worst: H = 392, 140 rows,
rnn.weight_ih_l1_reverse; the catalogue entries at H = 384: 8.1e-7), so the bar leaves a
factor of ten over what fp32 arithmetic itself loses here."""
import json
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import _smiles_cases as C
from conftest import rel_err
from mvml_gat._lib import MvmlError, call, lib, option, ptr, stream_ptr
from test_gpu_smiles import _rnn_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SENT = -7.0
RECURRENCE = set(C.SEQ_ENTRIES + C.WIDE_ENTRIES + C.CELL_ENTRIES)
WORST = {}  # family -> (error, case, tensor)


@pytest.fixture(scope="module", autouse=True)
def _margins():
    """Worst error per family: printed, and written to MVML_MARGINS_DIR where that is set."""
    yield
    print({k: f"{v[0]:.2e} {v[1]} {v[2]}" for k, v in WORST.items()})
    out = os.environ.get("MVML_MARGINS_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bilstm_shapes.json"), "w") as f:
        json.dump({k: {"error": v[0], "case": v[1], "tensor": v[2]} for k, v in WORST.items()}, f, indent=1)


def _note(family, case, errs):
    name = max(errs, key=errs.get)
    print(f"{family} {case}: worst {name} {errs[name]:.2e}")
    if family not in WORST or errs[name] > WORST[family][0]:
        WORST[family] = (errs[name], case, name)


def _spy(monkeypatch):
    """Record the name of every entry point mvml_gat.smiles calls."""
    import mvml_gat.smiles as sm
    names, real = [], sm.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(sm, "call", spy)
    return names


def _ran(names):
    return {n for n in names if n in RECURRENCE}


def _parity(monkeypatch, family, lens_name, layers, H=384, E=128, seq_max_b=None, wide_step=None,
            wide_pack=None, tile=0):
    """RNNModule against RNNModuleRef on the catalogue entry, and the recurrence that ran."""
    import mvml_gat.smiles as sm
    from mvml_gat import functional as Fn
    if seq_max_b is not None:
        monkeypatch.setattr(sm, "SEQ_MAX_B", seq_max_b)
    if wide_step is not None:
        monkeypatch.setattr(sm, "WIDE_STEP", wide_step)
    if wide_pack is not None:
        monkeypatch.setattr(sm, "WIDE_PACK", wide_pack)
    lens = C.lengths(lens_name)
    want = C.expected_entries(len(lens), H, Fn.GEMM_ALGO, C.SEQ_MAX_B if seq_max_b is None else seq_max_b,
                              True if wide_step is None else wide_step)
    names = _spy(monkeypatch)
    with option("lstm_tile", tile):
        errs = _rnn_parity(len(lens), max(lens), layers, True, False, H=H, lens=lens, E=E)
    assert _ran(names) == set(want), (sorted(_ran(names)), want)
    _note(family, f"{lens_name} L={layers} H={H} tile={tile}", errs)
    return want


# ------------------------------------------------------------------ module parity: fused path
@pytest.mark.parametrize("lens_name,layers", [
    ("one", 1), ("single7", 1), ("eq16", 1), ("eq17", 1), ("stair17", 1), ("cliff33", 1),
    ("blocks48", 1), ("cliff33", 2), ("stair17", 2), ("b512", 1)])
def test_fused_path_row_edges(lens_name, layers, monkeypatch):
    assert _parity(monkeypatch, "fused", lens_name, layers) == C.SEQ_ENTRIES


# ------------------------------------------------------------------ module parity: wide, H = 384
def test_wide_path_default_dispatch_b513(monkeypatch):
    """One row past SEQ_MAX_B: the wide step by the product's own dispatch (no monkeypatch)."""
    _parity(monkeypatch, "wide384", "b513", 1)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("lens_name", ["one", "single7", "eq17", "cliff33"])
def test_wide_path_few_rows(lens_name, layers, monkeypatch):
    _parity(monkeypatch, "wide384", lens_name, layers, seq_max_b=0)


@pytest.mark.parametrize("lens_name", ["one", "cliff33"])
def test_wide_path_few_rows_tile256(lens_name, monkeypatch):
    _parity(monkeypatch, "wide384", lens_name, 1, seq_max_b=0, tile=256)


# ------------------------------------------------------------------ module parity: hidden sizes
@pytest.mark.parametrize("lens_name", ["r5x9", "r140x12"])
@pytest.mark.parametrize("H", [8, 40, 72, 128, 200, 392])
def test_wide_step_hidden_sizes(H, lens_name, monkeypatch):
    _parity(monkeypatch, "wideH", lens_name, 2, H=H)


@pytest.mark.parametrize("lens_name", ["r5x9", "r140x12"])
@pytest.mark.parametrize("H", [8, 72, 392])
def test_wide_step_hidden_sizes_tile256(H, lens_name, monkeypatch):
    _parity(monkeypatch, "wideH", lens_name, 2, H=H, tile=256)


@pytest.mark.parametrize("lens_name", ["r5x9", "r140x12"])
@pytest.mark.parametrize("wide_step,wide_pack", [(False, False), (True, False), (False, True)])
def test_hidden_72_other_paths(wide_step, wide_pack, lens_name, monkeypatch):
    """H = 72 on the per-step GEMM + cell kernels (over all T x B rows), and the two mixed
    settings: the wide step over time-major projections, packed products around the cell path."""
    want = _parity(monkeypatch, "wideH", lens_name, 2, H=72, wide_step=wide_step, wide_pack=wide_pack)
    assert wide_step or want == C.CELL_ENTRIES


@pytest.mark.parametrize("H", [100, 36, 30])
def test_other_hidden_sizes_take_cell_path(H, monkeypatch):
    """test_gpu_smiles.test_rnn_module_parity_hidden_sizes' cases, with the path they name."""
    import mvml_gat.smiles as sm
    monkeypatch.setattr(sm, "SEQ_MAX_B", 0)
    names = _spy(monkeypatch)
    _rnn_parity(300, 20, 2, True, False, H=H)
    assert _ran(names) == set(C.CELL_ENTRIES)


# ------------------------------------------------------------------ one layer, dense gradient
W_NAMES = [f"{n}_l0{sfx}" for sfx in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


@pytest.mark.parametrize("lens_name,H,seq_max_b", [("cliff33", 384, None), ("cliff33", 384, 0),
                                                   ("r140x12", 72, None)])
def test_layer_dense_gradient(lens_name, H, seq_max_b, monkeypatch):
    import mvml_gat.smiles as sm
    from mvml_gat import functional as Fn
    from mvml_gat.smiles import BiLSTMLayerFunction, Packing
    if seq_max_b is not None:
        monkeypatch.setattr(sm, "SEQ_MAX_B", seq_max_b)
    lens = C.lengths(lens_name)
    B, T, In = len(lens), max(lens), 2 * H
    perm = C.packed_order(lens)[0]
    live = torch.from_numpy(C.live_mask(lens))[:, :, None]
    torch.manual_seed(H + B)
    ref = torch.nn.LSTM(In, H, 1, bidirectional=True).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.float().double())  # float32-representable: both sides get the same numbers
    gen = torch.Generator().manual_seed(B)
    x32 = 0.5 * torch.randn((T, B, In), generator=gen) * live  # zeros at padded rows: the contract
    up32 = torch.randn((T, B, 2 * H), generator=gen) * live
    xr = x32.double().requires_grad_()
    packed = pack_padded_sequence(xr, np.asarray(lens)[perm].tolist(), enforce_sorted=True)
    out_r, _ = pad_packed_sequence(ref(packed)[0], total_length=T)
    (out_r * up32.double()).sum().backward()

    pk = Packing(lens, torch.zeros((B, T), device=DEV), 39)
    w = [getattr(ref, n).detach().float().to(DEV).requires_grad_() for n in W_NAMES]
    x = x32.to(DEV).requires_grad_()
    names = _spy(monkeypatch)
    out = BiLSTMLayerFunction.apply(x, pk, False, *w)
    out.backward(up32.to(DEV))
    want = C.expected_entries(B, H, Fn.GEMM_ALGO, C.SEQ_MAX_B if seq_max_b is None else seq_max_b)
    assert _ran(names) == set(want), (sorted(_ran(names)), want)

    dead = ~live.expand(T, B, 2 * H).to(DEV)
    assert out.shape == (T, B, 2 * H) and x.grad.shape == (T, B, In)
    assert bool((out.detach()[dead] == 0.0).all()), "out is not exactly zero at padded positions"
    assert bool((x.grad[~live.expand(T, B, In).to(DEV)] == 0.0).all()), "g_x is not exactly zero at padded positions"
    errs = {"out": rel_err(out.detach(), out_r.detach()), "g_x": rel_err(x.grad, xr.grad)}
    for n, p in zip(W_NAMES, w):
        errs[n] = rel_err(p.grad, getattr(ref, n).grad)
    _note("layer", f"{lens_name} H={H} {want[0]}", errs)
    for n, e in errs.items():
        assert e < TOL, (n, e)


# ------------------------------------------------------------------ index kernels
def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _same_bits(got, want):
    """Bitwise equality of a float32 device tensor and a float32 numpy array."""
    want = np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def _meta(lens):
    perm, pos, batch_sizes, offsets = C.packed_order(lens)
    return perm, pos, batch_sizes, offsets, _dev(np.asarray(lens), torch.int32), _dev(perm, torch.int32), \
        _dev(pos, torch.int32)


@pytest.mark.parametrize("T,B,cols,ldtok", [(1, 1, 4, 1), (7, 5, 120, 9), (6, 33, 1536, 6)])
def test_gather_rows(T, B, cols, ldtok):
    lens = C.ragged_lengths(B, T, T + B)
    perm, _, _, _, d_lens, d_perm, _ = _meta(lens)
    tok = C.tokens_for(lens, 39, cols, T=T, ldtok=ldtok)
    table = np.random.default_rng(cols).standard_normal((39, cols)).astype(np.float32)
    out = torch.full((T * B + 2, cols), SENT, device=DEV)
    d_table, d_tok = _dev(table), _dev(tok)  # named: alive until the kernel has run
    call("mvml_bilstm_gather_rows", T, B, cols, ptr(d_table), ptr(d_tok), ldtok, ptr(d_lens),
         ptr(d_perm), ptr(out), stream_ptr())
    want = C.gather_rows_ref(table, tok, lens, perm, T)
    assert _same_bits(out[:T * B], want)
    assert bool((out[T * B:] == SENT).all())
    if B > 1:  # padded rows are written, as zeros
        assert (~want.any(axis=1)).sum() == T * B - sum(lens) > 0


@pytest.mark.parametrize("lens_name", ["one", "stair17"])
@pytest.mark.parametrize("H", [1, 5, 384])
def test_select_last(H, lens_name):
    lens = C.lengths(lens_name)
    B, T = len(lens), max(lens)
    assert 1 in lens and T in lens
    _, pos, _, _, d_lens, _, d_pos = _meta(lens)
    rng = np.random.default_rng(H)
    out = rng.standard_normal((T, B, 2 * H)).astype(np.float32)
    d_out = _dev(out)
    fea = torch.full((B + 1, 2 * H), SENT, device=DEV)
    call("mvml_bilstm_select_last", B, H, ptr(d_lens), ptr(d_pos), ptr(d_out), ptr(fea), 0, stream_ptr())
    assert _same_bits(fea[:B], C.select_last_gather(out, lens, pos))
    assert bool((fea[B:] == SENT).all()) and _same_bits(d_out, out)
    # dir 1: the scatter changes those B 2H elements and nothing else
    g_fea = rng.standard_normal((B, 2 * H)).astype(np.float32)
    d_fea = _dev(g_fea)
    g_out = torch.full((T * B + 1, 2 * H), SENT, device=DEV)
    call("mvml_bilstm_select_last", B, H, ptr(d_lens), ptr(d_pos), ptr(g_out), ptr(d_fea), 1, stream_ptr())
    want = np.full((T * B + 1, 2 * H), SENT, dtype=np.float32)
    C.select_last_scatter(want[:T * B].reshape(T, B, 2 * H), g_fea, lens, pos)
    assert _same_bits(g_out, want) and _same_bits(d_fea, g_fea)


@pytest.mark.parametrize("cols", [4, 260, 1536])
@pytest.mark.parametrize("B", [1, 3, 5, 700])
def test_pack_rows(B, cols):
    """Pack (dir 0) and unpack (dir 1) of a pitched source as the product passes it: one
    direction's half of a [T, B, 2 cols] buffer (ld = 2 cols, pointer at column d cols), over all
    steps and over the two shifted ranges of the W_hh gradient."""
    lens = C.ragged_lengths(B, 4 if B == 1 else 5, B)
    T = max(lens)
    batch_sizes = C.packed_order(lens)[2]
    rng = np.random.default_rng(B + cols)
    tm = rng.standard_normal((T, B, 2 * cols)).astype(np.float32)
    d_tm = _dev(tm)
    for d in (0, 1):
        half = slice(d * cols, (d + 1) * cols)
        for t0, t1, shift in ((0, T, 0), (1, T, -1), (0, T - 1, 1)):
            offs = np.concatenate([[0], np.cumsum(batch_sizes[t0:t1])]).astype(np.int32)
            n = int(offs[-1])
            d_offs = _dev(offs)
            packed = torch.full((n + 1, cols), SENT, device=DEV)
            call("mvml_bilstm_pack_rows", n, t1 - t0, B, cols, ptr(d_offs), t0, shift, ptr(d_tm[0, 0, half]),
                 2 * cols, ptr(packed), cols, 0, stream_ptr())
            want = C.pack_rows_ref(tm[:, :, half], batch_sizes, t0, t1, shift)
            assert want.shape == (n, cols)
            assert _same_bits(packed[:n], want), (d, t0, t1, shift)
            assert bool((packed[n:] == SENT).all()) and _same_bits(d_tm, tm)
            src = rng.standard_normal((n, cols)).astype(np.float32)
            d_src = _dev(src)
            d_back = torch.full((T, B, 2 * cols), SENT, device=DEV)
            call("mvml_bilstm_pack_rows", n, t1 - t0, B, cols, ptr(d_offs), t0, shift, ptr(d_back[0, 0, half]),
                 2 * cols, ptr(d_src), cols, 1, stream_ptr())
            back = np.full((T, B, 2 * cols), SENT, dtype=np.float32)
            C.unpack_rows_ref(back[:, :, half], src, batch_sizes, t0, t1, shift)
            assert _same_bits(d_back, back), (d, t0, t1, shift)


@pytest.mark.parametrize("B,T", [(5, 1), (700, 25)])
def test_packed_tokens(B, T):
    lens = C.ragged_lengths(B, T, B + T)
    perm, _, batch_sizes, offsets, _, d_perm, _ = _meta(lens)
    ldtok = T + 3
    tok = C.tokens_for(lens, 39, B, T=T, ldtok=ldtok)
    n = int(offsets[-1])
    out = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    d_offs, d_tok = _dev(offsets, torch.int32), _dev(tok)
    call("mvml_bilstm_packed_tokens", n, T, ptr(d_offs), ptr(d_tok), ldtok,
         ptr(d_perm), ptr(out), stream_ptr())
    assert np.array_equal(out[:n].cpu().numpy(), C.packed_tokens_ref(tok, perm, batch_sizes))
    assert int(out[n]) == -7


def _check_token_sums(runs, g_rows, tok_rows, vocab, cols):
    """Two runs' [vocab + 1, cols] outputs: bitwise equal, a sentinel guard row, exact zeros for
    absent tokens, and every entry within sequential fp32 summation's bound of the float64 sum."""
    a, b = (r.cpu().numpy() for r in runs)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    assert (a[vocab:] == SENT).all()
    s, asum, n = C.token_sums(g_rows, tok_rows, vocab)
    got = a[:vocab].astype(np.float64)
    assert (got[n == 0] == 0.0).all()
    excess = np.abs(got - s) - C.token_sum_bound(asum, n)
    assert (excess <= 0).all(), (float(excess.max()), np.unravel_index(excess.argmax(), excess.shape))


@pytest.mark.parametrize("vocab", [39, 64])
@pytest.mark.parametrize("T,B", [(1, 1), (15, 17), (16, 16), (1, 257), (19, 27)])
def test_token_grad(T, B, vocab):
    """T B = 1, 255, 256, 257, 513 positions against the 256-position chunks; cols against the
    256-column slabs.  Padded positions hold NaN: only live positions may be summed."""
    lens = C.ragged_lengths(B, T, T * B)
    perm, _, batch_sizes, _, d_lens, d_perm, _ = _meta(lens)
    ldtok = T + 1
    tok = C.tokens_for(lens, vocab, T + B, T=T, ldtok=ldtok)
    if T * B > 1:
        tok[tok == 5] = 6  # a token that never occurs
    tok_rows = C.packed_tokens_ref(tok, perm, batch_sizes)
    live = C.live_mask(lens).reshape(-1)
    d_tok = _dev(tok)
    for cols in (4, 120, 256, 260):
        g = np.random.default_rng(cols + B).standard_normal((T * B, cols)).astype(np.float32)
        g[~live] = np.nan
        d_g = _dev(g)
        nws = int(lib().mvml_bilstm_token_grad_workspace(T, B, cols, vocab))
        runs = []
        for _ in range(2):
            ws = torch.full((nws // 4,), float("nan"), device=DEV)
            out = torch.full((vocab + 1, cols), SENT, device=DEV)
            call("mvml_bilstm_token_grad", T, B, cols, ptr(d_g), ptr(d_tok), ldtok, ptr(d_lens), ptr(d_perm),
                 vocab, ptr(out), ptr(ws), nws, stream_ptr())
            runs.append(out)
        _check_token_sums(runs, g[live], tok_rows, vocab, cols)


@pytest.mark.parametrize("nrows", [0, 1, 7, 8, 9, 1023, 1024, 1025, 2055])
def test_token_grad_packed(nrows):
    """Row counts around the 8-row unrolled body with its scalar tail and the 1024-row chunks;
    a ragged last 256-column slab; a row pitch past cols (the pitch columns hold NaN)."""
    for vocab in (39, 64):
        rng = np.random.default_rng(nrows + vocab)
        tok = rng.integers(0, vocab, size=nrows).astype(np.int32)
        if nrows:
            tok[0] = vocab - 1
            tok[tok == 5] = 6
        d_tok = _dev(tok) if nrows else torch.zeros(1, dtype=torch.int32, device=DEV)
        for cols in (4, 260):
            for ldg in (cols, cols + 4):
                g = rng.standard_normal((max(nrows, 1), ldg)).astype(np.float32)
                g[:, cols:] = np.nan
                d_g = _dev(g)
                nws = int(lib().mvml_bilstm_token_grad_packed_workspace(nrows, cols, vocab))
                runs = []
                for _ in range(2):
                    ws = torch.full((nws // 4,), float("nan"), device=DEV)
                    out = torch.full((vocab + 1, cols), SENT, device=DEV)
                    call("mvml_bilstm_token_grad_packed", nrows, cols, ptr(d_g), ldg, ptr(d_tok), vocab,
                         ptr(out), ptr(ws), nws, stream_ptr())
                    runs.append(out)
                _check_token_sums(runs, g[:nrows, :cols], tok, vocab, cols)


def test_token_grads_refuse_vocab_65():
    T, B, cols, vocab = 2, 3, 8, C.TOK_MAX_VOCAB + 1
    lens = [2, 1, 2]
    perm, _, batch_sizes, offsets, d_lens, d_perm, _ = _meta(lens)
    tok = C.tokens_for(lens, vocab, 0)
    d_tok = _dev(tok)
    d_g = torch.randn((T * B, cols), device=DEV)
    ws = torch.zeros((4 * vocab * cols,), device=DEV)
    out = torch.full((vocab, cols), SENT, device=DEV)
    with pytest.raises(MvmlError, match="vocab <= 64"):
        call("mvml_bilstm_token_grad", T, B, cols, ptr(d_g), ptr(d_tok), T, ptr(d_lens), ptr(d_perm),
             vocab, ptr(out), ptr(ws), ws.numel() * 4, stream_ptr())
    tok_rows = _dev(C.packed_tokens_ref(tok, perm, batch_sizes))
    with pytest.raises(MvmlError, match="vocab <= 64"):
        call("mvml_bilstm_token_grad_packed", int(offsets[-1]), cols, ptr(d_g), cols, ptr(tok_rows), vocab,
             ptr(out), ptr(ws), ws.numel() * 4, stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
