"""Inputs and plain restatements for the SMILES BiLSTM shape tests (csrc/smiles_lstm.hip, the
wide-step entry points of csrc/gemm_f32.hip, mvml_gat/smiles.py).  No GPU import: the CPU
conditions on these inputs and restatements are in test_smiles_cases_cpu.py, the GPU
comparisons in test_gpu_smiles_shapes.py.

Packed layout (smiles_lstm.hip's header): the batch is ordered by descending length, perm[i] =
original index of sorted row i (ties keep their original order), pos = perm's inverse, and stored
time-major, row t * B + i; the sequences alive at step t are the prefix i < batch_sizes[t].

Every restatement below is written from its kernel's header comment, as a loop over the rows
that comment names, in numpy; none follows the kernel's body (no chunks, slabs or unrolling).
"""
import numpy as np

SEQ_H = 384       # the fused step kernels' hidden size (MVP's blstm_dim)
SEQ_MAX_B = 512   # the fused step path's widest batch
STEP_ROWS = 16    # rows of a fused step kernel's block
TOK_MAX_VOCAB = 64


# ------------------------------------------------------------------ length catalogue
def ragged_lengths(B, T, seed):
    """B lengths in 1 .. T in no particular order: every length present where B >= T, else at
    least one T and (B > 1) one 1."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, size=B)
    head = np.arange(1, T + 1) if B >= T else np.array([T, 1][:B])
    lens[:head.size] = head
    return rng.permutation(lens).tolist()


_LENGTHS = {
    "one": [1],
    "single7": [7],
    "eq16": [6] * 16,
    "eq17": [3] * 17,
    "stair17": list(range(17, 0, -1)),
    "cliff33": [3] + [2] * 15 + [1] * 17,            # batch sizes 33, 16, 1
    "blocks48": [5] * 16 + [3] * 16 + [1] * 16,      # batch sizes 48, 32, 32, 16, 16
    "b512": ragged_lengths(512, 6, 512),
    "b513": ragged_lengths(513, 6, 513),
    "r5x9": ragged_lengths(5, 9, 59),                # the hidden-size cases' ragged (B, T)
    "r140x12": ragged_lengths(140, 12, 152),         # 140 rows cross the 128-row GEMM tile
}
NAMES = tuple(_LENGTHS)


def lengths(name):
    """The entry's lengths in a fixed shuffled order (so perm and pos are not the identity)."""
    lens = np.asarray(_LENGTHS[name], dtype=np.int64)
    order = np.random.default_rng(len(name) + 31 * lens.size).permutation(lens.size)
    return lens[order].tolist()


def tokens_for(lens, vocab, seed, T=None, ldtok=None, low=0):
    """int32 [B, ldtok] tokens: uniform in [low, vocab) at live positions with the largest token
    vocab - 1 placed at the first live position, zeros (the pad token) elsewhere."""
    lens = np.asarray(lens, dtype=np.int64)
    T = int(lens.max()) if T is None else T
    ldtok = T if ldtok is None else ldtok
    rng = np.random.default_rng(seed)
    tok = rng.integers(low, vocab, size=(lens.size, ldtok)).astype(np.int32)
    tok[0, 0] = vocab - 1
    tok[np.arange(ldtok)[None, :] >= lens[:, None]] = 0
    return tok


# ------------------------------------------------------------------ packed order
def packed_order(lens):
    """(perm, pos, batch_sizes, offsets): descending length, ties in original order;
    batch_sizes[t] = number of sequences longer than t; offsets = their running sum."""
    lens = np.asarray(lens, dtype=np.int64)
    perm = np.asarray(sorted(range(lens.size), key=lambda b: (-lens[b], b)), dtype=np.int64)
    pos = np.empty_like(perm)
    for i, b in enumerate(perm):
        pos[b] = i
    batch_sizes = [int(sum(1 for n in lens if n > t)) for t in range(int(lens.max()))]
    offsets = np.concatenate([[0], np.cumsum(batch_sizes)]).astype(np.int64)
    return perm, pos, batch_sizes, offsets


def live_mask(lens):
    """bool [T, B] over the sorted, time-major layout: row i of step t is alive."""
    perm, _, batch_sizes, _ = packed_order(lens)
    m = np.zeros((len(batch_sizes), len(perm)), dtype=bool)
    for t, bs in enumerate(batch_sizes):
        m[t, :bs] = True
    return m


# ------------------------------------------------------------------ index kernels
def gather_rows_ref(table, tokens, lens, perm, T):
    """out[t * B + i, :] = table[tokens[perm[i], t], :] if t < lens[perm[i]] else 0."""
    B = len(perm)
    out = np.zeros((T * B, table.shape[1]), dtype=table.dtype)
    for t in range(T):
        for i in range(B):
            b = perm[i]
            if t < lens[b]:
                out[t * B + i] = table[tokens[b, t]]
    return out


def select_last_gather(out, lens, pos):
    """fea[b] = [out[len_b - 1, pos_b, :H] | out[0, pos_b, H:]] of the time-major [T, B, 2H] out."""
    T, B, H2 = out.shape
    H = H2 // 2
    fea = np.empty((B, H2), dtype=out.dtype)
    for b in range(B):
        fea[b, :H] = out[lens[b] - 1, pos[b], :H]
        fea[b, H:] = out[0, pos[b], H:]
    return fea


def select_last_scatter(g_out, fea, lens, pos):
    """The reverse copy, in place: g_out[len_b - 1, pos_b, :H] = fea[b, :H], g_out[0, pos_b, H:] =
    fea[b, H:]; nothing else is written."""
    H = g_out.shape[2] // 2
    for b in range(fea.shape[0]):
        g_out[lens[b] - 1, pos[b], :H] = fea[b, :H]
        g_out[0, pos[b], H:] = fea[b, H:]
    return g_out


def pack_rows_ref(tm, batch_sizes, t0, t1, shift):
    """Rows (t + shift, p), t in [t0, t1), p < batch_sizes[t], of the time-major [T, B, cols]
    view tm, consecutively."""
    rows = [tm[t + shift, p] for t in range(t0, t1) for p in range(batch_sizes[t])]
    return np.stack(rows) if rows else np.zeros((0, tm.shape[2]), dtype=tm.dtype)


def unpack_rows_ref(tm, packed, batch_sizes, t0, t1, shift):
    """The reverse copy, in place on the [T, B, cols] view tm; nothing else is written."""
    r = 0
    for t in range(t0, t1):
        for p in range(batch_sizes[t]):
            tm[t + shift, p] = packed[r]
            r += 1
    return tm


def packed_tokens_ref(tokens, perm, batch_sizes):
    """tok[offsets[t] + p] = tokens[perm[p], t]: step t of sorted sequence p."""
    return np.asarray([tokens[perm[p], t] for t, bs in enumerate(batch_sizes) for p in range(bs)],
                      dtype=np.int32)


def token_sums(g, tok, vocab):
    """Per-token sums over rows g[r] with token tok[r], in float64: (sum [vocab, cols],
    sum of |g| [vocab, cols], rows per token [vocab])."""
    g = np.asarray(g, dtype=np.float64)
    s = np.zeros((vocab, g.shape[1]))
    a = np.zeros((vocab, g.shape[1]))
    n = np.zeros(vocab, dtype=np.int64)
    for r, v in enumerate(tok):
        s[v] += g[r]
        a[v] += np.abs(g[r])
        n[v] += 1
    return s, a, n


def token_sum_bound(abs_sum, n):
    """Sequential fp32 summation of n terms: |fl(sum) - sum| <= (n - 1) u sum|g| + O(u^2) with
    u = 2^-24.  Summing chunks first and then the chunk sums in order passes no term through
    more than n - 1 rounded additions either (adding an exact zero does not round), so the same
    first-order bound holds; n u sum|g| covers the second-order term for n < 2^23."""
    return n[:, None] * 2.0 ** -24 * abs_sum


# ------------------------------------------------------------------ which recurrence runs
SEQ_ENTRIES = ("mvml_bilstm_seq_fwd", "mvml_bilstm_seq_bwd")
WIDE_ENTRIES = ("mvml_bilstm_wide_fwd", "mvml_bilstm_wide_bwd")
CELL_ENTRIES = ("mvml_lstm_cell_fwd", "mvml_lstm_cell_bwd")


def expected_entries(B, H, gemm_algo, seq_max_b=SEQ_MAX_B, wide_step=True):
    """The documented dispatch of a BiLSTM layer's recurrence (mvml_gat/smiles.py's module
    docstring and option comments): the fused step kernels for B <= 512 at H = 384; wider
    batches and other hidden sizes one dual launch per step for H % 8 == 0 on the split-fp16
    GEMM; a GEMM and a cell kernel per direction and step otherwise."""
    if B <= seq_max_b and H == SEQ_H:
        return SEQ_ENTRIES
    if wide_step and H % 8 == 0 and gemm_algo == "f16x2":
        return WIDE_ENTRIES
    return CELL_ENTRIES
