"""mvml_gin_edge_codes / mvml_gin_agg_fwd / mvml_gin_edge_emb_grad / mvml_embed_sum_fwd / _bwd /
mvml_relu_f32 (csrc/gin_agg.hip) and mvml_segment_pool_fwd / _bwd (csrc/segment_pool.hip) through
the C ABI against the CPU reference (tests/_gin_ref.py).

Graphs: GRAPHS of tests/test_gpu_gatv2_agg.py (the 170-atom `mixed`, a single atom, `hubs` with
in-degrees past one 64-entry chunk, `big_hub` with 202 in-edges = four chunks, `zero_in_degree`) and
N = 0.  Widths: 4; 64 and 68 (the last width of the four-rows-per-wave form and the first past it; at
D <= 64 option gin_subwave = 0 runs the one-row form, bitwise the default); 256 / 260, 512 /
516, 768 and 1024: each count of float4 slots per lane (1 .. 4) full and with a partly masked last
slot; 300, the default.  Tables: T = 1, 2, 4 with R = 1, 9, 256 rows in all; categories seeded, with
the first edges set to every table's last row.  The tables are staged in LDS where R * D * 4 <=
49152 bytes: R = 256 at D = 64 and D = 300 is past that, so the L2 path runs there by itself, and
option gin_lds = 0 runs it everywhere (bitwise the default).

X, E and G have row pitches past D with NaN in the pad; outputs sit between sentinel guards
(_Guarded) and are pre-filled with a sentinel that must survive in their pads.

Bar (the project's rule): conftest.rel_err <= max(1e-5, 4 e32) against the float64 reference, e32
the same reference in float32 against its float64 run."""
import functools

import numpy as np
import pytest
import torch

import mvml_gat
from _gin_ref import edge_term, embed_sum_ref, first_owner, gin_agg_ref, segment_pool_ref
from _util import batch_of_sizes
from conftest import rel_err
from mvml_gat._lib import lib, option, ptr, stream_ptr, ws_ptr_size
from test_gpu_gatv2_agg import FILL, GRAPHS, GUARD, MVML_ERR_INVALID, _Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
IFILL = -7777
WIDTHS = [4, 64, 68, 256, 260, 300, 512, 516, 768, 1024]
TABLES = {"T1R1": [1], "T2R9": [6, 3], "T4R256": [120, 100, 30, 6], "T1R256": [256], "T4R9": [4, 2, 2, 1]}
LDS_BYTES = 48 * 1024


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = GRAPHS[name]().to(DEV)
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    assert torch.equal(g.in_eid.cpu().long(), torch.argsort(dst, stable=True))
    return g, src, dst


def _bits(x):
    return x.contiguous().view(torch.int32)


def _budget(r32, r64):
    return max(TOL, 4 * rel_err(r32, r64))


def _padded(t, pad=12):
    X = torch.full((t.shape[0], t.shape[1] + pad), float("nan"))
    X[:, :t.shape[1]] = t
    return X


class _IGuarded:
    """An int32 device vector between two sentinel guards, all pre-filled."""

    def __init__(self, n):
        self.whole = torch.full((n + 2 * GUARD,), IFILL, dtype=torch.int32, device=DEV)
        self.t = self.whole[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.whole[:GUARD] == IFILL).all()) and bool((self.whole[-GUARD:] == IFILL).all())


def _cats(n, sizes, seed):
    """Seeded categories [n] per table (CPU int64); the first entries name every table's last row."""
    gen = torch.Generator().manual_seed(seed)
    cats = [torch.randint(0, s, (n,), generator=gen) for s in sizes]
    for t, s in enumerate(sizes):
        if n > t:
            cats[t][t] = s - 1
    return cats


def _tables(sizes, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn((s, D), generator=gen) for s in sizes]


def _table_args(cats_dev, sizes):
    T = len(sizes)
    return (T, *[ptr(c) for c in cats_dev], *[None] * (4 - T), *sizes, *[0] * (4 - T))


def _codes(g, cats, sizes, E=None):
    """(rc, guarded codes, status, device category tensors) of one mvml_gin_edge_codes call."""
    E = g.num_edges() if E is None else E
    dev = [c.to(torch.int32).to(DEV) for c in cats]
    codes = _IGuarded(max(E, 1))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib().mvml_gin_edge_codes(E, *_table_args(dev, sizes), ptr(g.in_eid), ptr(codes.t), ptr(status), stream_ptr())
    torch.cuda.synchronize()
    return rc, codes, status, dev


def _want_codes(dst, cats, sizes):
    order = torch.argsort(dst, stable=True)
    code = torch.zeros(order.numel(), dtype=torch.long)
    off = 0
    for t, (c, s) in enumerate(zip(cats, sizes)):
        code |= (off + c.clamp(0, s - 1)[order]) << (8 * t)
        off += s
    return code.to(torch.int32)  # (R <= 256 and T <= 4: at most the sign bit wraps)


def _agg(g, codes, X, D, Etab, R, T, rows=True, N=None, ldx=None, lde=None, out=None, ldo=None):
    N = g.num_nodes() if N is None else N
    ldo = D + 4 if ldo is None else ldo
    out = _Guarded(max(N, 1), ldo) if out is None else out
    omx = torch.zeros(1, dtype=torch.int32, device=DEV)
    orow = torch.zeros(max(N, 1), dtype=torch.int32, device=DEV)
    rc = lib().mvml_gin_agg_fwd(N, ptr(g.in_rowptr), ptr(g.in_src), ptr(codes), ptr(X),
                                X.stride(0) if ldx is None else ldx, D, ptr(Etab),
                                Etab.stride(0) if lde is None else lde, R, T, ptr(out.t), ldo, ptr(omx),
                                ptr(orow) if rows else None, stream_ptr())
    torch.cuda.synchronize()
    return rc, out, omx, orow


def _emb_grad(g, codes, G, D, R, T, N=None):
    N = g.num_nodes() if N is None else N
    dE = _Guarded(R, D)
    wp, wn = ws_ptr_size(lib().mvml_gin_emb_grad_workspace_size(N, R, D), DEV)
    rc = lib().mvml_gin_edge_emb_grad(N, ptr(g.in_rowptr), ptr(codes), ptr(G), G.stride(0), D, R, T, ptr(dE.t), wp, wn,
                                      stream_ptr())
    torch.cuda.synchronize()
    return rc, dE


def _ref(src, dst, Xc, tabs, cats, Gc, dtype):
    """(out, dX, dE concatenated) of the reference in dtype."""
    X = Xc.to(dtype).clone().requires_grad_()
    ws = [w.to(dtype).clone().requires_grad_() for w in tabs]
    out = gin_agg_ref(src, dst, X, ws, cats)
    out.backward(Gc.to(dtype))
    return out.detach(), X.grad, torch.cat([w.grad for w in ws], 0)


def _check(graph, D, tname, seed, backward=True):
    g, src, dst = _graph(graph)
    N, E = g.num_nodes(), g.num_edges()
    sizes = TABLES[tname]
    R, T = sum(sizes), len(sizes)
    what = f"{graph} D={D} {tname}"
    cats = _cats(E, sizes, seed)
    tabs = _tables(sizes, D, seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    Xc, Gc = torch.randn((N, D), generator=gen), torch.randn((N, D), generator=gen)
    rc, codes, status, _ = _codes(g, cats, sizes)
    assert rc == 0 and status.item() == 0 and codes.guards_intact(), (what, lib().mvml_last_error())
    assert torch.equal(codes.t.cpu(), _want_codes(dst, cats, sizes)), (what, "codes")
    X, Etab = _padded(Xc).to(DEV), _padded(torch.cat(tabs, 0), 8).to(DEV)
    o64, dX64, dE64 = _ref(src, dst, Xc, tabs, cats, Gc, torch.float64)
    o32, dX32, dE32 = _ref(src, dst, Xc, tabs, cats, Gc, torch.float32)
    rc, out, omx, orow = _agg(g, codes.t, X, D, Etab, R, T)
    assert rc == 0, (what, lib().mvml_last_error())
    got = out.t[:N, :D]
    e, b = rel_err(got, o64), _budget(o32, o64)
    print(f"gin_agg_fwd {what}: {e:.2e} / {b:.2e}")
    assert bool(torch.isfinite(got).all()) and e <= b, (what, e, b)
    assert out.guards_intact() and bool((out.t[:, D:] == FILL).all()), (what, "written outside the rows")
    empty = torch.bincount(dst, minlength=N) == 0
    if bool(empty.any()):
        assert float(got.cpu()[empty].abs().max()) == 0.0, (what, "a row without in-edges is 0")
    assert _bits(omx).item() == _bits(got.abs().max().reshape(1)).item(), (what, "out_amax")
    assert torch.equal(_bits(orow[:N]), _bits(got.abs().max(dim=1).values)), (what, "out_row_amax")
    rc, out2, omx2, _ = _agg(g, codes.t, X, D, Etab, R, T, rows=False)
    assert rc == 0 and torch.equal(_bits(out2.whole), _bits(out.whole)) and omx2.item() == omx.item(), (what, "repeat")
    with option("gin_lds", 0):  # every wave reads its table rows from L2: the same bits
        rc, out3, omx3, orow3 = _agg(g, codes.t, X, D, Etab, R, T)
    assert rc == 0 and torch.equal(_bits(out3.whole), _bits(out.whole)) and torch.equal(orow3, orow), (what, "gin_lds=0")
    if D <= 64:  # four rows per wave (the default there) against one row per wave, each on both table paths
        for sub, lds in ((0, 1), (0, 0), (1, 0)):
            with option("gin_subwave", sub), option("gin_lds", lds):
                rc, out4, omx4, orow4 = _agg(g, codes.t, X, D, Etab, R, T)
            assert rc == 0 and torch.equal(_bits(out4.whole), _bits(out.whole)) and torch.equal(orow4, orow) \
                and omx4.item() == omx.item(), (what, f"gin_subwave={sub} gin_lds={lds}")
    if not backward:
        return
    G = _padded(Gc).to(DEV)
    # dX: mvml_gcn_agg over the out-CSR with NULL scales
    dX = _Guarded(N, D + 4)
    rc = lib().mvml_gcn_agg(N, ptr(g.out_rowptr), ptr(g.out_dst), ptr(G), G.stride(0), D, None, None, None, 0,
                            ptr(dX.t), D + 4, None, None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and rel_err(dX.t[:, :D], dX64) <= _budget(dX32, dX64), (what, "dX")
    rc, dE = _emb_grad(g, codes.t, G, D, R, T)
    assert rc == 0, (what, lib().mvml_last_error())
    e, b = rel_err(dE.t, dE64), _budget(dE32, dE64)
    print(f"gin_edge_emb_grad {what}: {e:.2e} / {b:.2e}")
    assert bool(torch.isfinite(dE.t).all()) and e <= b and dE.guards_intact(), (what, "dE", e, b)
    rc, dE2 = _emb_grad(g, codes.t, G, D, R, T)
    assert rc == 0 and torch.equal(_bits(dE2.whole), _bits(dE.whole)), (what, "dE repeat")


@pytest.mark.parametrize("D", WIDTHS)
def test_every_width_on_mixed(D):
    _check("mixed", D, "T2R9", seed=100 + D)


@pytest.mark.parametrize("D", [64, 300])
@pytest.mark.parametrize("graph", ["one_atom", "hubs", "big_hub", "zero_in_degree"])
def test_every_graph(graph, D):
    _check(graph, D, "T2R9", seed=200 + D)


@pytest.mark.parametrize("D", [4, 64, 300])
@pytest.mark.parametrize("tname", ["T1R1", "T4R256", "T1R256", "T4R9"])
def test_every_table_shape(tname, D):
    R = sum(TABLES[tname])
    if tname.endswith("R256"):  # D = 4 is staged in LDS, D = 64 and D = 300 are past the budget: the L2 path
        assert (R * D * 4 <= LDS_BYTES) == (D == 4)
    _check("mixed", D, tname, seed=300 + D)


def test_widest_rows_with_the_largest_table_on_hubs():
    _check("hubs", 1024, "T4R256", seed=77)


def test_no_atoms():
    g, _, _ = _graph("one_atom")
    out = _Guarded(1, 8)
    X, Etab = torch.zeros((1, 4), device=DEV), torch.zeros((9, 4), device=DEV)
    codes = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc, out, _, _ = _agg(g, codes, X, 4, Etab, 9, 2, N=0, out=out, ldo=8)
    assert rc == 0 and bool((out.whole == FILL).all())
    rc, dE = _emb_grad(g, codes, X, 4, 9, 2, N=0)
    assert rc == 0 and float(dE.t.abs().max()) == 0.0 and dE.guards_intact()  # an empty batch: zeros
    rc, c, status, _ = _codes(g, [torch.zeros(1, dtype=torch.long)] * 2, [6, 3], E=0)
    assert rc == 0 and bool((c.whole == IFILL).all()) and status.item() == 0


def _sub_batch(sb, k):
    """Molecule k of the SynthBatch sb alone, and its atom and edge ranges in sb."""
    no, eo = np.concatenate([[0], np.cumsum(sb.num_nodes)]), np.concatenate([[0], np.cumsum(sb.num_edges)])
    a, b, ea, eb = int(no[k]), int(no[k + 1]), int(eo[k]), int(eo[k + 1])
    one = mvml_gat.from_arrays(sb.num_nodes[k:k + 1], sb.num_edges[k:k + 1], sb.src_local[ea:eb], sb.dst_local[ea:eb])
    return one, (a, b), (ea, eb)


@pytest.mark.parametrize("D", [64, 300])
def test_a_molecule_alone_has_the_bits_it_has_inside_the_batch(D):
    sb = batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5], seed=1)
    g, src, dst = _graph("mixed")
    sizes = TABLES["T2R9"]
    cats, tabs = _cats(g.num_edges(), sizes, 5), _tables(sizes, D, 6)
    Xc = torch.randn((g.num_nodes(), D), generator=torch.Generator().manual_seed(7))
    Etab = torch.cat(tabs, 0).to(DEV)
    _, codes, _, _ = _codes(g, cats, sizes)
    rc, whole, _, _ = _agg(g, codes.t, Xc.to(DEV), D, Etab, 9, 2)
    assert rc == 0
    for k in (2, 1, 6):
        one, (a, b), (ea, eb) = _sub_batch(sb, k)
        one = one.to(DEV)
        _, c1, st, _ = _codes(one, [c[ea:eb] for c in cats], sizes)
        assert st.item() == 0
        for lds, sub in ((1, 1), (0, 1), (1, 0)):  # a different grid, the other table path, the other form
            with option("gin_lds", lds), option("gin_subwave", sub):
                rc, part, _, _ = _agg(one, c1.t, Xc[a:b].to(DEV), D, Etab, 9, 2)
            assert rc == 0 and torch.equal(_bits(part.t[:, :D]), _bits(whole.t[a:b, :D])), (k, lds, sub)


def test_out_of_range_categories_are_counted_and_clamped():
    g, src, dst = _graph("mixed")
    E, sizes = g.num_edges(), [6, 3]
    cats = _cats(E, sizes, 9)
    cats[0][5], cats[0][17], cats[1][40], cats[1][41] = -1, 6, 3, 1 << 20
    rc, codes, status, _ = _codes(g, cats, sizes)
    assert rc == 0 and status.item() == 4 and codes.guards_intact()
    got = codes.t.cpu()
    assert torch.equal(got, _want_codes(dst, cats, sizes))  # (clamped into the tables)
    assert int((got & 255).max()) <= 5 and 6 <= int(((got >> 8) & 255).min()) and int(((got >> 8) & 255).max()) <= 8
    assert int((got >> 16).abs().max()) == 0
    # the forward on clamped codes equals the reference on clamped categories
    D = 20
    tabs, Xc = _tables(sizes, D, 1), torch.randn((g.num_nodes(), D), generator=torch.Generator().manual_seed(2))
    rc, out, _, _ = _agg(g, codes.t, Xc.to(DEV), D, torch.cat(tabs, 0).to(DEV), 9, 2)
    want = gin_agg_ref(src, dst, Xc.double(), [w.double() for w in tabs], [c.clamp(0, s - 1) for c, s in zip(cats, sizes)])
    assert rc == 0 and rel_err(out.t[:, :D], want) <= TOL and out.guards_intact()


@pytest.mark.parametrize("why", ["D%4", "D>1024", "misaligned X", "misaligned E", "out is X", "R>256", "T>R", "T=0",
                                 "pitch<D"])
def test_agg_refusals_leave_the_buffers_untouched(why):
    g, _, _ = _graph("mixed")
    N = g.num_nodes()
    D, R, T = 8, 9, 2
    big = torch.zeros(N * 1040 + 8, device=DEV)
    X, Etab = big[:N * 12].view(N, 12), torch.zeros((257, 12), device=DEV)
    codes = torch.zeros(g.num_edges(), dtype=torch.int32, device=DEV)
    out = _Guarded(N, 1040)
    kw = {}
    if why == "D%4":
        D = 6
    elif why == "D>1024":
        D, X = 1028, big[:N * 1040].view(N, 1040)
        Etab = torch.zeros((9, 1040), device=DEV)
    elif why == "misaligned X":
        X = big[1:N * 12 + 1].view(N, 12)
    elif why == "misaligned E":
        Etab = torch.zeros(9 * 12 + 1, device=DEV)[1:].view(9, 12)
    elif why == "out is X":
        class _Alias:
            t = X
        kw = dict(out=_Alias, ldo=12)
    elif why == "R>256":
        R = 257
    elif why == "T>R":
        R, T = 3, 4
    elif why == "T=0":
        T = 0
    elif why == "pitch<D":
        kw = dict(ldx=4)
    rc, o, _, _ = _agg(g, codes, X, D, Etab, R, T, **({"out": out, "ldo": 1040} | kw))
    assert rc == MVML_ERR_INVALID and lib().mvml_last_error(), why
    assert bool((out.whole == FILL).all()) and float(big.abs().max()) == 0.0, why


@pytest.mark.parametrize("why", ["R>256", "T=5", "empty table", "missing array"])
def test_codes_refusals_leave_the_buffers_untouched(why):
    g, _, _ = _graph("mixed")
    E = g.num_edges()
    sizes = {"R>256": [200, 57], "T=5": [2, 2], "empty table": [6, 0], "missing array": [6, 3]}[why]
    dev = [torch.zeros(E, dtype=torch.int32, device=DEV) for _ in sizes]
    args = list(_table_args(dev, sizes))
    if why == "T=5":
        args[0] = 5
    if why == "missing array":
        args[2] = None
    codes = _IGuarded(E)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib().mvml_gin_edge_codes(E, *args, ptr(g.in_eid), ptr(codes.t), ptr(status), stream_ptr())
    torch.cuda.synchronize()
    assert rc == MVML_ERR_INVALID and bool((codes.whole == IFILL).all()) and status.item() == 0, why


# ---- the two-stage table gradients ----------------------------------------------------------------
def _embed(idx, sizes, tab, D, N=None, status=None):
    N = idx[0].shape[0] if N is None else N
    out = _Guarded(max(N, 1), D + 4)
    rc = lib().mvml_embed_sum_fwd(N, *_table_args(idx, sizes), ptr(tab), tab.stride(0), D, ptr(out.t), D + 4, ptr(status),
                                  stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _embed_bwd(idx, sizes, G, D, N=None):
    N = idx[0].shape[0] if N is None else N
    R = sum(sizes)
    dT = _Guarded(R, D)
    wp, wn = ws_ptr_size(lib().mvml_gin_emb_grad_workspace_size(N, R, D), DEV)
    rc = lib().mvml_embed_sum_bwd(N, *_table_args(idx, sizes), ptr(G), G.stride(0), D, ptr(dT.t), wp, wn, stream_ptr())
    torch.cuda.synchronize()
    return rc, dT


def _embed_ref(tabs, idx, Gc, dtype):
    ws = [w.to(dtype).clone().requires_grad_() for w in tabs]
    out = embed_sum_ref(ws, idx)
    out.backward(Gc.to(dtype))
    return out.detach(), torch.cat([w.grad for w in ws], 0)


@pytest.mark.parametrize("D", [4, 64, 300, 1024])
@pytest.mark.parametrize("case", ["N1", "carbon", "four_tables", "full_tables"])
def test_embed_sum_forward_and_backward(case, D):
    N, sizes = {"N1": (1, [120, 3]), "carbon": (3000, [120, 3]), "four_tables": (170, [5, 1, 7, 2]),
                "full_tables": (700, [128, 128, 128, 128])}[case]
    assert lib().mvml_gin_partial_rows(3000) >= 3 and lib().mvml_gin_partial_rows(1) == 1
    idx = _cats(N, sizes, 11)
    if case == "carbon":  # one row of the first table owns more than 90 % of the atoms
        keep = torch.rand(N, generator=torch.Generator().manual_seed(3)) < 0.07
        idx[0] = torch.where(keep, idx[0], torch.full_like(idx[0], 5))
        assert float((idx[0] == 5).float().mean()) > 0.9
    tabs = _tables(sizes, D, 12)
    Gc = torch.randn((N, D), generator=torch.Generator().manual_seed(13))
    o64, d64 = _embed_ref(tabs, idx, Gc, torch.float64)
    o32, d32 = _embed_ref(tabs, idx, Gc, torch.float32)
    dev = [c.to(torch.int32).to(DEV) for c in idx]
    tab = _padded(torch.cat(tabs, 0), 8).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc, out = _embed(dev, sizes, tab, D, status=status)
    assert rc == 0 and status.item() == 0, lib().mvml_last_error()
    assert rel_err(out.t[:, :D], o64) <= _budget(o32, o64) and out.guards_intact() and bool((out.t[:, D:] == FILL).all())
    rc, out2 = _embed(dev, sizes, tab, D)  # (status may be NULL)
    assert rc == 0 and torch.equal(_bits(out2.whole), _bits(out.whole))
    G = _padded(Gc).to(DEV)
    rc, dT = _embed_bwd(dev, sizes, G, D)
    assert rc == 0, lib().mvml_last_error()
    e, b = rel_err(dT.t, d64), _budget(d32, d64)
    print(f"embed_sum_bwd {case} D={D}: {e:.2e} / {b:.2e}")
    assert bool(torch.isfinite(dT.t).all()) and e <= b and dT.guards_intact(), (e, b)
    rc, dT2 = _embed_bwd(dev, sizes, G, D)
    assert rc == 0 and torch.equal(_bits(dT2.whole), _bits(dT.whole))


def test_embed_sum_counts_and_clamps_out_of_range_indices():
    sizes, D, N = [6, 3], 8, 50
    idx = _cats(N, sizes, 1)
    idx[0][7], idx[1][9], idx[1][10] = 6, -5, 3
    tabs = _tables(sizes, D, 2)
    dev = [c.to(torch.int32).to(DEV) for c in idx]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc, out = _embed(dev, sizes, torch.cat(tabs, 0).to(DEV), D, status=status)
    want = embed_sum_ref([w.double() for w in tabs], [c.clamp(0, s - 1) for c, s in zip(idx, sizes)])
    assert rc == 0 and status.item() == 3 and rel_err(out.t[:, :D], want) <= TOL and out.guards_intact()
    rc, dT = _embed_bwd(dev, sizes, torch.ones((N, D), device=DEV), D)
    assert rc == 0 and dT.guards_intact() and float(dT.t.sum()) == 2 * N * D  # every atom lands in both tables


@pytest.mark.parametrize("why", ["D%4", "D>1024", "129 rows", "T=5", "misaligned tab", "out is tab"])
def test_embed_refusals_leave_the_buffers_untouched(why):
    N, D, sizes = 10, 8, [6, 3]
    tab = torch.zeros((300, 1040), device=DEV)
    if why == "D%4":
        D = 6
    elif why == "D>1024":
        D = 1028
    elif why == "129 rows":
        sizes = [129, 3]
    dev = [torch.zeros(N, dtype=torch.int32, device=DEV) for _ in sizes]
    args = list(_table_args(dev, sizes))
    if why == "T=5":
        args[0] = 5
    tp = tab
    if why == "misaligned tab":
        tp = tab.view(-1)[1:1 + 9 * 1040].view(9, 1040)
    out = _Guarded(N, 1040)
    op = tab if why == "out is tab" else out.t
    rc = lib().mvml_embed_sum_fwd(N, *args, ptr(tp), 1040, D, ptr(op), 1040, None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == MVML_ERR_INVALID and bool((out.whole == FILL).all()) and float(tab.abs().max()) == 0.0, why


def test_edge_table_gradient_over_several_atom_ranges():
    """A few thousand atoms: mvml_gin_partial_rows(N) >= 3 partial tables, summed in a fixed order."""
    sb = batch_of_sizes([30] * 100 + [7] * 11, seed=4)
    g = sb.to_graph().to(DEV)
    N, E = g.num_nodes(), g.num_edges()
    assert lib().mvml_gin_partial_rows(N) >= 3
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    for D, tname in ((300, "T2R9"), (64, "T4R256")):
        sizes = TABLES[tname]
        cats, tabs = _cats(E, sizes, 21), _tables(sizes, D, 22)
        gen = torch.Generator().manual_seed(23)
        Xc, Gc = torch.randn((N, D), generator=gen), torch.randn((N, D), generator=gen)
        _, _, d64 = _ref(src, dst, Xc, tabs, cats, Gc, torch.float64)
        _, _, d32 = _ref(src, dst, Xc, tabs, cats, Gc, torch.float32)
        rc, codes, status, _ = _codes(g, cats, sizes)
        assert rc == 0 and status.item() == 0
        G = _padded(Gc).to(DEV)
        rc, dE = _emb_grad(g, codes.t, G, D, sum(sizes), len(sizes))
        e, b = rel_err(dE.t, d64), _budget(d32, d64)
        print(f"gin_edge_emb_grad N={N} D={D} {tname}: {e:.2e} / {b:.2e}")
        assert rc == 0 and e <= b and dE.guards_intact(), (D, tname, e, b)
        rc, dE2 = _emb_grad(g, codes.t, G, D, sum(sizes), len(sizes))
        assert rc == 0 and torch.equal(_bits(dE2.whole), _bits(dE.whole))


def test_emb_grad_refuses_a_short_workspace_and_bad_shapes():
    g, _, _ = _graph("mixed")
    N = g.num_nodes()
    codes = torch.zeros(g.num_edges(), dtype=torch.int32, device=DEV)
    G = torch.zeros((N, 8), device=DEV)
    dE = _Guarded(9, 8)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    rc = lib().mvml_gin_edge_emb_grad(N, ptr(g.in_rowptr), ptr(codes), ptr(G), 8, 8, 9, 2, ptr(dE.t), ptr(ws), 64,
                                      stream_ptr())
    assert rc == 3 and bool((dE.whole == FILL).all())  # MVML_ERR_WORKSPACE
    wp, wn = ws_ptr_size(lib().mvml_gin_emb_grad_workspace_size(N, 300, 1028), DEV)
    for D, R in ((6, 9), (1028, 9), (8, 257)):
        rc = lib().mvml_gin_edge_emb_grad(N, ptr(g.in_rowptr), ptr(codes), ptr(G), 1040, D, R, 2, ptr(dE.t), wp, wn,
                                          stream_ptr())
        assert rc == MVML_ERR_INVALID and bool((dE.whole == FILL).all()), (D, R)
    torch.cuda.synchronize()


# ---- pooling --------------------------------------------------------------------------------------
POOL_OFFSETS = {"mixed": [0, 25, 26, 66, 73, 96, 99, 163, 165, 170], "with_empty": [0, 0, 12, 12, 13, 40, 40],
                "long": [0, 700, 701]}


def _pool(mode, offs, X, D, N=None, argmax=None):
    B = len(offs) - 1
    N = X.shape[0] if N is None else N
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    out = _Guarded(max(B, 1), D + 4)
    arg = torch.full((max(B, 1), D + 8), IFILL, dtype=torch.int32, device=DEV) if argmax is None else argmax
    m = {"sum": 0, "mean": 1, "max": 2}[mode]
    rc = lib().mvml_segment_pool_fwd(B, N, D, m, ptr(od), ptr(X), X.stride(0), ptr(out.t), D + 4, ptr(arg), D + 8,
                                     stream_ptr())
    torch.cuda.synchronize()
    return rc, out, arg, od


def _pool_ref(offs, Xc, mode, arg, Gc, dtype):
    X = Xc.to(dtype).clone().requires_grad_()
    out, own = segment_pool_ref(offs, X, mode, arg)
    out.backward(Gc.to(dtype))
    return out.detach(), X.grad


@pytest.mark.parametrize("D", [4, 64, 68, 300, 1024, 1028, 1800, 2048])
@pytest.mark.parametrize("case", ["mixed", "with_empty", "long"])
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_segment_pool_forward_and_backward(mode, case, D):
    offs = POOL_OFFSETS[case]
    B, N = len(offs) - 1, offs[-1]
    gen = torch.Generator().manual_seed(31 + D)
    Xc, Gc = torch.randn((N, D), generator=gen), torch.randn((B, D), generator=gen)
    sizes = np.diff(offs)
    k = int(np.argmax(sizes))  # a planted tie in the largest molecule: the lowest index must own it
    a = offs[k]
    if sizes[k] >= 3:
        Xc[a + 2, 0] = Xc[a + 1, 0] = 50.0
    X, G = _padded(Xc).to(DEV), _padded(Gc).to(DEV)
    rc, out, arg, od = _pool(mode, offs, X, D)
    assert rc == 0, lib().mvml_last_error()
    own = first_owner(offs, Xc)
    if mode == "max":
        assert torch.equal(arg[:, :D].cpu().long(), own), "argmax: the lowest atom index owns a maximum"
        if sizes[k] >= 3:
            assert int(arg[k, 0]) == a + 1
        assert bool((arg[:, D:] == IFILL).all())
    else:
        assert bool((arg == IFILL).all()), "argmax is written by max alone"
    o64, d64 = _pool_ref(offs, Xc, mode, own, Gc, torch.float64)
    o32, d32 = _pool_ref(offs, Xc, mode, own, Gc, torch.float32)
    e, b = rel_err(out.t[:, :D], o64), _budget(o32, o64)
    assert e <= b and out.guards_intact() and bool((out.t[:, D:] == FILL).all()), (e, b)
    for gi in np.nonzero(sizes == 0)[0]:
        assert float(out.t[gi, :D].abs().max()) == 0.0 and (mode != "max" or bool((arg[gi, :D] == -1).all()))
    gX = _Guarded(max(N, 1), D + 4)
    rc = lib().mvml_segment_pool_bwd(B, N, D, {"sum": 0, "mean": 1, "max": 2}[mode], ptr(od), ptr(G), G.stride(0), ptr(arg),
                                     D + 8, ptr(gX.t), D + 4, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().mvml_last_error()
    e, b = rel_err(gX.t[:, :D], d64), _budget(d32, d64)
    print(f"segment_pool {mode} {case} D={D}: bwd {e:.2e} / {b:.2e}")
    assert bool(torch.isfinite(gX.t[:, :D]).all()), "every gX row is written"
    assert e <= b and gX.guards_intact() and bool((gX.t[:, D:] == FILL).all()), (e, b)
    rc, out2, arg2, _ = _pool(mode, offs, X, D)
    assert rc == 0 and torch.equal(_bits(out2.whole), _bits(out.whole)) and torch.equal(arg2, arg)


@pytest.mark.parametrize("why", ["D%4", "D>2048", "mode", "misaligned X", "out is X", "no argmax"])
def test_pool_refusals_leave_the_buffers_untouched(why):
    offs, D, mode = [0, 3, 5], 8, 2
    X = torch.zeros(5 * 2064 + 4, device=DEV)
    Xv = X[:5 * 2064].view(5, 2064)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    out = _Guarded(2, 2064)
    arg = torch.full((2, 2064), IFILL, dtype=torch.int32, device=DEV)
    op, ap = out.t, arg
    if why == "D%4":
        D = 10
    elif why == "D>2048":
        D = 2052
    elif why == "mode":
        mode = 3
    elif why == "misaligned X":
        Xv = X[1:5 * 2064 + 1].view(5, 2064)
    elif why == "out is X":
        op = Xv
    elif why == "no argmax":
        ap = None
    rc = lib().mvml_segment_pool_fwd(2, 5, D, mode, ptr(od), ptr(Xv), 2064, ptr(op), 2064, ptr(ap), 2064, stream_ptr())
    torch.cuda.synchronize()
    assert rc == MVML_ERR_INVALID and lib().mvml_last_error(), why
    assert bool((out.whole == FILL).all()) and bool((arg == IFILL).all()) and float(X.abs().max()) == 0.0, why


@pytest.mark.parametrize("n", [0, 1, 3, 4, 1000, 1027])
def test_relu_f32(n):
    x = torch.randn(max(n, 1), generator=torch.Generator().manual_seed(n)).to(DEV)[:n]
    if n >= 3:
        x[1], x[2] = -0.0, float("nan")
    y = _Guarded(1, max(n, 1))
    rc = lib().mvml_relu_f32(n, ptr(x), ptr(y.t), stream_ptr())
    torch.cuda.synchronize()
    want = torch.where(x > 0, x, torch.zeros_like(x))
    assert rc == 0 and torch.equal(_bits(y.t.view(-1)[:n]), _bits(want)) and y.guards_intact()
    assert bool((y.t.view(-1)[n:] == FILL).all())
    rc = lib().mvml_relu_f32(n, ptr(x), ptr(x), stream_ptr())  # in place
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(_bits(x), _bits(want))
