"""Layer 1 over the distinct atom-feature rows: the class map (mvml_feat_classes) against
numpy.unique, the row-mapped aggregation entries against the plain ones, and the GAT layer /
GNNModule on the mapped path against the materialised path of the same library, bit for bit.

Shapes are small (8-12 molecules, a few hundred atoms, H = 4 and F = 8 / 16, one H = 1 case): the
map changes which row an address points at, never the arithmetic, so every comparison here is
torch.equal — there is no tolerance to size.  The oracle comparison of the model-level test keeps
the bar of test_gpu_parity_configs.py (1e-5, or 4 x the fp32 oracle's own error).
"""

import numpy as np
import pytest
import torch

from _util import batch_of_sizes, graph_dict, model_pair, randomize_
from conftest import rel_err
from mvml_gat import _lib, batching
from mvml_gat import functional as Fn
from mvml_gat._lib import option, ptr
from mvml_gat.nn import GATLayer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = batching.L_MAX_CLASSES
TOL = 1e-5


# ------------------------------------------------------------------------------ class build
def _build(X):
    """(cls, Xc, count) of mvml_feat_classes on the rows of X (numpy float32 [N, ld])."""
    n, ld = X.shape
    Xd = torch.as_tensor(X).to(DEV).contiguous()
    cls = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    Xc = torch.zeros((CAP, ld), dtype=torch.float32, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    wp, wn = _lib.ws_ptr_size(_lib.lib().mvml_feat_classes_workspace_size(), torch.device(DEV))
    _lib.call("mvml_feat_classes", n, ptr(Xd) if n else None, ld, ptr(cls), ptr(Xc), ptr(cnt), wp, wn,
              _lib.stream_ptr(torch.device(DEV)))
    return cls[:n].cpu().numpy(), Xc.cpu().numpy(), int(cnt.item())


def _unique_first(X):
    """numpy.unique over whole rows compared by bits, classes re-ordered by first occurrence."""
    bits = np.ascontiguousarray(X).view(np.uint32)
    _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)            # unique's class -> rank by first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return rank[inv.reshape(-1)], X[np.sort(first)]


def _rows(kind, rng):
    base = rng.standard_normal((1, 76)).astype(np.float32)
    base[:, 74:] = 0.0
    if kind == "one_class":
        return np.repeat(base, 300, 0)
    if kind == "all_distinct":
        return rng.standard_normal((300, 76)).astype(np.float32)
    if kind in ("last_real_column", "pad_column"):
        X = np.repeat(base, 300, 0)
        X[:, 73 if kind == "last_real_column" else 75] = rng.integers(0, 3, 300).astype(np.float32)
        return X
    if kind == "signed_zero":
        X = np.repeat(base, 300, 0)
        X[:, 5] = np.where(rng.random(300) < 0.5, 0.0, -0.0).astype(np.float32)
        return X
    if kind in ("capacity", "capacity_plus_one"):
        c = CAP + (kind == "capacity_plus_one")
        X = np.zeros((3 * c, 8), dtype=np.float32)
        X[:, 0] = rng.permutation(np.arange(3 * c) % c)
        return X
    if kind == "featurizer":  # one-hot blocks and small integers, a few dozen classes
        X = np.zeros((700, 76), dtype=np.float32)
        X[np.arange(700), rng.integers(0, 5, 700)] = 1.0
        X[np.arange(700), 43 + rng.integers(0, 4, 700)] = 1.0
        X[:, 60] = rng.integers(0, 3, 700)
        return X
    raise KeyError(kind)


CLASS_CASES = ["one_class", "all_distinct", "last_real_column", "pad_column", "signed_zero", "capacity",
               "featurizer"]


@pytest.mark.parametrize("kind", CLASS_CASES)
def test_class_build_matches_unique(kind):
    X = _rows(kind, np.random.default_rng(3))
    cls, Xc, cnt = _build(X)
    want_cls, want_rows = _unique_first(X)
    assert cnt == len(want_rows)
    assert np.array_equal(cls, want_cls)
    assert np.array_equal(Xc[:cnt].view(np.uint32), want_rows.view(np.uint32))
    if kind == "signed_zero":
        assert cnt == 2
    # a second build of the same input gives the same numbering
    cls2, Xc2, cnt2 = _build(X)
    assert cnt2 == cnt and np.array_equal(cls2, cls) and np.array_equal(Xc2.view(np.uint32), Xc.view(np.uint32))


def test_class_build_over_capacity_and_empty():
    X = _rows("capacity_plus_one", np.random.default_rng(4))
    cls, _, cnt = _build(X)
    assert cnt == CAP + 1 and not cls.any()  # no map: every id stays a valid row
    _, _, cnt0 = _build(np.zeros((0, 76), dtype=np.float32))
    assert cnt0 == 0


# ------------------------------------------------------------------------------ graphs
def _few_class_feats(n, rng, classes=12):
    table = np.zeros((classes, 74), dtype=np.float32)
    table[np.arange(classes), rng.integers(0, 40, classes)] = 1.0
    table[:, 50] = rng.integers(0, 4, classes)
    table[:, 73] = rng.random(classes).astype(np.float32)
    return table[rng.integers(0, classes, n)]


def _graph(kind, feats="few", seed=0):
    rng = np.random.default_rng(seed)
    if kind == "mixed":      # 10 molecules, one of them a single atom
        sb = batch_of_sizes([25, 1, 40, 7, 23, 3, 64, 2, 5, 31], seed=1)
    elif kind == "empty":    # a molecule without atoms in the batch
        sb = batch_of_sizes([25, 12, 40, 7, 23, 3, 33, 2, 5], seed=2)
        sb = _with_empty_molecule(sb)
    elif kind == "hub":      # one molecule with a hub of in-degree >= 64: big window / fallbacks
        sb = batch_of_sizes([150, 20, 9, 33, 12, 40, 7, 16], seed=7, hubs=True, partners=70)
    elif kind == "many":     # 141 molecules of 64 atoms: 9,024 atoms >= 8 x (capacity + 76)
        sb = batch_of_sizes([64] * 141, seed=3)
    else:
        raise KeyError(kind)
    n = int(sb.num_nodes.sum())
    if isinstance(feats, tuple):  # exactly this many distinct rows, every one of them present
        k = feats[1]
        table = rng.standard_normal((k, 74)).astype(np.float32)
        sb.feats = table[rng.permutation(np.concatenate([np.arange(k), rng.integers(0, k, n - k)]))]
    elif feats == "few":
        sb.feats = _few_class_feats(n, rng)
    elif feats == "distinct":  # every row its own class: N < 8 C, the batch keeps no map
        sb.feats = rng.standard_normal((n, 74)).astype(np.float32)
    return sb


def _with_empty_molecule(sb):
    from mvml_gat.synth import SynthBatch
    nn_ = np.insert(sb.num_nodes, 3, 0)
    ne_ = np.insert(sb.num_edges, 3, 0)
    return SynthBatch(nn_, ne_, sb.src_local, sb.dst_local, sb.feats)


def _run_layer(sb, mapped, H, F, mode, bias=True, residual=True, train=True, link=False, seed=0, expect=None):
    """out, attn and every parameter gradient of one GATLayer on the batch's own feature buffer.
    expect: the path the layer must have taken — "mapped" (the *_map entries ran, forward and
    backward, on a table of C rows; the default with mapped), "plain" (no map asked of the entries;
    the default without), "refused" (the mapped forward entry was called, refused, and the plain
    one ran on the materialised Y)."""
    expect = expect or ("mapped" if mapped else "plain")
    torch.manual_seed(seed)
    layer = GATLayer(74, F, H, agg_mode=mode, activation=torch.nn.functional.elu if mode == "flatten" else None,
                     residual=residual, bias=bias)
    randomize_(layer, seed)
    layer = layer.to(DEV)
    layer.train(train)
    nxt = None
    if link:  # a following layer that claims the ELU link (flatten + ELU feeding the next layer)
        nxt = GATLayer(H * F, 8, 2, agg_mode="mean").to(DEV)
    prev = Fn.FEAT_CLASSES
    Fn.FEAT_CLASSES = mapped
    cap, names = {}, []
    prev_cap = Fn.DEBUG_CAPTURE
    prev_link = (Fn.ELU_LINK[0], Fn.ELU_LINK_POLICY)
    real_call = Fn.call

    def counting_call(name, *args, **kw):
        names.append(name)
        return real_call(name, *args, **kw)

    try:
        g = sb.to_graph().to(DEV)
        assert g.feat_maps == []  # built when the first GAT layer asks, not at upload
        with torch.no_grad():
            layer(g, g.ndata["h"])
        assert len(g.feat_maps) == int(expect != "plain")
        g.recollate()  # the per-step rebuild of the map that now exists
        Fn.DEBUG_CAPTURE, Fn.call = cap, counting_call
        if link:
            Fn.ELU_LINK[0], Fn.ELU_LINK_POLICY = True, "on"
        out = layer(g, g.ndata["h"])
        last = nxt(g, out) if link else out
        gen = torch.Generator().manual_seed(seed + 1)
        last.backward(torch.randn(last.shape, generator=gen).to(DEV))
        torch.cuda.synchronize()
    finally:
        Fn.FEAT_CLASSES, Fn.DEBUG_CAPTURE, Fn.call = prev, prev_cap, real_call
        Fn.ELU_LINK[0], Fn.ELU_LINK_POLICY = prev_link
    # the path taken, positively: layer 1's forward is the first record, its backward the last
    n_map = sum(n_.endswith("_map") for n_ in names)
    took, y_rows = cap["mapped_fwd"][0]
    if expect == "mapped":
        assert took and cap["mapped_bwd"][-1] and n_map == 2 and y_rows == g.feat_maps[0].C < g.num_nodes()
    else:
        assert not took and not cap["mapped_bwd"][-1] and y_rows == g.num_nodes()
        assert n_map == int(expect == "refused")
    res = {"out": out.detach(), "attn": cap["attn"].detach()}
    for n_, p in list(layer.named_parameters()) + ([("next." + k, v) for k, v in nxt.named_parameters()] if link else []):
        res["grad " + n_] = p.grad.detach()
    return res


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


LAYER_CASES = {
    # name: (graph, H, F, mode, layer keywords, options)
    "flatten_elu": ("mixed", 4, 16, "flatten", {}, {}),
    "flatten_elu_linked": ("mixed", 4, 16, "flatten", {"link": True}, {}),
    "mean": ("mixed", 4, 8, "mean", {}, {}),
    "one_head": ("mixed", 1, 16, "flatten", {}, {}),
    "eval": ("mixed", 4, 16, "flatten", {"train": False}, {}),
    "empty_molecule": ("empty", 4, 16, "flatten", {}, {}),
    "dst_wave_fwd": ("mixed", 4, 16, "flatten", {}, {"dst_fwd": 1}),
    "dst_wave_fwd_split_softmax": ("mixed", 4, 16, "flatten", {}, {"dst_fwd": 2}),
    "window_fwd_window_bwd": ("mixed", 4, 32, "flatten", {}, {"dst_fwd": 0, "flat_src": 0, "mean_src": 0}),
    "window_mean": ("mixed", 4, 32, "mean", {}, {"dst_fwd": 0, "mean_src": 0}),
    "hub_big_window": ("hub", 4, 32, "flatten", {}, {"dst_fwd": 0, "flat_src": 0, "big_window": 1}),
    "hub_fallbacks": ("hub", 4, 32, "flatten", {}, {"dst_fwd": 0, "flat_src": 0, "big_window": 0}),
    "hub_mean_fallbacks": ("hub", 4, 32, "mean", {}, {"dst_fwd": 0, "mean_src": 0, "big_window": 0}),
    "atomwise_bwd": ("mixed", 4, 16, "flatten", {}, {"bwd_atomwise": 1, "flat_src": 0}),
    "flat_src_bwd": ("hub", 4, 16, "flatten", {}, {"flat_src": 2}),
    "mean_src_bwd": ("mixed", 4, 16, "mean", {}, {"mean_src": 1}),
}


@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_layer_mapped_equals_materialised(case, monkeypatch):
    kind, H, F, mode, kw, opts = LAYER_CASES[case]
    sb = _graph(kind)
    if "dst_fwd" in opts:  # forced the way test_gpu_parity_configs.py forces the forward
        monkeypatch.setattr(Fn, "DST_FWD_POLICY", "all" if opts["dst_fwd"] else "off")
        monkeypatch.setattr(Fn, "DST_FWD_KIND", opts["dst_fwd"])
    if "flat_src" in opts:
        monkeypatch.setattr(Fn, "FLAT_SRC_AUTO", False)
    import contextlib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(option(k, v))
        a = _run_layer(sb, True, H, F, mode, **kw)
        b = _run_layer(sb, False, H, F, mode, **kw)
    _same(a, b)


@pytest.mark.parametrize("kw", [{"bias": False}, {"residual": False}], ids=["no_bias", "no_residual"])
def test_layer_without_mapped_layout_stays_plain(kw):
    """No row-mapped separate-residual instances: the layer does not ask for the map at all."""
    sb = _graph("mixed")
    _same(_run_layer(sb, True, 4, 16, "flatten", expect="plain", **kw), _run_layer(sb, False, 4, 16, "flatten", **kw))


@pytest.mark.parametrize("kw", [{"bias": False}, {"residual": False}], ids=["no_bias", "no_residual"])
def test_layer_refused_map_falls_back(kw, monkeypatch):
    """A layer that does try such a layout: the entry refuses, the layer materialises Y."""
    monkeypatch.setattr(Fn, "map_layout_ok", lambda sep, bias: True)
    sb = _graph("mixed")
    a = _run_layer(sb, True, 4, 16, "flatten", expect="refused", **kw)
    _same(a, _run_layer(sb, False, 4, 16, "flatten", **kw))


def test_too_few_rows_per_class_keeps_no_map():
    sb = _graph("mixed", feats="distinct")  # N < 8 C
    a = _run_layer(sb, True, 4, 16, "flatten", expect="plain")
    _same(a, _run_layer(sb, False, 4, 16, "flatten"))


@pytest.mark.parametrize("classes", [CAP, CAP + 1, CAP + 76], ids=["capacity", "capacity_plus_one", "well_over"])
def test_capacity_rule_at_graph_level(classes):
    """9,024 atoms (N >= 8 C either way, so only the capacity rule decides): exactly 1024 classes
    carry a map with C = 1024 and the layer is bitwise the plain path; one class more and the batch
    carries none (the build reports capacity + 1 and all-zero ids, which nothing may read)."""
    sb = _graph("many", feats=("classes", classes))
    fits = classes <= CAP
    a = _run_layer(sb, True, 4, 16, "flatten", expect="mapped" if fits else "plain")
    _same(a, _run_layer(sb, False, 4, 16, "flatten"))


def test_mapped_entry_refuses_separate_residual():
    """Called directly: a residual apart from Y's rows returns MVML_ERR_INVALID, nothing written."""
    sb = _graph("mixed")
    g = sb.to_graph().to(DEV)
    N, E, H, F = g.num_nodes(), g.num_edges(), 4, 16
    Y = torch.randn(8, 192, device=DEV)
    yrow = torch.zeros(N, dtype=torch.int32, device=DEV)
    elr = torch.randn(N, 2 * H, device=DEV)
    R = torch.randn(N, H * F, device=DEV)
    out = torch.full((N, H * F), 7.0, device=DEV)
    attn = torch.full((E, H), 7.0, device=DEV)
    bias = torch.zeros(H * F, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    L = _lib.lib()
    rc = L.mvml_gat_agg_fwd_res_map(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src), ptr(Y),
                                    192, H, F, ptr(elr), ptr(R), H * F, ptr(bias), 0.2, 0, ptr(out), ptr(attn), None,
                                    None, st, ptr(yrow))
    assert rc == 1 and b"row map" in L.mvml_last_error()
    gY = torch.full((N, 192), 7.0, device=DEV)
    gR = torch.full((N, H * F), 7.0, device=DEV)
    wp, wn = _lib.ws_ptr_size(L.mvml_gat_agg_bwd_workspace_size(E, H), torch.device(DEV))
    rc = L.mvml_gat_agg_bwd_res_map(N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                                    ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Y), 192, ptr(elr),
                                    ptr(attn), ptr(out), ptr(out), H, F, 0.2, 0, ptr(gY), 192, H * F, ptr(gR), H * F,
                                    None, None, wp, wn, st, ptr(yrow))
    assert rc == 1 and b"row map" in L.mvml_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((attn == 7.0).all()) and bool((gY == 7.0).all())


# ------------------------------------------------------------------------------ model level
def _module_step(sb, mapped, prod):
    prev, Fn.FEAT_CLASSES = Fn.FEAT_CLASSES, mapped
    try:
        g = sb.to_graph().to(DEV)
        prod.zero_grad()
        out = prod(g, g.ndata["h"])
        assert len(g.feat_maps) == int(mapped)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
    finally:
        Fn.FEAT_CLASSES = prev
    return out.detach(), {n: p.grad.detach().clone() for n, p in prod.named_parameters()}, gout


def test_gnn_module_mapped_bitwise_and_oracle():
    sb = _graph("mixed")
    prod, ref = model_pair(hidden=(16, 32), seed=3)
    prod, ref = prod.eval().to(DEV), ref.eval()
    out_m, grads_m, gout = _module_step(sb, True, prod)
    out_p, grads_p, _ = _module_step(sb, False, prod)
    assert torch.equal(out_m, out_p)
    for n in grads_m:
        assert torch.equal(grads_m[n], grads_p[n]), n
    ref32 = type(ref)(74, [16, 32], 0.5, 6, 3).eval()
    ref32.load_state_dict(ref.state_dict())
    ref64 = ref.double()
    gd = graph_dict(sb)
    X = torch.as_tensor(sb.feats, dtype=torch.float64)
    out_r = ref64(gd, X)
    out_r.backward(gout.double())
    ref32(gd, X.float()).backward(gout)
    assert rel_err(out_m, out_r) < TOL
    p64, p32 = dict(ref64.named_parameters()), dict(ref32.named_parameters())
    for n, gr in grads_m.items():
        e, budget = rel_err(gr, p64[n].grad), max(TOL, 4 * rel_err(p32[n].grad, p64[n].grad))
        print(f"{n}: {e:.2e} / {budget:.2e}")
        assert e < budget, (n, e, budget)
