"""Microbenchmark of GIN's kernels (csrc/gin_agg.hip, csrc/segment_pool.hip) and modules on one GPU.

Kernels in isolation, on the config-3 batch with seeded bond categories in [0, 6) x [0, 3) (R = 9
table rows) and atom categories in [0, 120) x [0, 3) with 80 % of the atoms on one row (carbon), at
D = 64, 300, 1024: ms per launch, GB/s against the algorithmic bytes (functional.gin_agg_fwd_bytes
etc.) and the fraction of 8 TB/s.

mvml_gin_agg_fwd is timed interleaved with two yardsticks that exist without it:
  * mvml_gcn_agg with NULL scales at the same width on the same graph (the same gather, no edge term);
  * the unfused composition: that call, then the edge term as its own pass written here,
    out += C E with C [N, 12] the per-atom counts of the 9 table rows (made once, outside the timed
    region) on the f32 GEMM with beta = 1;
and with itself under MVML_OPT_GIN_LDS = 0 (every wave reads its table rows from L2 instead of
the workgroup's LDS copy).  At D <= 64 the four-rows-per-wave form against one row per wave
(MVML_OPT_GIN_SUBWAVE), alternating.

Then mvml_gin_edge_emb_grad, mvml_embed_sum_fwd / _bwd and the three pools forward / backward;
one GINLayer D -> D forward + backward and one GINPredictor (5 layers) training step with FlatAdam.

Method (tools/gcn_bench.py's): device events around LAUNCHES back-to-back launches, 3 warm-up
windows, REPS timed windows per variant with the variants of a comparison interleaved; the median
and the min .. max spread are printed, and the device the run was on.

    python tools/gin_bench.py [--mols 65536] [--widths 64,300,1024] [--out profiles/gin_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F_  # noqa: E402

from gcn_bench import row, timed  # noqa: E402
from mvml_gat import FlatAdam, GINLayer, GINPredictor, _lib, bce_with_logits, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

EDGE_TABLES, NODE_TABLES = [6, 3], [120, 3]


def categories(g):
    gen = torch.Generator().manual_seed(0)
    N, E = g.num_nodes(), g.num_edges()
    ec = [torch.randint(0, s, (E,), generator=gen, dtype=torch.int32).cuda() for s in EDGE_TABLES]
    z = torch.randint(0, NODE_TABLES[0], (N,), generator=gen, dtype=torch.int32)
    z[torch.rand(N, generator=gen) < 0.8] = 5  # carbon
    nc = [z.cuda(), torch.randint(0, NODE_TABLES[1], (N,), generator=gen, dtype=torch.int32).cuda()]
    return nc, ec


def table_args(cats, sizes):
    T = len(sizes)
    return (T, *[ptr(c) for c in cats], *[None] * (4 - T), *sizes, *[0] * (4 - T))


def bench_kernels(g, D, nc, ec):
    st = _lib.stream_ptr()
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    R, T, Rn = sum(EDGE_TABLES), len(EDGE_TABLES), sum(NODE_TABLES)
    torch.manual_seed(0)
    X = torch.randn((N, D), device="cuda") * 0.3
    G = torch.randn((N, D), device="cuda")
    Gb = torch.randn((B, D), device="cuda")
    tab = torch.randn((R, D), device="cuda") * 0.1
    ntab = torch.randn((Rn, D), device="cuda") * 0.1
    out, out2 = torch.empty((N, D), device="cuda"), torch.empty((N, D), device="cuda")
    rows = torch.empty(N, dtype=torch.int32, device="cuda")
    codes = Fn.gin_edge_codes(g, ec, EDGE_TABLES)
    # the composition's count matrix [N, 12] (9 rows, K padded to 4 q) and its table, made once
    slot_dst = torch.repeat_interleave(torch.arange(N, device="cuda"), (g.in_rowptr[1:] - g.in_rowptr[:-1]).long())
    C = torch.zeros((N, 12), device="cuda")
    for t in range(T):
        C.index_put_((slot_dst, ((codes[:E] >> (8 * t)) & 255).long()), torch.ones(E, device="cuda"), accumulate=True)
    tab12 = torch.zeros((12, D), device="cuda")
    tab12[:R] = tab
    fby, gby = Fn.gin_agg_fwd_bytes(N, E, D, R), Fn.gcn_agg_bytes(N, E, D)

    def fused():
        call("mvml_gin_agg_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(codes), ptr(X), D, D, ptr(tab), D, R, T,
             ptr(out), D, None, ptr(rows), st)

    def fused_l2():
        with _lib.option("gin_lds", 0):
            fused()

    def gcn():
        call("mvml_gcn_agg", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(X), D, D, None, None, None, 0, ptr(out2), D, None,
             ptr(rows), st)

    def composition():
        gcn()
        Fn.gemm(C, tab12, N, D, 12, 0, 1, 12, D, out2, D, beta=1.0, algo="f32")

    fused(), composition()
    torch.cuda.synchronize()
    err = float((out - out2).abs().max() / out.abs().max())
    assert err < 1e-5, err  # the composition computes the same function
    res = {"composition_rel_diff": err}
    t = timed({"fused": fused, "gcn": gcn, "composition": composition, "fused_l2": fused_l2})
    res["fused"] = row(f"gin_agg_fwd D={D} R={R} (tables in LDS)", t["fused"], fby)
    res["fused_l2"] = row(f"gin_agg_fwd D={D} R={R} (tables from L2)", t["fused_l2"], fby)
    res["gcn"] = row(f"gcn_agg D={D} NULL scales (+ row max)", t["gcn"], gby)
    res["composition"] = row(f"gcn_agg + count GEMM (K = 12) D={D}", t["composition"], gby + 4 * (2 * N * D + 12 * N))
    res["fused_over_gcn"] = t["fused"][0] / t["gcn"][0]
    res["fused_over_composition"] = t["fused"][0] / t["composition"][0]
    res["lds_over_l2"] = t["fused"][0] / t["fused_l2"][0]
    print(f"  fused / gcn_agg time: {res['fused_over_gcn']:.3f} (bytes {fby / gby:.3f});  fused / composition: "
          f"{res['fused_over_composition']:.3f};  LDS / L2 tables: {res['lds_over_l2']:.3f}", flush=True)

    if D <= 64:
        def one_row():
            with _lib.option("gin_subwave", 0):
                fused()
        t = timed({"sub": fused, "row": one_row})
        res["fused_subwave"] = row(f"gin_agg_fwd D={D}, four rows per wave", t["sub"], fby)
        res["fused_one_row"] = row(f"gin_agg_fwd D={D}, one row per wave", t["row"], fby)
        res["subwave_over_one_row"] = t["sub"][0] / t["row"][0]
        print(f"  sub-wave / one-row time: {res['subwave_over_one_row']:.3f}", flush=True)

    dE = torch.empty((R, D), device="cuda")
    dT = torch.empty((Rn, D), device="cuda")
    wp, wn = _lib.ws_ptr_size(max(_lib.lib().mvml_gin_emb_grad_workspace_size(N, R, D),
                                  _lib.lib().mvml_gin_emb_grad_workspace_size(N, Rn, D)), "cuda")
    nargs = table_args(nc, NODE_TABLES)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    kern = {
        "edge_emb_grad": (lambda: call("mvml_gin_edge_emb_grad", N, ptr(g.in_rowptr), ptr(codes), ptr(G), D, D, R, T,
                                       ptr(dE), wp, wn, st), Fn.gin_edge_emb_grad_bytes(N, E, D, R)),
        "embed_sum_fwd": (lambda: call("mvml_embed_sum_fwd", N, *nargs, ptr(ntab), D, D, ptr(out), D, ptr(status), st),
                          Fn.embed_sum_fwd_bytes(N, 2, D, Rn)),
        "embed_sum_bwd": (lambda: call("mvml_embed_sum_bwd", N, *nargs, ptr(G), D, D, ptr(dT), wp, wn, st),
                          Fn.embed_sum_bwd_bytes(N, 2, D, Rn)),
    }
    pooled = torch.empty((B, D), device="cuda")
    arg = torch.empty((B, D), dtype=torch.int32, device="cuda")
    for mode, m in Fn.POOL_MODES.items():
        by = Fn.segment_pool_bytes(B, N, D, mode)
        kern[f"pool_{mode}_fwd"] = (lambda m=m: call("mvml_segment_pool_fwd", B, N, D, m, ptr(g.node_offsets), ptr(X), D,
                                                     ptr(pooled), D, ptr(arg), D, st), by)
        kern[f"pool_{mode}_bwd"] = (lambda m=m: call("mvml_segment_pool_bwd", B, N, D, m, ptr(g.node_offsets), ptr(Gb), D,
                                                     ptr(arg), D, ptr(out), D, st), by)
    kern["pool_max_fwd"][0]()  # arg for the backward
    t = timed({k: v[0] for k, v in kern.items()})
    for k, (_, by) in kern.items():
        res[k] = row(f"{k} D={D}", t[k], by)
    return res


def bench_modules(g, nc, ec, D, layers):
    res = {}
    N = g.num_nodes()
    X = torch.randn((N, D), device="cuda") * 0.3
    go = torch.randn((N, D), device="cuda")
    torch.manual_seed(0)
    layer = GINLayer(EDGE_TABLES, D, activation=F_.relu).cuda()
    x = X.detach().requires_grad_()
    model = GINPredictor(NODE_TABLES, EDGE_TABLES, num_layers=layers, emb_dim=D, n_tasks=11).cuda()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    y = (torch.rand((g.batch_size, 11), device="cuda") > 0.5).float()

    def train_step():
        opt.zero_grad()
        bce_with_logits(model(g, nc, ec), y).backward()
        opt.step()

    steps = {f"GINLayer {D}->{D} fwd+bwd": lambda: layer(g, x, ec).backward(go),
             f"GINPredictor({layers} x {D}) training step": train_step}
    t = timed(steps, launches=3, reps=7, warm=2)
    for k in steps:
        res[k] = row(k, t[k])
    res["peak_GB"] = torch.cuda.max_memory_allocated() / 1e9
    print(f"  peak device memory: {res['peak_GB']:.1f} GB", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--widths", default="64,300,1024")
    ap.add_argument("--module-width", type=int, default=300)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gin_bench: needs a GPU (no timing is taken on the CPU)")
    props = torch.cuda.get_device_properties(0)
    box = f"{props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs"
    sb = synth.config3(a.mols)
    g = sb.to_graph().to("cuda")
    nc, ec = categories(g)
    print(f"device: {box}\nconfig3: {a.mols} molecules, N={g.num_nodes()}, E={g.num_edges()}", flush=True)
    result = {"device": box, "mols": a.mols, "N": g.num_nodes(), "E": g.num_edges()}
    for D in (int(w) for w in a.widths.split(",")):
        result[f"D{D}"] = bench_kernels(g, D, nc, ec)
    if not a.no_modules:
        result["modules"] = bench_modules(g, nc, ec, a.module_width, a.layers)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
