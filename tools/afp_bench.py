"""Microbenchmark of AttentiveFP's kernels (csrc/afp_agg.hip, csrc/gru.hip, csrc/attn_pool.hip) and
of one AttentiveFPPredictor training step on one GPU.

On the config-3 batch with De = 10 seeded bond features, at G = 64, 200, 512: ms per launch, GB/s
against the algorithmic bytes (functional.afp_context_fwd_bytes etc.) and the fraction of 8 TB/s.
  * mvml_afp_context_fwd / _bwd interleaved with mvml_gat_agg_fwd_res / _bwd_res at H = 1 and the
    same width (the later layers' aggregation: comparable bytes, no bond term);
  * mvml_gru_cell_fwd / _bwd on the atom rows and on the graph rows, the forward interleaved with
    mvml_lstm_cell_fwd on the same rows (4D gate columns and a cell state where the GRU has 6D and none);
  * mvml_attn_pool_fwd / _bwd, the forward interleaved with mvml_wsum_max_fwd (the same rows read
    once, a sigmoid gate instead of the softmax, plus the column maximum);
  * one AttentiveFPPredictor(39, 10, graph_feat_size = G) training step with FlatAdam.

Method (tools/gcn_bench.py's): device events around back-to-back launches, warm-up windows, timed
windows per variant with the variants of a comparison interleaved; median and min .. max.

    python tools/afp_bench.py [--mols 65536] [--widths 64,200,512] [--out profiles/afp_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from gcn_bench import row, timed  # noqa: E402
from mvml_gat import AttentiveFPPredictor, FlatAdam, _lib, bce_with_logits, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

FN, DE = 39, 10


def bench_kernels(g, G, e):
    st = _lib.stream_ptr()
    L = _lib.lib()
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    rnd = lambda *s: torch.randn(s, device="cuda")
    rows = Fn.afp_edge_rows(g, e)
    P, t, W1eT, b1, w2e, gs = rnd(N, G), rnd(N), rnd(DE, G) / 3, rnd(G), rnd(G) / G ** 0.5, rnd(N, G)
    s, attn = torch.empty((N, G), device="cuda"), torch.empty(E, device="cuda")
    gP, g_t, g_w2e, g_w1b = torch.empty((N, G), device="cuda"), torch.empty(N, device="cuda"), rnd(G), rnd(DE + 1, G)
    wp, wn = _lib.ws_ptr_size(L.mvml_afp_context_bwd_workspace_size(N, E, G, DE), "cuda")
    elr, out, gat_attn, gY = rnd(N, 2), torch.empty((N, G), device="cuda"), torch.empty((E, 1), device="cuda"), torch.empty((N, G + 4), device="cuda")
    gwp, gwn = _lib.ws_ptr_size(L.mvml_gat_agg_bwd_workspace_size(E, 1), "cuda")

    def ctx_fwd():
        call("mvml_afp_context_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(P), G, G, ptr(rows), DE, ptr(W1eT), ptr(b1),
             ptr(w2e), ptr(t), ptr(s), G, ptr(attn), st)

    def ctx_bwd():
        call("mvml_afp_context_bwd", N, E, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
             ptr(g.out_inslot), ptr(P), G, G, ptr(rows), DE, ptr(W1eT), ptr(b1), ptr(w2e), ptr(t), ptr(s), G, ptr(attn),
             ptr(gs), G, ptr(gP), G, ptr(g_t), ptr(g_w2e), ptr(g_w1b), wp, wn, st)

    def gat_fwd():
        call("mvml_gat_agg_fwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src), ptr(P), G,
             1, G, ptr(elr), None, 0, None, 0.01, 0, ptr(out), ptr(gat_attn), None, None, st)

    def gat_bwd():
        call("mvml_gat_agg_bwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
             ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(P), G, ptr(elr), ptr(gat_attn), ptr(out), ptr(gs), 1, G,
             0.01, 0, ptr(gY), G + 4, G, None, 0, None, None, gwp, gwn, st)

    res = {}
    tm = timed({"ctx_fwd": ctx_fwd, "gat_fwd": gat_fwd})
    res["context_fwd"] = row(f"afp_context_fwd G={G} De={DE}", tm["ctx_fwd"], Fn.afp_context_fwd_bytes(N, E, G, DE))
    res["gat_fwd"] = row(f"gat_agg_fwd_res H=1 F={G}", tm["gat_fwd"], Fn.agg_fwd_bytes(N, E, 1, G, G, 0))
    tm = timed({"ctx_bwd": ctx_bwd, "gat_bwd": gat_bwd})
    res["context_bwd"] = row(f"afp_context_bwd G={G} De={DE}", tm["ctx_bwd"], Fn.afp_context_bwd_bytes(N, E, G, DE))
    res["gat_bwd"] = row(f"gat_agg_bwd_res H=1 F={G}", tm["gat_bwd"], Fn.agg_bwd_bytes(N, E, 1, G, G, 0))

    for M, what in ((N, "atoms"), (B, "graphs")):
        gi, gh, bi, bh, h = rnd(M, 3 * G), rnd(M, 3 * G), rnd(3 * G), rnd(3 * G), rnd(M, G)
        o, save, go = torch.empty((M, G), device="cuda"), torch.empty((M, 4 * G), device="cuda"), rnd(M, G)
        g_gi, g_gh, g_h = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)

        def gru_fwd():
            call("mvml_gru_cell_fwd", M, G, ptr(gi), ptr(gh), ptr(bi), ptr(bh), ptr(h), G, 1, ptr(o), G, ptr(save), st)

        def gru_bwd():
            call("mvml_gru_cell_bwd", M, G, ptr(save), ptr(h), G, ptr(o), G, ptr(go), G, 1, ptr(g_gi), ptr(g_gh), ptr(g_h), G, st)
        gp, lbi, lbh, cp = rnd(M, 4 * G), rnd(4 * G), rnd(4 * G), rnd(M, G)
        co, ho, act = torch.empty_like(cp), torch.empty_like(cp), torch.empty_like(gp)

        def lstm_fwd():
            call("mvml_lstm_cell_fwd", M, G, ptr(gp), ptr(lbi), ptr(lbh), ptr(cp), ptr(co), ptr(ho), G, ptr(act), None, 0, st)
        tm = timed({"f": gru_fwd, "lstm": lstm_fwd, "b": gru_bwd})
        res[f"lstm_fwd_{what}"] = row(f"lstm_cell_fwd M={M} D={G}", tm["lstm"], 4 * M * G * (4 + 1 + 1 + 1 + 4))
        res[f"gru_fwd_{what}"] = row(f"gru_cell_fwd M={M} D={G}", tm["f"], Fn.gru_cell_bytes(M, G, False))
        res[f"gru_bwd_{what}"] = row(f"gru_cell_bwd M={M} D={G}", tm["b"], Fn.gru_cell_bytes(M, G, True))

    X, wn_, u, gr = rnd(N, G), rnd(G) / G ** 0.5, rnd(B), rnd(B, G)
    r, a, gX, g_u, g_wn = torch.empty((B, G), device="cuda"), torch.empty(N, device="cuda"), torch.empty((N, G), device="cuda"), rnd(B), rnd(G)
    pwp, pwn = _lib.ws_ptr_size(L.mvml_attn_pool_bwd_workspace_size(B, N, G), "cuda")

    def pool_fwd():
        call("mvml_attn_pool_fwd", B, N, G, ptr(g.node_offsets), ptr(X), G, ptr(wn_), ptr(u), 0.01, ptr(r), G, ptr(a), st)

    def pool_bwd():
        call("mvml_attn_pool_bwd", B, N, G, ptr(g.node_offsets), ptr(X), G, ptr(wn_), ptr(u), 0.01, ptr(r), G, ptr(a), ptr(gr),
             G, 0, ptr(gX), G, ptr(g_u), ptr(g_wn), pwp, pwn, st)
    wbias, wout = rnd(1), torch.empty((B, 2 * G), device="cuda")
    gate, amax = torch.empty(N, device="cuda"), torch.empty((B, G), dtype=torch.int32, device="cuda")

    def wsum_fwd():
        call("mvml_wsum_max_fwd", B, N, G, ptr(g.node_offsets), ptr(X), G, ptr(wn_), ptr(wbias), ptr(wout), 2 * G, ptr(gate),
             ptr(amax), G, st)
    tm = timed({"f": pool_fwd, "w": wsum_fwd, "b": pool_bwd})
    res["wsum_max_fwd"] = row(f"wsum_max_fwd D={G}", tm["w"], 4 * (N * G + 3 * B * G + N + B))
    res["attn_pool_fwd"] = row(f"attn_pool_fwd D={G}", tm["f"], Fn.attn_pool_bytes(B, N, G, False))
    res["attn_pool_bwd"] = row(f"attn_pool_bwd D={G}", tm["b"], Fn.attn_pool_bytes(B, N, G, True))
    return res


def bench_step(g, G, x, e):
    torch.manual_seed(0)
    model = AttentiveFPPredictor(FN, DE, graph_feat_size=G, n_tasks=11).cuda().train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    y = (torch.rand(g.batch_size, 11, device="cuda") < 0.5).float()

    def step():
        opt.zero_grad()
        bce_with_logits(model(g, x, e), y).backward()
        opt.step()
    tm = timed({"step": step}, launches=3, reps=7, warm=2)
    return {"step": row(f"AttentiveFPPredictor G={G} step (FlatAdam)", tm["step"]),
            "max_memory_gb": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--widths", default="64,200,512")
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sb = synth.config3(a.mols)
    g = sb.to_graph().to("cuda")
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((g.num_nodes(), FN), generator=gen).cuda()
    e = torch.randn((g.num_edges(), DE), generator=gen).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}; {g.batch_size} molecules, {g.num_nodes()} atoms, {g.num_edges()} edges")
    res = {}
    for G in (int(w) for w in a.widths.split(",")):
        res[f"G{G}"] = bench_kernels(g, G, e)
        if not a.no_modules:
            res[f"G{G}"].update(bench_step(g, G, x, e))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
