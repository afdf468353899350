"""Microbenchmark of D-MPNN's bond-state kernels (csrc/dmpnn.hip) and of one DMPNNPredictor training
step on one GPU.

On the config-3 batch with De = 14 seeded bond features, at hidden sizes 64 and 300:
  * mvml_dmpnn_update and its adjoint, mvml_dmpnn_init_fwd, mvml_dmpnn_atom_sum and its adjoint: ms per
    launch and the algorithmic bytes (functional.dmpnn_*_bytes) as a share of the 8 TB/s HBM peak;
  * beside them the W_h product R = M W_h^T over the E slot rows on the project's GEMM (its A, B and C
    once as bytes), and mvml_gcn_agg at the same width, the yardstick among the row kernels;
  * one DMPNNPredictor(39, 14, D, depth 3) training step with FlatAdam.

Method (tools/gcn_bench.py's): device events around back-to-back launches, warm-up windows, timed
windows per variant with the variants interleaved; median and min .. max.

    python tools/dmpnn_bench.py [--mols 65536] [--sizes 64,300] [--out profiles/dmpnn_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from gcn_bench import row, timed  # noqa: E402
from mvml_gat import DMPNNPredictor, FlatAdam, _lib, bce_with_logits, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

FN, DE = 39, 14


def bench_kernels(g, D):
    st = _lib.stream_ptr()
    N, E = g.num_nodes(), g.num_edges()
    rnd = lambda *s: torch.randn(s, device="cuda")
    new = lambda *s: torch.empty(s, device="cuda")
    M, R, inp, go, b = rnd(E, D).relu_(), rnd(E, D), rnd(E, D), rnd(E, D), rnd(D)
    W, P, WieT, ga, X = rnd(D, D) / D ** 0.5, rnd(N, D), rnd(DE, D), rnd(N, D), rnd(N, D)
    rows = Fn.afp_edge_rows(g, rnd(E, DE))
    out, dR, dpre, inp2, M0, a, dM, Rg, agg = new(E, D), new(E, D), new(E, D), new(E, D), new(E, D), new(N, D), new(E, D), new(E, D), new(N, D)
    rev, csr = Fn.dmpnn_rev_slots(g), (ptr(g.in_rowptr), ptr(g.out_rowptr), ptr(g.out_inslot))
    call("mvml_dmpnn_update", N, E, *csr, ptr(rev), ptr(R), D, ptr(inp), D, ptr(b), D, ptr(out), D, st)
    calls = {
        "update": lambda: call("mvml_dmpnn_update", N, E, *csr, ptr(rev), ptr(R), D, ptr(inp), D, ptr(b), D, ptr(out), D, st),
        "update_bwd": lambda: call("mvml_dmpnn_update_bwd", N, E, *csr, ptr(rev), ptr(out), D, ptr(go), D, D, ptr(dR), D,
                                   ptr(dpre), D, st),
        "init": lambda: call("mvml_dmpnn_init_fwd", N, E, ptr(g.in_src), ptr(P), D, D, ptr(rows), DE, ptr(WieT), ptr(b),
                             ptr(inp2), D, ptr(M0), D, st),
        "atom_sum": lambda: call("mvml_dmpnn_atom_sum", N, E, csr[0], None, ptr(M), D, D, ptr(a), D, st),
        "atom_sum_bwd": lambda: call("mvml_dmpnn_atom_sum_bwd", N, E, csr[0], ptr(ga), D, D, ptr(dM), D, st),
        "gemm_wh": lambda: Fn.gemm(M, W, E, D, D, 0, 0, D, D, Rg, D),
        "gcn_agg": lambda: call("mvml_gcn_agg", N, csr[0], ptr(g.in_src), ptr(X), D, D, None, None, None, 0, ptr(agg), D,
                                None, None, st),
    }
    by = {"update": Fn.dmpnn_update_bytes(N, E, D), "update_bwd": Fn.dmpnn_update_bytes(N, E, D, True),
          "init": Fn.dmpnn_init_bytes(N, E, D, DE), "atom_sum": Fn.dmpnn_atom_sum_bytes(N, E, D),
          "atom_sum_bwd": Fn.dmpnn_atom_sum_bytes(N, E, D), "gemm_wh": 4 * (2 * E * D + D * D),
          "gcn_agg": Fn.gcn_agg_bytes(N, E, D)}
    tm = timed(calls, launches=4, reps=7, warm=2)
    return {k: row(f"{k} D={D}", tm[k], by[k]) for k in calls}


def bench_step(g, D, x, e):
    torch.manual_seed(0)
    model = DMPNNPredictor(FN, DE, hidden_size=D, depth=3, n_tasks=11).cuda().train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    y = (torch.rand(g.batch_size, 11, device="cuda") < 0.5).float()

    def step():
        opt.zero_grad()
        bce_with_logits(model(g, x, e), y).backward()
        opt.step()
    tm = timed({"step": step}, launches=2, reps=5, warm=1)
    return {"step": row(f"DMPNNPredictor D={D} depth=3 step (FlatAdam)", tm["step"]),
            "max_memory_gb": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--sizes", default="64,300")
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = synth.config3(a.mols).to_graph().to("cuda")
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((g.num_nodes(), FN), generator=gen).cuda()
    e = torch.randn((g.num_edges(), DE), generator=gen).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}; {g.batch_size} molecules, {g.num_nodes()} atoms, {g.num_edges()} edges")
    res = {}
    for D in (int(v) for v in a.sizes.split(",")):
        res[f"D{D}"] = bench_kernels(g, D)
        torch.cuda.empty_cache()
        if not a.no_modules:
            res[f"D{D}"].update(bench_step(g, D, x, e))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
