"""Microbenchmark of SAGEConv's neighbour maximum (mvml_sage_max_fwd / mvml_sage_max_bwd,
csrc/sage_agg.hip) and of the GraphSAGE modules on one GPU.

Kernels in isolation, on the config-3 batch, at D = 64, 192, 384: ms per launch, GB/s against the
algorithmic bytes (functional.sage_max_fwd_bytes = 4 (3 N D + N + 1 + E): X read, out and arg
written; functional.sage_max_bwd_bytes = 4 ((3 + gate) N D + N + 1 + 2 E): G, arg and the gate read,
gX written) and the fraction of 8 TB/s.  Interleaved with them mvml_gcn_agg at the same width on
the same graph (functional.gcn_agg_bytes): the peer that gathers the same rows and stores one row
less (no arg).  At D = 64 the sub-wave forms against one row per wave (MVML_OPT_SAGE_SUBWAVE),
alternating.

Modules: one SAGEConv 64 -> 64 forward + backward per aggregator, and one GraphSAGEPredictor(74)
training step (forward, BCE, backward, FlatAdam).

Method (tools/gcn_bench.py's): device events around LAUNCHES back-to-back launches, 3 warm-up
windows, REPS timed windows per variant with the variants of a comparison interleaved; the median
and the min .. max spread are printed, and the device the run was on.

    python tools/sage_bench.py [--mols 65536] [--out profiles/sage_bench.json]
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
from mvml_gat import FlatAdam, GraphSAGEPredictor, SAGEConv, _lib, bce_with_logits, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402


def bench_kernel(g, D):
    st = _lib.stream_ptr()
    N, E = g.num_nodes(), g.num_edges()
    torch.manual_seed(0)
    X = torch.relu(torch.randn((N, D), device="cuda") * 0.3)  # a ReLU output, as fc_pool's
    G = torch.randn((N, D), device="cuda")
    out, gX = torch.empty((N, D), device="cuda"), torch.empty((N, D), device="cuda")
    arg = torch.empty((N, D), dtype=torch.int32, device="cuda")
    rows = torch.empty(N, dtype=torch.int32, device="cuda")
    fby, bby, gby = Fn.sage_max_fwd_bytes(N, E, D), Fn.sage_max_bwd_bytes(N, E, D, True), Fn.gcn_agg_bytes(N, E, D)

    def fwd():
        call("mvml_sage_max_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(X), D, D, ptr(out), D, ptr(arg), D, None,
             ptr(rows), st)

    def bwd():
        call("mvml_sage_max_bwd", N, ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(G), D, ptr(arg), D, D,
             ptr(X), D, ptr(gX), D, st)

    def gcn(transpose=False):
        rp, nb = (g.out_rowptr, g.out_dst) if transpose else (g.in_rowptr, g.in_src)
        return lambda: call("mvml_gcn_agg", N, ptr(rp), ptr(nb), ptr(X), D, D, None, None, None, 0, ptr(out), D, None,
                            ptr(rows), st)

    fwd()  # arg for the backward
    res = {}
    t = timed({"max_fwd": fwd, "gcn_fwd": gcn(), "max_bwd": bwd, "gcn_T": gcn(True)})
    res["max_fwd"] = row(f"sage_max_fwd D={D} (+ arg, row max)", t["max_fwd"], fby)
    res["gcn_fwd"] = row(f"gcn_agg D={D} none fwd (+ row max)", t["gcn_fwd"], gby)
    res["max_bwd"] = row(f"sage_max_bwd D={D} gated", t["max_bwd"], bby)
    res["gcn_T"] = row(f"gcn_agg D={D} none out-CSR (+ row max)", t["gcn_T"], gby)
    res["max_fwd_over_gcn"] = t["max_fwd"][0] / t["gcn_fwd"][0]
    res["max_bwd_over_gcn_T"] = t["max_bwd"][0] / t["gcn_T"][0]
    res["fwd_bytes_over_gcn"] = fby / gby
    res["bwd_bytes_over_gcn"] = bby / gby
    print(f"  max fwd / gcn fwd time: {res['max_fwd_over_gcn']:.3f} (bytes {fby / gby:.3f});  "
          f"max bwd / gcn out-CSR time: {res['max_bwd_over_gcn_T']:.3f} (bytes {bby / gby:.3f})", flush=True)
    if D <= 64:
        def form(fn, v):
            def run():
                with _lib.option("sage_subwave", v):
                    fn()
            return run
        t = timed({"fwd_sub": form(fwd, 1), "fwd_row": form(fwd, 0), "bwd_sub": form(bwd, 1), "bwd_row": form(bwd, 0)})
        res["fwd_subwave"] = row(f"sage_max_fwd D={D}, four rows per wave", t["fwd_sub"], fby)
        res["fwd_one_row"] = row(f"sage_max_fwd D={D}, one row per wave", t["fwd_row"], fby)
        res["bwd_subwave"] = row(f"sage_max_bwd D={D}, four rows per wave", t["bwd_sub"], bby)
        res["bwd_one_row"] = row(f"sage_max_bwd D={D}, one row per wave", t["bwd_row"], bby)
        res["fwd_subwave_over_one_row"] = t["fwd_sub"][0] / t["fwd_row"][0]
        res["bwd_subwave_over_one_row"] = t["bwd_sub"][0] / t["bwd_row"][0]
        print(f"  sub-wave / one-row time: fwd {res['fwd_subwave_over_one_row']:.3f}, "
              f"bwd {res['bwd_subwave_over_one_row']:.3f}", flush=True)
    return res


def bench_modules(g, feats):
    res = {}
    N = g.num_nodes()
    X2 = torch.randn((N, 64), device="cuda") * 0.3
    go = torch.randn((N, 64), device="cuda")
    steps = {}
    for aggr in Fn.SAGE_AGGREGATORS:
        torch.manual_seed(0)
        conv = SAGEConv(64, 64, aggr, activation=F_.relu).cuda()
        x = X2.detach().requires_grad_()
        steps[f"SAGEConv 64->64 {aggr} fwd+bwd"] = (lambda conv=conv, x=x: conv(g, x).backward(go))
    torch.manual_seed(0)
    model = GraphSAGEPredictor(74, n_tasks=11).cuda()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    y = (torch.rand((g.batch_size, 11), device="cuda") > 0.5).float()

    def train_step():
        opt.zero_grad()
        bce_with_logits(model(g, feats), y).backward()
        opt.step()
    steps["GraphSAGEPredictor(74) training step"] = train_step
    t = timed(steps, launches=3, reps=7, warm=2)
    for k in steps:
        res[k] = row(k, t[k])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--widths", default="64,192,384")
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sage_bench: needs a GPU (no timing is taken on the CPU)")
    props = torch.cuda.get_device_properties(0)
    box = f"{props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs"
    sb = synth.config3(a.mols)
    g = sb.to_graph().to("cuda")
    print(f"device: {box}\nconfig3: {a.mols} molecules, N={g.num_nodes()}, E={g.num_edges()}", flush=True)
    result = {"device": box, "mols": a.mols, "N": g.num_nodes(), "E": g.num_edges()}
    for D in (int(w) for w in a.widths.split(",")):
        result[f"D{D}"] = bench_kernel(g, D)
    if not a.no_modules:
        result["modules"] = bench_modules(g, g.ndata["h"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
