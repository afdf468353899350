"""Microbenchmark of the GCN aggregation (mvml_gcn_agg, csrc/gcn_agg.hip) and of the GCN modules
on one GPU.

Kernel in isolation, on the config-3 batch: mvml_gcn_agg at D = 64, 192, 384 for norm 'none' (no
scales) and 'both' (both scales), forward CSR and the swapped (out-CSR) call; ms per launch, GB/s
against the algorithmic bytes 4 (2 N D + N + 1 + E + 2 N) (functional.gcn_agg_bytes) and the
fraction of 8 TB/s.  Next to it mvml_gat_agg_fwd_res at H = 1, F = D, mode 2 on the same graph in
the same process: the destination-wave GAT kernel doing strictly more work (a softmax and the
attention store) on the same gather.  At D = 64 the sub-wave form against one row per wave
(MVML_OPT_GCN_SUBWAVE), alternating.

Whole layer: one GCNLayer forward + backward at GCN's default widths, and one GCNPredictor training
step (forward, BCE, backward, FlatAdam).

Method: device events around LAUNCHES back-to-back launches, 3 warm-up windows, REPS timed
windows per variant with the variants of a comparison interleaved; the median and the min .. max
spread are printed, and the device the run was on.

    python tools/gcn_bench.py [--mols 65536] [--out profiles/gcn_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT]
import torch  # noqa: E402
import torch.nn.functional as F_  # noqa: E402

from mvml_gat import FlatAdam, GCNLayer, GCNPredictor, _lib, bce_with_logits, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

HBM_TBS = 8.0
LAUNCHES, REPS = 20, 9


def timed(variants, launches=LAUNCHES, reps=REPS, warm=3):
    """{name: (median ms per call, min, max)} of the callables in `variants`, interleaved."""
    for _ in range(warm):
        for fn in variants.values():
            for _ in range(launches):
                fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches):
                fn()
            e.record()
            torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e) / launches)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def row(name, t, by=None):
    ms, lo, hi = t
    r = {"ms": ms, "min_ms": lo, "max_ms": hi}
    line = f"  {name:44s} {ms:8.4f} ms  ({lo:.4f} .. {hi:.4f})"
    if by is not None:
        gbs = by / ms / 1e6
        r.update(bytes=by, gbs=gbs, frac_hbm=gbs / 1e3 / HBM_TBS)
        line += f"  {by / 1e9:6.3f} GB  {gbs:7.1f} GB/s  {100 * r['frac_hbm']:5.1f} % of 8 TB/s"
    print(line, flush=True)
    return r


def bench_kernel(g, D):
    st = _lib.stream_ptr()
    N, E = g.num_nodes(), g.num_edges()
    torch.manual_seed(0)
    X = torch.randn((N, D), device="cuda") * 0.3
    out = torch.empty((N, D), device="cuda")
    bias = torch.randn(D, device="cuda") * 0.1
    rows = torch.empty(N, dtype=torch.int32, device="cuda")
    s, d = Fn.gcn_scales(g, "both")
    by = Fn.gcn_agg_bytes(N, E, D)

    def agg(scales, transpose=False):
        ns, rs = scales
        rp, nb = (g.out_rowptr, g.out_dst) if transpose else (g.in_rowptr, g.in_src)
        b, act = (None, 0) if transpose else (bias, 1)
        return lambda: call("mvml_gcn_agg", N, ptr(rp), ptr(nb), ptr(X), D, D, ptr(ns), ptr(rs), ptr(b), act,
                            ptr(out), D, None, ptr(rows), st)

    res = {}
    t = timed({"none": agg((None, None)), "both": agg((s, d)), "both_T": agg((d, s), True)})
    res["gcn_none"] = row(f"gcn_agg D={D} none fwd (+ bias, ReLU, row max)", t["none"], by)
    res["gcn_both"] = row(f"gcn_agg D={D} both fwd (+ bias, ReLU, row max)", t["both"], by)
    res["gcn_both_T"] = row(f"gcn_agg D={D} both out-CSR (dX)", t["both_T"], by)
    if D <= 64:
        def form(v):
            f = agg((s, d))

            def run():
                with _lib.option("gcn_subwave", v):
                    f()
            return run
        t = timed({"sub": form(1), "row": form(0)})
        res["subwave"] = row(f"gcn_agg D={D} both, four rows per wave", t["sub"], by)
        res["one_row"] = row(f"gcn_agg D={D} both, one row per wave", t["row"], by)
        res["subwave_over_one_row"] = t["sub"][0] / t["row"][0]
        print(f"  sub-wave / one-row time: {res['subwave_over_one_row']:.3f}", flush=True)
    # the yardstick: the destination-wave GAT forward at H = 1, F = D, flatten without ELU
    elr = torch.randn((N, 2), device="cuda")
    attn = torch.empty((E, 1), device="cuda")
    R = torch.randn((N, D), device="cuda") * 0.3

    def gat(kind):
        def run():
            with _lib.option("dst_fwd", kind):
                call("mvml_gat_agg_fwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr), ptr(g.in_src),
                     ptr(X), D, 1, D, ptr(elr), ptr(R), D, ptr(bias), 0.2, 2, ptr(out), ptr(attn), None, ptr(rows), st)
        return run
    t = timed({"gat1": gat(1), "gat2": gat(2), "gcn": agg((s, d))})
    gby = Fn.agg_fwd_bytes(N, E, 1, D, D, D)
    res["gat_fused_softmax"] = row(f"gat_agg_fwd_res H=1 F={D} softmax in the wave", t["gat1"], gby)
    res["gat_split_softmax"] = row(f"gat_agg_fwd_res H=1 F={D} softmax first", t["gat2"], gby)
    res["gcn_both_again"] = row(f"gcn_agg D={D} both fwd (interleaved with the above)", t["gcn"], by)
    res["gcn_over_gat"] = t["gcn"][0] / min(t["gat1"][0], t["gat2"][0])
    print(f"  gcn / fastest gat time: {res['gcn_over_gat']:.3f}", flush=True)
    return res


def bench_modules(g, feats):
    res = {}
    N = g.num_nodes()
    X2 = torch.randn((N, 64), device="cuda") * 0.3
    steps = {}
    for name, fin, X in (("GCNLayer 74->64 both fwd+bwd", 74, feats), ("GCNLayer 64->64 both fwd+bwd", 64, X2)):
        torch.manual_seed(0)
        layer = GCNLayer(fin, 64, "both", F_.relu).cuda()
        x = X.detach().requires_grad_(fin != 74)
        go = torch.randn((N, 64), device="cuda")
        steps[name] = (lambda layer=layer, x=x, go=go: layer(g, x).backward(go))
    torch.manual_seed(0)
    model = GCNPredictor(74, n_tasks=11).cuda()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    y = (torch.rand((g.batch_size, 11), device="cuda") > 0.5).float()

    def train_step():
        opt.zero_grad()
        bce_with_logits(model(g, feats), y).backward()
        opt.step()
    steps["GCNPredictor(74) training step"] = train_step
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
        raise SystemExit("gcn_bench: needs a GPU (no timing is taken on the CPU)")
    props = torch.cuda.get_device_properties(0)
    box = f"{props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs"
    sb = synth.config3(a.mols)
    g = sb.to_graph().to("cuda")
    print(f"device: {box}\nconfig3: {a.mols} molecules, N={g.num_nodes()}, E={g.num_edges()}", flush=True)
    result = {"device": box, "mols": a.mols, "N": g.num_nodes(), "E": g.num_edges(), "launches": LAUNCHES, "reps": REPS}
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
