"""Microbenchmark of Weave's Gaussian-histogram readout (csrc/weave_gather.hip) and of one WeaveGather
training step on one GPU.

On the config-3 batch, at node_in_feats F = 128 (WeavePredictor's graph_feats) and F = 64 with dgllife's 11
default memberships:
  * mvml_weave_gather_fwd and mvml_weave_gather_bwd: ms per launch against their algorithmic bytes
    (functional.weave_gather_bytes) and the exp evaluations per second (functional.weave_gather_exps);
  * beside them mvml_segment_pool_fwd in sum mode at the same F: the same walk over the atom rows without
    the histogram, the floor of what a readout of these rows costs;
  * one WeaveGather forward + backward (histogram, to_out, tanh and their gradients);
  * at --small-mols molecules, where [N, F K] fits comfortably: the fused forward against the materialised
    composition (the [N, F K] histogram by torch, then mvml_segment_pool_fwd over it; in this tool only), and
    the norm-wise distance of the two results.

The atom values are drawn from tanh of a unit normal, the range WeavePredictor's node_to_graph hands the
readout; the timings do not depend on the values beyond exp's range.

Method (tools/gcn_bench.py's): device events around back-to-back launches, warm-up windows, timed windows
per variant with the variants interleaved; median and min .. max.

    python tools/weave_bench.py [--mols 65536] [--small-mols 4096] [--out profiles/weave_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from gcn_bench import row, timed  # noqa: E402
from mvml_gat import WeaveGather, _lib, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

MEANS, STDS = [m for m, _ in Fn.WEAVE_MEMBERSHIPS], [s for _, s in Fn.WEAVE_MEMBERSHIPS]
K = len(MEANS)


def exp_row(name, t, by, n_exp):
    r = row(name, t, by)
    r.update(exps=n_exp, gexps=n_exp / t[0] / 1e6)
    print(f"  {'':44s} {n_exp / 1e9:8.2f} G exp  {r['gexps']:7.1f} G exp/s", flush=True)
    return r


def atom_rows(g, F):
    return torch.tanh(torch.randn((g.num_nodes(), F), device="cuda", generator=torch.Generator("cuda").manual_seed(0)))


def gather_calls(g, F):
    st = _lib.stream_ptr()
    B, N = g.batch_size, g.num_nodes()
    X, out, dX = atom_rows(g, F), torch.empty((B, F * K), device="cuda"), torch.empty((N, F), device="cuda")
    dG, pooled = torch.randn((B, F * K), device="cuda"), torch.empty((B, F), device="cuda")
    mu, sd, off = Fn._host_floats(MEANS), Fn._host_floats(STDS), g.node_offsets
    calls = {
        "gather_fwd": lambda: call("mvml_weave_gather_fwd", B, N, F, K, mu, sd, ptr(off), ptr(X), F, ptr(out), F * K, st),
        "gather_bwd": lambda: call("mvml_weave_gather_bwd", B, N, F, K, mu, sd, ptr(off), ptr(X), F, ptr(dG), F * K, ptr(dX), F,
                                   st),
        "segment_sum": lambda: call("mvml_segment_pool_fwd", B, N, F, 0, ptr(off), ptr(X), F, ptr(pooled), F, None, F, st),
    }
    return calls, X, out


def bench_kernels(g, F):
    B, N = g.batch_size, g.num_nodes()
    calls, _, _ = gather_calls(g, F)
    tm = timed(calls, launches=4, reps=7, warm=2)
    by = Fn.weave_gather_bytes(B, N, F, K)
    return {"gather_fwd": exp_row(f"gather_fwd F={F} K={K}", tm["gather_fwd"], by, Fn.weave_gather_exps(N, F, K)),
            "gather_bwd": exp_row(f"gather_bwd F={F} K={K}", tm["gather_bwd"], by + 4 * N * F, Fn.weave_gather_exps(N, F, K)),
            "segment_sum": row(f"segment_pool_fwd sum D={F}", tm["segment_sum"], Fn.segment_pool_bytes(B, N, F, "sum"))}


def bench_fused_vs_materialised(g, F):
    """The fused forward against the [N, F K] histogram by torch -> mvml_segment_pool_fwd where it fits."""
    st = _lib.stream_ptr()
    B, N = g.batch_size, g.num_nodes()
    calls, X, out = gather_calls(g, F)
    mu, sd = (torch.tensor(v, device="cuda") for v in (MEANS, STDS))
    pooled, box = torch.empty((B, F * K), device="cuda"), {}

    def materialised():
        q = torch.exp(-(X[..., None] - mu) ** 2 / (2 * sd ** 2)) + 1e-7
        p = (q / q.sum(-1, keepdim=True)).flatten(1)
        call("mvml_segment_pool_fwd", B, N, F * K, 0, ptr(g.node_offsets), ptr(p), F * K, ptr(pooled), F * K, None, F * K, st)
        box["out"] = pooled
    tm = timed({"fused": calls["gather_fwd"], "materialised": materialised}, launches=2, reps=7, warm=2)
    dist = float((out - box["out"]).abs().max() / box["out"].abs().max())
    print(f"  fused against materialised, max|a - b| / max|b|: {dist:.2e}  ([N, F K] = {N * F * K * 4 / 1e9:.2f} GB)", flush=True)
    return {"fused": row(f"gather forward fused F={F} N={N}", tm["fused"]),
            "materialised": row(f"gather forward materialised F={F}", tm["materialised"]), "distance": dist}


def bench_module(g, F):
    torch.manual_seed(0)
    model = WeaveGather(F).cuda().train()
    X = atom_rows(g, F).requires_grad_()
    gy = torch.randn((g.batch_size, F), device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        X.grad = None
        model(g, X).backward(gy)
    tm = timed({"step": step}, launches=2, reps=5, warm=1)
    return {"step": row(f"WeaveGather F={F} forward + backward", tm["step"]),
            "max_memory_gb": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--small-mols", type=int, default=4096)
    ap.add_argument("--sizes", default="128,64")
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = synth.config3(a.mols).to_graph().to("cuda")
    print(f"device: {torch.cuda.get_device_name(0)}; {g.batch_size} molecules, {g.num_nodes()} atoms, {g.num_edges()} edges")
    res = {}
    for F in (int(v) for v in a.sizes.split(",")):
        res[f"F{F}"] = bench_kernels(g, F)
        torch.cuda.empty_cache()
        if not a.no_modules:
            res[f"F{F}"].update(bench_module(g, F))
            torch.cuda.empty_cache()
    small = synth.config3(a.small_mols).to_graph().to("cuda")
    res["fused_vs_materialised"] = bench_fused_vs_materialised(small, 128)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
