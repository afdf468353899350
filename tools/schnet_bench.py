"""Microbenchmark of SchNet's fused filter-network kernels (csrc/schnet.hip) and of one SchNetPredictor
training step on one GPU.

On the config-3 batch, at (F, H, K) = (64, 64, 300) and (128, 128, 300) (cutoff 30, gap 0.1):
  * mvml_schnet_filter_fwd, mvml_schnet_filter_bwd, mvml_schnet_dw1 and mvml_schnet_split_w: ms per
    launch against their algorithmic bytes (functional.schnet_*_bytes) and useful flops;
  * mvml_cfconv_agg over the in-slots and over the out-edges, beside mvml_gcn_agg at the same width;
  * one 3-layer SchNetPredictor training step with FlatAdam;
  * at --small-mols molecules, where the [E, K] expansion fits: the fused filter forward against the
    materialised composition (the expansion by torch, then the project's GEMMs and mvml_ssp_fwd; in this
    tool only), and the norm-wise distance of the two results.

The distances are drawn uniform in [0.9, 3.0]: nobody has measured these kernels on real conformers'
distance distributions, and the timings do not depend on the values beyond exp's range.

Method (tools/gcn_bench.py's): device events around back-to-back launches, warm-up windows, timed
windows per variant with the variants interleaved; median and min .. max.

    python tools/schnet_bench.py [--mols 65536] [--small-mols 4096] [--out profiles/schnet_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mvml-mpi_amd"), ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from gcn_bench import row, timed  # noqa: E402
from mvml_gat import FlatAdam, RBFExpansion, SchNetPredictor, _lib, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402

CUTOFF, GAP = 30.0, 0.1


def dists(g):
    gen = torch.Generator().manual_seed(0)
    return (0.9 + 2.1 * torch.rand(g.num_edges(), generator=gen)).cuda()


def flops_row(name, t, by, fl):
    r = row(name, t, by)
    r.update(flops=fl, tflops=fl / t[0] / 1e9)
    print(f"  {'':44s} {fl / 1e9:8.1f} GFLOP useful  {r['tflops']:6.1f} TFLOP/s", flush=True)
    return r


def operands(g, H, K):
    N, E = g.num_nodes(), g.num_edges()
    rnd = lambda *s: torch.randn(s, device="cuda")
    rbf = RBFExpansion(high=CUTOFF, gap=GAP).cuda()
    W1, b1, W2, b2 = rnd(H, K) / K ** 0.5, rnd(H), rnd(H, H) / H ** 0.5, rnd(H)
    d, ldd = Fn.schnet_slot_dists(g, dists(g))
    return rbf, W1, b1, W2, b2, d, ldd, Fn.schnet_image(W1, W2, H, K)


def bench_kernels(g, H, K):
    st = _lib.stream_ptr()
    N, E = g.num_nodes(), g.num_edges()
    rnd = lambda *s: torch.randn(s, device="cuda")
    new = lambda *s: torch.empty(s, device="cuda")
    rbf, W1, b1, W2, b2, d, ldd, image = operands(g, H, K)
    s1, he, dp2, dp1, hv, dA, a, dhv, dW1, agg = new(E, H), new(E, H), new(E, H), new(E, H), rnd(N, H), rnd(N, H), new(N, H), new(N, H), new(H, K), new(N, H)
    sd, cen, gamma = Fn.nnconv_slot_dst(g), rbf.centers, rbf.gamma
    fwd = lambda: call("mvml_schnet_filter_fwd", E, ptr(d), ldd, ptr(cen), K, gamma, H, ptr(image), ptr(b1), ptr(b2), ptr(s1),
                       H, ptr(he), H, st)
    fwd()
    calls = {
        "filter_fwd": fwd,
        "filter_bwd": lambda: call("mvml_schnet_filter_bwd", E, ptr(g.in_src), ptr(sd), ptr(dA), H, ptr(hv), H, ptr(s1), H,
                                   ptr(he), H, H, K, ptr(image), ptr(dp2), H, ptr(dp1), H, st),
        "dw1": lambda: Fn.schnet_dw1(d, ldd, cen, gamma, dp1, E, H, K, dW1),
        "split_w": lambda: call("mvml_schnet_split_w", H, K, ptr(W1), ptr(W2), ptr(image), st),
        "cfconv_agg": lambda: call("mvml_cfconv_agg", N, E, ptr(g.in_rowptr), None, ptr(g.in_src), ptr(hv), H, ptr(he), H, H,
                                   ptr(a), H, st),
        "cfconv_agg_T": lambda: call("mvml_cfconv_agg", N, E, ptr(g.out_rowptr), ptr(g.out_inslot), ptr(sd), ptr(dA), H,
                                     ptr(he), H, H, ptr(dhv), H, st),
        "gcn_agg": lambda: call("mvml_gcn_agg", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(hv), H, H, None, None, None, 0,
                                ptr(agg), H, None, None, st),
    }
    calls["filter_bwd"]()
    by = {"filter_fwd": Fn.schnet_filter_fwd_bytes(E, H, K), "filter_bwd": Fn.schnet_filter_bwd_bytes(N, E, H),
          "dw1": Fn.schnet_dw1_bytes(E, H, K), "split_w": 4 * (H * K + H * H) + _lib.lib().mvml_schnet_image_bytes(H, K),
          "cfconv_agg": Fn.cfconv_agg_bytes(N, E, H), "cfconv_agg_T": Fn.cfconv_agg_bytes(N, E, H),
          "gcn_agg": Fn.gcn_agg_bytes(N, E, H)}
    fl = {"filter_fwd": Fn.schnet_filter_flops(E, H, K), "filter_bwd": 2 * E * H * H, "dw1": 2 * E * H * K}
    tm = timed(calls, launches=4, reps=7, warm=2)
    return {k: (flops_row(f"{k} H={H} K={K}", tm[k], by[k], fl[k]) if k in fl else row(f"{k} H={H} K={K}", tm[k], by[k]))
            for k in calls}


def bench_fused_vs_materialised(g, H, K):
    """The fused forward against rbf by torch -> GEMM -> ssp -> GEMM -> ssp where [E, K] fits."""
    st = _lib.stream_ptr()
    E = g.num_edges()
    rbf, W1, b1, W2, b2, d, ldd, image = operands(g, H, K)
    s1, he = torch.empty((E, H), device="cuda"), torch.empty((E, H), device="cuda")
    dcol = d[:E, 0].contiguous()
    box = {}

    def fused():
        call("mvml_schnet_filter_fwd", E, ptr(d), ldd, ptr(rbf.centers), K, rbf.gamma, H, ptr(image), ptr(b1), ptr(b2), ptr(s1),
             H, ptr(he), H, st)

    def materialised():
        x = torch.exp(-rbf.gamma * (dcol[:, None] - rbf.centers[None, :]) ** 2)
        y = Fn.linear_forward(x, W1, b1)[2]
        call("mvml_ssp_fwd", y.numel(), ptr(y), ptr(y), st)
        z = Fn.linear_forward(y, W2, b2)[2]
        call("mvml_ssp_fwd", z.numel(), ptr(z), ptr(z), st)
        box["he"] = z
    tm = timed({"fused": fused, "materialised": materialised}, launches=2, reps=7, warm=2)
    dist = float((he - box["he"]).abs().max() / box["he"].abs().max())
    print(f"  fused against materialised he, max|a - b| / max|b|: {dist:.2e}  ([E, K] = {E * K * 4 / 1e9:.2f} GB)", flush=True)
    return {"fused": row(f"filter forward fused H={H} K={K} E={E}", tm["fused"]),
            "materialised": row(f"filter forward materialised H={H} K={K}", tm["materialised"]), "distance": dist}


def bench_step(g, F, H):
    torch.manual_seed(0)
    model = SchNetPredictor(node_feats=F, hidden_feats=[H, H, H], n_tasks=11, cutoff=CUTOFF, gap=GAP).cuda().train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    y = torch.randn(g.batch_size, 11, device="cuda")
    types = torch.randint(0, 100, (g.num_nodes(),), device="cuda", dtype=torch.int32)
    d = dists(g)

    def step():
        opt.zero_grad()
        ((model(g, types, d) - y) ** 2).mean().backward()
        opt.step()
    tm = timed({"step": step}, launches=2, reps=5, warm=1)
    return {"step": row(f"SchNetPredictor F={F} H={H} x3 step (FlatAdam)", tm["step"]),
            "max_memory_gb": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--small-mols", type=int, default=4096)
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--no-modules", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K = Fn.schnet_num_centers(CUTOFF, GAP)
    g = synth.config3(a.mols).to_graph().to("cuda")
    print(f"device: {torch.cuda.get_device_name(0)}; {g.batch_size} molecules, {g.num_nodes()} atoms, {g.num_edges()} edges")
    res = {}
    for H in (int(v) for v in a.sizes.split(",")):
        res[f"H{H}"] = bench_kernels(g, H, K)
        torch.cuda.empty_cache()
        if not a.no_modules:
            res[f"H{H}"].update(bench_step(g, H, H))
            torch.cuda.empty_cache()
    small = synth.config3(a.small_mols).to_graph().to("cuda")
    res["fused_vs_materialised"] = bench_fused_vs_materialised(small, 64, K)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
