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

The pair-update layers (csrc/weave_pair.hip), on the same batch with 12 bond features, every width H = 50
(dgllife's default) and 128:
  * mvml_weave_split_w, mvml_weave_edge_fwd (with and without the saved operand), mvml_weave_edge_bwd,
    mvml_weave_e2n_fwd and mvml_weave_e2n_bwd against their algorithmic bytes and useful flops;
  * one WeaveLayer forward + backward and one WeavePredictor step at the defaults;
  * at --small-mols molecules: the fused edge forward against the composition that materialises first,
    second, their sum, third and the concat (products on the project's GEMM, the rest by torch; in this
    tool only), their ratio and distance.

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


def flop_row(name, t, by, flops):
    r = row(name, t, by)
    r.update(flops=flops, tflops=flops / t[0] / 1e9)
    print(f"  {'':44s} {flops / 1e9:8.2f} GFLOP useful  {r['tflops']:6.2f} TFLOP/s", flush=True)
    return r


def pair_state(g, H, De=12):
    """Operands of the five kernels of csrc/weave_pair.hip with every width H and De bond features."""
    N, E = g.num_nodes(), g.num_edges()
    gen = torch.Generator("cuda").manual_seed(H)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)
    Hq, De4 = Fn._round4(H), Fn._round4(De)
    s = dict(N=N, E=E, H=H, De=De, Hq=Hq, De4=De4, W_ee=rnd(H, De) * De ** -0.5, W_en=rnd(H, De) * De ** -0.5,
             W_ue=rnd(H, 2 * H) * (2 * H) ** -0.5, b=rnd(H) * 0.1, e=Fn.zeros((E, De4), device="cuda"), LR=Fn.zeros((N, 2 * Hq), device="cuda"),
             en=torch.empty((E, Hq), device="cuda"), A=torch.empty((E, 2 * Hq), device="cuda"), G=rnd(E, Hq),
             dpre=torch.empty((E, Hq), device="cuda"), dfs=torch.empty((E, 2 * Hq), device="cuda"),
             dthird=torch.empty((E, Hq), device="cuda"), S=torch.empty((N, H), device="cuda"), dS=rnd(N, H),
             dpre_en=torch.empty((E, Hq), device="cuda"), dst=Fn.nnconv_slot_dst(g))
    s["e"][:, :De] = rnd(E, De)
    s["LR"][:, :H], s["LR"][:, Hq:Hq + H] = rnd(N, H), rnd(N, H)
    s["image"] = Fn.weave_image(De, H, H, H, H, s["W_ee"], s["W_en"], s["W_ue"])
    s["ws"] = torch.empty(_lib.lib().mvml_weave_e2n_workspace_size(E, H), dtype=torch.uint8, device="cuda")
    return s


def pair_calls(g, s):
    st = _lib.stream_ptr()
    N, E, H, De, Hq, De4 = (s[k] for k in ("N", "E", "H", "De", "Hq", "De4"))
    P = lambda k: ptr(s[k])

    def edge_fwd(A):
        return lambda: call("mvml_weave_edge_fwd", N, E, ptr(g.in_src), P("dst"), P("e"), De4, De, P("LR"), 2 * Hq, Hq, H, H, H, H,
                            P("image"), P("b"), P("b"), P("en"), Hq, ptr(A), 2 * Hq, st)
    return {
        "split_w": lambda: call("mvml_weave_split_w", De, H, H, H, H, P("W_ee"), P("W_en"), P("W_ue"), P("image"), st),
        "edge_fwd": edge_fwd(None), "edge_fwd_grad": edge_fwd(s["A"]),
        "edge_bwd": lambda: call("mvml_weave_edge_bwd", N, E, ptr(g.in_src), P("dst"), P("G"), Hq, P("en"), Hq, P("A"), 2 * Hq, P("LR"),
                                 2 * Hq, Hq, De, H, H, H, H, P("image"), P("dpre"), Hq, P("dfs"), 2 * Hq, P("dthird"), Hq, st),
        "e2n_fwd": lambda: call("mvml_weave_e2n_fwd", N, E, ptr(g.in_rowptr), P("dst"), P("e"), De4, De, H, H, H, H, P("image"), P("b"),
                                P("S"), H, P("ws"), s["ws"].numel(), st),
        "e2n_bwd": lambda: call("mvml_weave_e2n_bwd", N, E, P("dst"), P("e"), De4, De, H, H, H, H, P("image"), P("b"), P("dS"), H,
                                P("dpre_en"), Hq, st)}


def bench_pair_kernels(g, H):
    s = pair_state(g, H)
    N, E, De = s["N"], s["E"], s["De"]
    calls = pair_calls(g, s)
    calls["edge_fwd_grad"]()  # (the backward reads e' and the saved operand)
    tm = timed(calls, launches=4, reps=7, warm=2)
    fl = Fn.weave_edge_flops(E, De, H, H, H)
    return {"split_w": row(f"weave_split_w H={H}", tm["split_w"]),
            "edge_fwd": flop_row(f"weave_edge_fwd H={H}", tm["edge_fwd"], Fn.weave_edge_fwd_bytes(N, E, De, H, H, H), fl),
            "edge_fwd_grad": flop_row(f"weave_edge_fwd H={H} (+ saved operand)", tm["edge_fwd_grad"],
                                      Fn.weave_edge_fwd_bytes(N, E, De, H, H, H, True), fl),
            "edge_bwd": flop_row(f"weave_edge_bwd H={H}", tm["edge_bwd"], Fn.weave_edge_bwd_bytes(N, E, H, H, H), 4 * E * H * H),
            "e2n_fwd": flop_row(f"weave_e2n_fwd H={H}", tm["e2n_fwd"], Fn.weave_e2n_bytes(N, E, De, H), Fn.weave_e2n_flops(E, De, H)),
            "e2n_bwd": flop_row(f"weave_e2n_bwd H={H}", tm["e2n_bwd"], Fn.weave_e2n_bytes(N, E, De, H, True),
                                Fn.weave_e2n_flops(E, De, H))}


def bench_pair_fused_vs_materialised(g, H):
    """The fused edge forward against the composition that writes first, second, their sum, third and the
    concat: the products on the project's GEMM, the gathers and element-wise steps by torch (in this tool only)."""
    s = pair_state(g, H)
    Hq, De = s["Hq"], s["De"]
    src, dst = g.in_src.long(), s["dst"].long()
    L, R, e = s["LR"][:, :H].contiguous(), s["LR"][:, Hq:Hq + H].contiguous(), s["e"][:, :De].contiguous()
    box = {}

    def materialised():
        first, second = torch.relu(L[src] + R[dst]), torch.relu(R[src] + L[dst])
        third = Fn.linear_forward(e, s["W_ee"], s["b"], act=1)[2]
        box["out"] = Fn.linear_forward(torch.cat([first + second, third], 1), s["W_ue"], s["b"], act=1)[2]
    tm = timed({"fused": pair_calls(g, s)["edge_fwd"], "materialised": materialised}, launches=2, reps=7, warm=2)
    dist = float((s["en"][:, :H] - box["out"]).abs().max() / box["out"].abs().max())
    print(f"  fused against materialised, max|a - b| / max|b|: {dist:.2e}", flush=True)
    return {"fused": row(f"edge forward fused H={H} E={s['E']}", tm["fused"]),
            "materialised": row(f"edge forward materialised H={H}", tm["materialised"]), "distance": dist,
            "ratio": tm["materialised"][0] / tm["fused"][0]}


def bench_pair_modules(g, De=12, Dn=27):
    from mvml_gat import WeaveLayer, WeavePredictor
    torch.manual_seed(0)
    N, E, B = g.num_nodes(), g.num_edges(), g.batch_size
    x, e = torch.randn((N, Dn), device="cuda").requires_grad_(), torch.randn((E, De), device="cuda")
    layer, model = WeaveLayer(Dn, De).cuda().train(), WeavePredictor(Dn, De).cuda().train()
    gx, ge, gy = torch.randn((N, 50), device="cuda"), torch.randn((E, 50), device="cuda"), torch.randn((B, 1), device="cuda")

    def layer_step():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        torch.autograd.backward(list(layer(g, x, e)), [gx, ge])

    def model_step():
        model.zero_grad(set_to_none=True)
        x.grad = None
        model(g, x, e).backward(gy)
    tm = timed({"layer": layer_step, "predictor": model_step}, launches=2, reps=5, warm=1)
    return {"layer": row("WeaveLayer H=50 forward + backward", tm["layer"]),
            "predictor": row("WeavePredictor forward + backward", tm["predictor"]),
            "max_memory_gb": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=65536)
    ap.add_argument("--small-mols", type=int, default=4096)
    ap.add_argument("--sizes", default="128,64")
    ap.add_argument("--pair-sizes", default="50,128")
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
    print("pair-update layers (csrc/weave_pair.hip), 12 bond features:")
    for H in (int(v) for v in a.pair_sizes.split(",")):
        res[f"pair_H{H}"] = bench_pair_kernels(g, H)
        torch.cuda.empty_cache()
    if not a.no_modules:
        res["pair_modules"] = bench_pair_modules(g)
        torch.cuda.empty_cache()
    res["pair_fused_vs_materialised"] = bench_pair_fused_vs_materialised(small, 50)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
