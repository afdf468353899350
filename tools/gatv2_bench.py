"""Microbenchmark of the GATv2 aggregation (mvml_gatv2_agg_fwd / _bwd, csrc/gatv2_agg.hip) on one
GPU: time per launch (device events, 2 warm-up passes, median of 8), TB/s against the algorithmic
bytes (mvml_gat.functional.gatv2_fwd_bytes / gatv2_bwd_bytes) and the fraction of 8 TB/s; the
yardstick mvml_gat_agg_fwd_res / mvml_gat_agg_bwd_res on the same graph, shape and mode in the
same process (time per algorithmic byte, GATv2 / GAT); and whole GATv2Layer against GATLayer
forward + backward at the model's two layers.

    python tools/gatv2_bench.py [--configs 3:65536,5:8192] [--out profiles/gatv2_bench.json]
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

from mvml_gat import _lib, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr  # noqa: E402
from mvml_gat.nn import GATLayer, GATv2Layer  # noqa: E402

HBM_TBS = 8.0
SHAPES = ((4, 192, 0, "4x192 flatten+ELU"), (4, 384, 1, "4x384 head mean"))


def median_ms(fn, warm=2, reps=8):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def row(name, ms, by):
    tbs = by / ms / 1e9
    print(f"  {name:34s} {ms:8.3f} ms  {by / 1e9:7.2f} GB  {tbs:6.3f} TB/s  {100 * tbs / HBM_TBS:5.1f} % of 8 TB/s",
          flush=True)
    return {"ms": ms, "bytes": by, "tbs": tbs, "frac_hbm": tbs / HBM_TBS}


def bench_kernels(g, H, F, mode, name):
    L, st = _lib.lib(), _lib.stream_ptr()
    N, E, HF = g.num_nodes(), g.num_edges(), H * F
    oc = rw = F if mode == 1 else HF
    torch.manual_seed(0)
    ldy = Fn._row_pitch(2 * HF)
    Y = torch.randn((N, ldy), device="cuda") * 0.3
    R = torch.randn((N, rw), device="cuda") * 0.3
    av = 3 * torch.randn(HF, device="cuda") / F ** 0.5
    out = torch.empty((N, oc), device="cuda")
    attn = torch.empty((E, H), device="cuda")
    g_out = torch.randn((N, oc), device="cuda")
    zr = ptr(Y[:, HF:])
    res = {}
    fwd = lambda: call("mvml_gatv2_agg_fwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(Y), ldy, zr, ldy, H, F, ptr(av),
                       ptr(R), rw, 0.2, mode, ptr(out), ptr(attn), st)
    res["gatv2_fwd"] = row(f"gatv2_agg_fwd {name}", median_ms(fwd), Fn.gatv2_fwd_bytes(N, E, H, F, oc, rw))
    gY = torch.empty((N, ldy), device="cuda")
    gR = torch.empty((N, rw), device="cuda")
    gav = torch.empty(HF, device="cuda")
    wsz = L.mvml_gatv2_agg_bwd_workspace_size(N, E, H, F)
    ws = torch.empty(wsz, dtype=torch.uint8, device="cuda")
    bwd = lambda: call("mvml_gatv2_agg_bwd", N, ptr(g.in_rowptr), ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst),
                       ptr(g.out_inslot), E, ptr(Y), ldy, zr, ldy, H, F, ptr(av), ptr(attn), ptr(out), ptr(g_out),
                       0.2, mode, ptr(gY), ldy, ptr(gY[:, HF:]), ldy, ptr(gR), rw, ptr(gav), ptr(ws), wsz, st)
    res["gatv2_bwd"] = row(f"gatv2_agg_bwd {name}", median_ms(bwd), Fn.gatv2_bwd_bytes(N, E, H, F, oc, rw, mode))
    del gY, gav, ws
    # the yardstick: GAT's separate-residual entries as the Python layer runs them on this batch
    elr = torch.randn((N, 2 * H), device="cuda")
    bias = torch.randn(HF, device="cuda") * 0.1
    large = Fn._large_batch(g)
    ldz = Fn._row_pitch(HF)
    Z = Y[:, :ldz] if ldz <= ldy else torch.randn((N, ldz), device="cuda") * 0.3
    ldz = Z.stride(0)
    with _lib.option("dst_fwd", 1 if large else 2):
        gfwd = lambda: call("mvml_gat_agg_fwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                            ptr(g.in_src), ptr(Z), ldz, H, F, ptr(elr), ptr(R), rw, ptr(bias), 0.2, mode, ptr(out),
                            ptr(attn), None, None, st)
        res["gat_fwd"] = row(f"gat_agg_fwd_res {name}", median_ms(gfwd), Fn.agg_fwd_bytes(N, E, H, F, oc, rw))
    ldg = Fn._row_pitch(HF + 2 * H)
    gY = torch.empty((N, ldg), device="cuda")
    wsz = L.mvml_gat_agg_bwd_workspace_size(E, H)
    ws = torch.empty(max(wsz, 1), dtype=torch.uint8, device="cuda")
    with _lib.option("flat_src", 2 if (large and mode != 1) else 0):
        gbwd = lambda: call("mvml_gat_agg_bwd_res", N, ptr(g.node_groups), g.num_node_groups, ptr(g.in_rowptr),
                            ptr(g.in_src), ptr(g.out_rowptr), ptr(g.out_dst), ptr(g.out_inslot), ptr(Z), ldz,
                            ptr(elr), ptr(attn), ptr(out), ptr(g_out), H, F, 0.2, mode, ptr(gY), ldg, HF, ptr(gR), rw,
                            None, None, ptr(ws), wsz, st)
        res["gat_bwd"] = row(f"gat_agg_bwd_res {name}", median_ms(gbwd), Fn.agg_bwd_bytes(N, E, H, F, oc, mode))
    for k in ("fwd", "bwd"):
        a, b = res["gatv2_" + k], res["gat_" + k]
        res[f"ratio_{k}_time_per_byte"] = (a["ms"] / a["bytes"]) / (b["ms"] / b["bytes"])
        res[f"ratio_{k}_time"] = a["ms"] / b["ms"]
        print(f"  {k}: GATv2 / GAT time per algorithmic byte {res[f'ratio_{k}_time_per_byte']:.2f}, "
              f"time {res[f'ratio_{k}_time']:.2f}", flush=True)
    return res


def bench_layers(g, feats):
    """GATv2Layer against GATLayer, forward + backward, at the model's two layers."""
    res = {}
    N = g.num_nodes()
    X2 = torch.randn((N, 768), device="cuda") * 0.3
    for name, fin, Fo, mode, act, X in (("layer 1 74->4x192 flatten+ELU", 74, 192, "flatten", F_.elu, feats),
                                        ("layer 2 768->4x384 mean", 768, 384, "mean", None, X2)):
        for kind, mk in (("gat", lambda: GATLayer(fin, Fo, 4, agg_mode=mode, activation=act)),
                         ("gatv2", lambda: GATv2Layer(fin, Fo, 4, agg_mode=mode, activation=act))):
            torch.manual_seed(0)
            layer = mk().cuda()
            x = X.detach().requires_grad_(fin != 74)
            go = [None]

            def step():
                out = layer(g, x)
                if go[0] is None:
                    go[0] = torch.randn_like(out)
                out.backward(go[0])

            ms = median_ms(step)
            res[f"{kind} {name}"] = ms
            print(f"  {kind:6s} {name:32s} fwd+bwd {ms:8.3f} ms", flush=True)
            del layer
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3:65536,5:8192", help="synth config:molecules, comma separated")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    result = {}
    for spec in a.configs.split(","):
        cfg, mols = spec.split(":")
        sb = getattr(synth, f"config{cfg}")(int(mols))
        g = sb.to_graph().to("cuda")
        print(f"config{cfg}: {mols} molecules, N={g.num_nodes()}, E={g.num_edges()}, "
              f"g_attn partial rows {_lib.lib().mvml_gatv2_partial_rows(g.num_nodes())}", flush=True)
        r = {"N": g.num_nodes(), "E": g.num_edges()}
        for H, F, mode, name in SHAPES:
            r[name] = bench_kernels(g, H, F, mode, name)
        if not a.no_layers:
            r["layers"] = bench_layers(g, torch.as_tensor(sb.feats, dtype=torch.float32).cuda())
        result[f"config{cfg}"] = r
        del g
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
