"""The weighted-sum-and-max readout (mvml_wsum_max_fwd / _bwd) beside Set2Set's segment pass
(mvml_set2set_seg_fwd, the yardstick: the same access pattern, one wave per molecule, each atom
row read once) on the bench batches: config 3 (65,536 KEGG-like molecules) and config 5 (8,192
molecules of 150-400 atoms), D = 384.  Device events, warm-up passes, the median of the timed ones.
For the two new kernels: ms, TB/s of the algorithmic bytes and the share of the 8 TB/s HBM peak
(forward 4 (N D + N + 3 B D), backward 4 (2 N D + N + 3 B D + partials written and read back));
then forward + backward of the modules WeightedSumAndMax(D) and Set2Set(D, 6, 3) on the same X.

    python tools/readout_bench.py [--D 384] [--reps 8] [--warmup 2] [--configs 3 5]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mvml-mpi_amd")]
from mvml_gat import _lib, synth  # noqa: E402
from mvml_gat import functional as Fn  # noqa: E402
from mvml_gat._lib import call, ptr, stream_ptr  # noqa: E402
from mvml_gat.nn import Set2Set, WeightedSumAndMax  # noqa: E402

PEAK_TBS = 8.0  # HBM3E spec


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def run(name, sb, D, a):
    dev = "cuda"
    g = sb.to_graph().to(dev)
    B, N = g.batch_size, int(sb.num_nodes.sum())
    offs = g.node_offsets
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((N, D), device=dev, generator=gen)
    W = torch.randn(D, device=dev, generator=gen) / D ** 0.5
    b = torch.zeros(1, device=dev)
    g_out = torch.randn((B, 2 * D), device=dev, generator=gen)
    out = torch.empty((B, 2 * D), device=dev)
    gate = torch.empty(N, device=dev)
    argmax = torch.empty((B, D), dtype=torch.int32, device=dev)
    gX = torch.empty((N, D), device=dev)
    R = _lib.lib().mvml_wsum_max_bwd_part_rows(B)
    ldp = D + 4
    part = torch.empty((R, ldp), device=dev)
    gW, gb = torch.empty(D, device=dev), torch.empty(1, device=dev)
    qstar = torch.randn((B, 3 * D), device=dev, generator=gen) / D ** 0.5
    lse = torch.empty(B, device=dev)
    st = stream_ptr()

    def fwd():
        call("mvml_wsum_max_fwd", B, N, D, ptr(offs), ptr(X), D, ptr(W), ptr(b), ptr(out), 2 * D, ptr(gate),
             ptr(argmax), D, st)

    def bwd():
        call("mvml_wsum_max_bwd", B, N, D, ptr(offs), ptr(X), D, ptr(W), ptr(gate), ptr(argmax), D, ptr(g_out),
             2 * D, ptr(gX), D, ptr(part), ldp, st)
        Fn.colsum(part, R, D, ldp, gW)
        Fn.colsum(part, R, 1, ldp, gb, offset=D)

    def seg():
        call("mvml_set2set_seg_fwd", B, D, ptr(offs), ptr(X), ptr(qstar), 3 * D, ptr(lse), st)

    print(f"== {name}: B={B} molecules, N={N} atoms, D={D}, X = {N * D * 4 / 1e9:.2f} GB", flush=True)
    fb = 4 * (N * D + N + 3 * B * D)
    bb = 4 * (2 * N * D + N + 3 * B * D + 2 * R * (D + 1))
    sb_ = 4 * (N * D + 2 * B * D + B)
    res = {}
    for key, fn, nbytes in (("wsum_max_fwd", fwd, fb), ("wsum_max_bwd (+ 2 colsum)", bwd, bb),
                            ("set2set_seg_fwd", seg, sb_)):
        med, lo, hi = median_ms(fn, a.warmup, a.reps)
        tbs = nbytes / med / 1e9
        res[key] = (med, tbs)
        print(f"{key:28s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}; {a.reps} passes)  "
              f"{nbytes / 1e9:6.2f} GB  {tbs:5.2f} TB/s  {100 * tbs / PEAK_TBS:4.1f} % of {PEAK_TBS:.0f} TB/s",
              flush=True)
    print(f"wsum_max_fwd per byte vs set2set_seg_fwd: {res['set2set_seg_fwd'][1] / res['wsum_max_fwd'][1]:.3f}x "
          "the time per byte", flush=True)

    Xg = X.requires_grad_()
    mods = {}
    for key, mod, go in (("WeightedSumAndMax", WeightedSumAndMax(D).to(dev), g_out),
                         ("Set2Set(D, 6, 3)", Set2Set(D, 6, 3).to(dev), g_out)):
        def step(mod=mod, go=go):
            Xg.grad = None
            mod.zero_grad(set_to_none=True)
            mod(g, Xg).backward(go)
        med, lo, hi = median_ms(step, a.warmup, a.reps)
        mods[key] = med
        print(f"{key:28s} {med:8.3f} ms forward + backward (min {lo:.3f}, max {hi:.3f})", flush=True)
    print(f"Set2Set / WeightedSumAndMax, forward + backward: {mods['Set2Set(D, 6, 3)'] / mods['WeightedSumAndMax']:.1f}x",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=384)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--mols3", type=int, default=65536)
    ap.add_argument("--mols5", type=int, default=8192)
    a = ap.parse_args()
    if a.reps < 6:
        ap.error("--reps: at least 6 timed passes")
    print(_lib.lib().mvml_version().decode(), torch.cuda.get_device_name(0), flush=True)
    if 3 in a.configs:
        run("config 3", synth.config3(a.mols3), a.D, a)
    if 5 in a.configs:
        run("config 5", synth.config5(a.mols5), a.D, a)


if __name__ == "__main__":
    main()
