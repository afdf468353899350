"""mvml_batchnorm1d_fwd / _bwd on the two tall shapes they are sized for — [65536, 128] (the
predictor's molecule rows) and [1_750_000, 768] (atom rows, what a BatchNorm between graph layers
would feed) — forward and backward, in training and eval mode.  Device events, warm-up passes, the
median of the timed ones.  Two kinds of figure per line, and no pass bar on either:
  * the share of the 8 TB/s HBM peak reached on the ALGORITHMIC bytes (fp32): training forward
    12 M C (x read twice, y written), training backward 20 M C (x and g_y read twice, g_x
    written), eval forward 8 M C, eval backward 12 M C;
  * the ratio to torch's own BatchNorm on the same device and tensors
    (torch.nn.functional.batch_norm and its autograd backward): torch ms / mvml ms, > 1 = faster
    than torch.

    python tools/batchnorm_bench.py [--reps 8] [--warmup 2] [--shapes 65536x128 1750000x768]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mvml-mpi_amd")]
from mvml_gat import _lib  # noqa: E402
from mvml_gat._lib import call, ptr, stream_ptr  # noqa: E402

PEAK_TBS = 8.0  # HBM3E spec
EPS, MOM = 1e-5, 0.1


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


def run(M, C, a):
    dev = "cuda"
    L = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((M, C), device=dev, generator=gen)
    gy = torch.randn((M, C), device=dev, generator=gen)
    w = 1 + 0.1 * torch.randn(C, device=dev, generator=gen)
    b = torch.randn(C, device=dev, generator=gen)
    y, gx = torch.empty_like(x), torch.empty_like(x)
    gw, gb = torch.empty(C, device=dev), torch.empty(C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    save = torch.empty((2, C), dtype=torch.float64, device=dev)
    wsz = L.mvml_batchnorm1d_workspace_size(M, C)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    st = stream_ptr()
    print(f"== [{M}, {C}]: x = {M * C * 4 / 1e9:.3f} GB, {L.mvml_batchnorm1d_part_rows(M)} stripes, "
          f"workspace {wsz / 1e6:.2f} MB", flush=True)

    def fwd(training):
        call("mvml_batchnorm1d_fwd", M, C, ptr(x), C, ptr(w), ptr(b), training, MOM, EPS, ptr(rm), ptr(rv), ptr(nbt),
             ptr(y), C, ptr(save[0]), ptr(save[1]), ptr(ws), wsz, st)

    def bwd(training):
        call("mvml_batchnorm1d_bwd", M, C, ptr(x), C, ptr(w), training, ptr(save[0]), ptr(save[1]), ptr(gy), C,
             ptr(gx), C, ptr(gw), ptr(gb), ptr(ws), wsz, st)

    xt, wt, bt = x.requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    trm, trv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    for mode, training, fbytes, bbytes in (("train", 1, 12, 20), ("eval", 0, 8, 12)):
        yt = F.batch_norm(xt, trm, trv, wt, bt, bool(training), MOM, EPS)
        rows = (("fwd", lambda: fwd(training), fbytes,
                 lambda: F.batch_norm(xt, trm, trv, wt, bt, bool(training), MOM, EPS)),
                ("bwd", lambda: bwd(training), bbytes,
                 lambda: torch.autograd.grad(yt, (xt, wt, bt), gy, retain_graph=True)))
        fwd(training)  # the backward's save_mean / save_invstd are this mode's
        for what, fn, per, tfn in rows:
            med, lo, hi = median_ms(fn, a.warmup, a.reps)
            tmed, tlo, thi = median_ms(tfn, a.warmup, a.reps)
            nbytes = per * M * C
            tbs = nbytes / med / 1e9
            print(f"{mode:5s} {what}  mvml {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}; {a.reps} passes)  "
                  f"{nbytes / 1e9:6.2f} GB algorithmic ({per} M C)  {tbs:5.2f} TB/s = {100 * tbs / PEAK_TBS:4.1f} % of "
                  f"the {PEAK_TBS:.0f} TB/s peak | torch {tmed:8.3f} ms (min {tlo:.3f}, max {thi:.3f})  "
                  f"torch / mvml = {tmed / med:.2f}x", flush=True)
        del yt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["65536x128", "1750000x768"])
    a = ap.parse_args()
    if a.reps < 6:
        ap.error("--reps: at least 6 timed passes")
    print(_lib.lib().mvml_version().decode(), torch.cuda.get_device_name(0), flush=True)
    print("share of peak: algorithmic bytes / time against 8 TB/s; torch / mvml: torch.nn.functional.batch_norm "
          "(and its autograd backward) on the same device and tensors, > 1 = mvml faster; no pass bar", flush=True)
    for s in a.shapes:
        M, C = (int(v) for v in s.split("x"))
        run(M, C, a)


if __name__ == "__main__":
    main()
