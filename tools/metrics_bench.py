"""MultiLabelMeter.update (mvml_multilabel_metrics: two launches) against the host restatement of
the reference's evaluate (utils.py:109-135: device->host copy, the accuracy() loop, three sklearn
calls) on the same [B, 11] inputs, at the bench's batch (65,536) and the reference's (64).

update: HIP events around every call, warmed, median and spread over --reps calls (device time
from the first launch's start to the second's end, the stream otherwise idle), plus the host
wall time of a call (enqueue only).  Budget: a per-step metric may cost at most 1% of the step
it annotates; pass the step time measured in the same session (python bench.py, ms_per_step) as
--step-ms and the tool prints the comparison at B = 65,536.

    python tools/metrics_bench.py [--reps 50] [--step-ms 137.0] [--no-host]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mvml-mpi_amd")]
from mvml_gat import MultiLabelMeter  # noqa: E402


def reference_evaluate(label, output):
    """utils.py:126-135 restated (sigmoid on the device, the copy, the row loop, sklearn)."""
    from sklearn.metrics import f1_score, precision_score, recall_score
    warnings.filterwarnings("ignore")  # main.py:15 (sklearn's zero-division warnings)
    zs = torch.sigmoid(output).to('cpu').data.numpy()
    ts = label.to('cpu').data.numpy().astype(int)
    preds = np.array(list(map(lambda x: (x >= 0.5).astype(int), zs))).astype(int)
    count = 0
    for i in range(ts.shape[0]):
        count += sum(np.logical_and(ts[i], preds[i])) / sum(np.logical_or(ts[i], preds[i]))
    counts = [sum(ts[:, i] ^ preds[:, i]) for i in range(ts.shape[1])]
    return (count / ts.shape[0], precision_score(ts, preds, average="samples"),
            recall_score(ts, preds, average="samples"), f1_score(ts, preds, average="samples"), counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=None,
                    help="ms_per_step of python bench.py from the same session (the 1%% budget)")
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU")
    dev = "cuda:0"
    C = 11
    for B in (65536, 64):
        g = torch.Generator().manual_seed(B)
        y = (torch.rand(B, C, generator=g) < 0.3).float()
        y[torch.arange(B), torch.randint(C, (B,), generator=g)] = 1.0  # at least one label per row
        z = torch.randn(B, C, generator=g)
        yd, zd = y.to(dev), z.to(dev)
        meter = MultiLabelMeter(C, dev, capacity=a.reps + 8)
        for _ in range(5):
            meter.update(yd, zd)
        torch.cuda.synchronize()
        meter.reset()
        ev, wall = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            meter.update(yd, zd)
            e1.record()
            wall.append((time.perf_counter() - t0) * 1e6)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        us = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
        med = statistics.median(us)
        r = meter.compute()
        print(f"update [{B}, {C}]: device {med:.1f} us median of {a.reps} (min {us[0]:.1f}, "
              f"p90 {us[int(0.9 * (len(us) - 1))]:.1f}, max {us[-1]:.1f}); host enqueue "
              f"{statistics.median(wall):.1f} us median; {2 * B * C * 4 / 1e6:.2f} MB read; "
              f"f1_score {r['f1_score']:.6f}", flush=True)
        if B == 65536 and a.step_ms is not None:
            share = med / 1e3 / a.step_ms
            print(f"budget: update {med / 1e3:.4f} ms vs step {a.step_ms:.3f} ms (bench.py ms_per_step, same "
                  f"session) = {100 * share:.3f}% of the step; limit 1% -> {'within' if share <= 0.01 else 'OVER'}",
                  flush=True)
        if not a.no_host:
            reference_evaluate(yd[:64], zd[:64])  # warm sklearn's imports
            t0 = time.perf_counter()
            ref = reference_evaluate(yd, zd)
            dt = time.perf_counter() - t0
            print(f"host evaluate [{B}, {C}] (reference restated, copy included): {dt * 1e3:.1f} ms, one run; "
                  f"f1_score {ref[3]:.6f}; ratio to update {dt * 1e6 / med:.0f}x", flush=True)


if __name__ == "__main__":
    main()
