"""float64 NumPy restatement of the multi-label metric definitions of include/mvml_gat.h
(mvml_multilabel_metrics) and of MultiLabelMeter's reporting rule.  Shared by the CPU and GPU
metric tests; tests/test_metrics_cpu.py checks it against the literal reference formulas
(utils.py:109-135: the accuracy() loop and sklearn's average="samples" scores)."""
import math

import numpy as np


def predict(z):
    """p = (z >= 0): NaN gives 0, -0.0 gives 1."""
    z = np.asarray(z)
    with np.errstate(invalid="ignore"):
        return (z >= 0).astype(np.int64)


def batch_sums(y, z):
    """(sums[8] float64, class_counts [4][C] int64) of one batch, as the kernel defines them.
    The four sums are exactly rounded sums (math.fsum) of the correctly rounded per-row terms."""
    y = (np.asarray(y) >= 0.5).astype(np.int64)
    p = predict(z)
    B = y.shape[0]
    t = (y & p).sum(1)
    u = (y | p).sum(1)
    a = y.sum(1)
    b = p.sum(1)
    jac = [ti / ui if ui else 0.0 for ti, ui in zip(t.tolist(), u.tolist())]
    pre = [ti / bi if bi else 0.0 for ti, bi in zip(t.tolist(), b.tolist())]
    rec = [ti / ai if ai else 0.0 for ti, ai in zip(t.tolist(), a.tolist())]
    f1 = [2 * ti / (ai + bi) if ai + bi else 0.0 for ti, ai, bi in zip(t.tolist(), a.tolist(), b.tolist())]
    sums = np.array([math.fsum(jac), math.fsum(pre), math.fsum(rec), math.fsum(f1), float(B),
                     float((u == 0).sum()), 0.0, 0.0])
    counts = np.stack([(y & p).sum(0), ((1 - y) & p).sum(0), (y & (1 - p)).sum(0),
                       ((1 - y) & (1 - p)).sum(0)]).astype(np.int64)
    return sums, counts


def batch_means(sums):
    """(acc, precision, recall, f1) of one batch from its sums; acc is NaN when a row had an
    empty union (the reference's 0 / 0)."""
    B = sums[4]
    m = [sums[k] / B if B else float("nan") for k in range(4)]
    if sums[5] > 0:
        m[0] = float("nan")
    return m


def class_wise(counts):
    tp, fp, fn, tn = (np.asarray(c, dtype=np.float64) for c in counts)
    n = tp + fp + fn + tn

    def div(a, b):
        return [float(x / d) if d else 0.0 for x, d in zip(a, b)]
    return [div(tp + tn, n), div(tp, tp + fp), div(tp, tp + fn), div(2 * tp, 2 * tp + fp + fn)]


def meter_ref(batches):
    """MultiLabelMeter.compute() for a list of (labels, logits) batches: the mean over batches of
    per-batch means (main.py:54-55), the per-sample variants and the class counts."""
    all_sums, counts = [], None
    for y, z in batches:
        s, c = batch_sums(y, z)
        all_sums.append(s)
        counts = c if counts is None else counts + c
    return summarize_ref(all_sums, counts)


def summarize_ref(all_sums, counts):
    names = ("acc", "precision", "recall", "f1_score")
    means = [batch_means(s) for s in all_sums]
    rows = sum(s[4] for s in all_sums)
    out = {}
    for k, name in enumerate(names):
        out[name] = math.fsum(m[k] for m in means) / len(means)
        out[name + "_per_sample"] = math.fsum(s[k] for s in all_sums) / rows
    out["n_batches"] = len(all_sums)
    out["n_samples"] = int(rows)
    out["class_counts"] = np.asarray(counts).tolist()
    out["class_wise"] = class_wise(counts)
    return out


def random_batch(rng, B, C, min_abs=1e-3, min_labels=1):
    """Labels in {0, 1} with at least ``min_labels`` per row, logits with |z| >= min_abs."""
    y = (rng.random((B, C)) < 0.3).astype(np.float32)
    for i in range(B):
        while y[i].sum() < min_labels:
            y[i, rng.integers(C)] = 1.0
    z = rng.standard_normal((B, C)).astype(np.float32)
    z = np.where(np.abs(z) < min_abs, np.float32(min_abs), z).astype(np.float32)
    return y, z
