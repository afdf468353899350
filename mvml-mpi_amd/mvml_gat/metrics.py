"""The reference's per-batch metrics (utils.py:109-173) on the device.

main.py:32 calls ``evaluate(labels, pred)`` after every forward; the reference implements it as
a device->host copy, a Python loop over the rows and three sklearn calls.  Here one HIP entry
point (mvml_multilabel_metrics) computes a batch's sums on the stream the forward ran on:

    meter = MultiLabelMeter(11, "cuda:0")
    for batch in loader:
        ...
        meter.update(labels, logits)        # enqueue only: no host read-back
    res = meter.compute()                   # the one synchronisation
    res["acc"], res["precision"], res["recall"], res["f1_score"]    # main.py:54-55 / 108-109

``evaluate`` and ``evaluate_class_wise`` are drop-ins for the reference's functions of those
names on device tensors.  Definitions (prediction rule z >= 0, zero-division values, empty
unions): include/mvml_gat.h, mvml_multilabel_metrics.
"""
import ctypes
import math

import torch
import torch.distributed as dist

from . import _lib
from ._lib import call, ptr, stream_ptr

_NAMES = ("acc", "precision", "recall", "f1_score")


def _rows_ld(t, C):
    """A [B, C] fp32 tensor as (tensor, leading dimension): rows of unit column stride are
    passed in place by their row stride; anything else is made contiguous."""
    if t.dtype != torch.float32:
        t = t.float()
    B = t.shape[0]
    if t.stride(1) == 1 or C == 1:
        if B <= 1:
            return t, C
        if t.stride(0) >= C:
            return t, t.stride(0)
    return t.contiguous(), C


def reduce_metric_buffers(sums, class_counts, group=None):
    """Sum the per-batch ``sums`` ([n, 8] fp64) and the ``class_counts`` ([4, C] int64) over the
    ranks of ``group`` in place: every rank scored its shard of each of the same n batches, and
    afterwards each row holds the sums and the row count of the whole batch.  Plain tensors of
    any device (gloo on CPU tensors in the tests, RCCL on the GPU)."""
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(class_counts, op=dist.ReduceOp.SUM, group=group)
    return sums, class_counts


def class_wise(class_counts):
    """Per-class binary accuracy, precision, recall and F1 from [4][C] tp / fp / fn / tn counts:
    evaluate_class_wise (utils.py:138-173) for C classes; 0 where a denominator is 0 (sklearn's
    default).  Returns four lists of C floats."""
    tp, fp, fn, tn = ([float(v) for v in row] for row in class_counts)
    acc, pre, rec, f1 = [], [], [], []
    for c in range(len(tp)):
        n = tp[c] + fp[c] + fn[c] + tn[c]
        acc.append((tp[c] + tn[c]) / n if n else float("nan"))
        pre.append(tp[c] / (tp[c] + fp[c]) if tp[c] + fp[c] else 0.0)
        rec.append(tp[c] / (tp[c] + fn[c]) if tp[c] + fn[c] else 0.0)
        f1.append(2 * tp[c] / (2 * tp[c] + fp[c] + fn[c]) if 2 * tp[c] + fp[c] + fn[c] else 0.0)
    return [acc, pre, rec, f1]


def summarize(sums, class_counts):
    """The result dict of MultiLabelMeter.compute from host values: ``sums`` a list of n rows of
    8 floats (one per batch), ``class_counts`` four lists of C ints."""
    n = len(sums)
    per_batch = [[], [], [], []]
    for s in sums:
        rows = s[4]
        for k in range(4):
            per_batch[k].append(s[k] / rows if rows else float("nan"))
        if s[5] > 0:  # a row with an empty union: the reference's 0 / 0
            per_batch[0][-1] = float("nan")
    rows = sum(s[4] for s in sums)
    out = {}
    for k, name in enumerate(_NAMES):
        out[name] = math.fsum(per_batch[k]) / n if n else float("nan")
        out[name + "_per_sample"] = math.fsum(s[k] for s in sums) / rows if rows else float("nan")
    out["n_batches"] = n
    out["n_samples"] = int(rows)
    out["n_empty_union"] = int(sum(s[5] for s in sums))
    out["class_counts"] = [[int(v) for v in row] for row in class_counts]
    out["class_wise"] = class_wise(class_counts)
    return out


class MultiLabelMeter:
    """Accumulates evaluate()'s metrics over the batches of a phase without leaving the device.

    ``update(labels, logits)`` enqueues mvml_multilabel_metrics on the current stream: the
    batch's ``sums[8]`` land in the batch's own row of a device [capacity, 8] fp64 buffer (the
    host knows the row index; the buffer doubles when full, by a device copy in stream order)
    and the per-class tp / fp / fn / tn counts accumulate in one [4, C] int64 buffer.
    ``compute()`` is the only synchronisation: one device->host copy.  ``acc`` / ``precision`` /
    ``recall`` / ``f1_score`` are the MEAN OVER BATCHES OF PER-BATCH MEANS, which is what the
    reference reports (main.py:54-55, 108-109: a short last batch weighs as much as a full one);
    the ``*_per_sample`` entries divide the sums over all rows by the number of rows.  A batch
    with an empty-union row has ``acc`` NaN, as the reference's 0 / 0 gives; ``acc_per_sample``
    counts such rows as 0 and ``n_empty_union`` says how many there were."""

    def __init__(self, num_classes, device, capacity=64):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("MultiLabelMeter: num_classes >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MvmlError("MultiLabelMeter runs on the GPU (there is no CPU fallback)")
        self.sums = torch.zeros(max(int(capacity), 1), 8, dtype=torch.float64, device=self.device)
        self.class_counts = torch.zeros(4, self.num_classes, dtype=torch.int64, device=self.device)
        self.n_batches = 0

    @property
    def capacity(self):
        return self.sums.shape[0]

    def reset(self):
        self.n_batches = 0
        self.sums.zero_()
        self.class_counts.zero_()

    def _row_ptr(self):
        if self.n_batches == self.capacity:
            grown = torch.zeros(2 * self.capacity, 8, dtype=torch.float64, device=self.device)
            grown[:self.capacity].copy_(self.sums)
            self.sums = grown
        return ctypes.c_void_p(self.sums.data_ptr() + self.n_batches * 8 * 8)

    @torch.no_grad()
    def update(self, labels, logits):
        C = self.num_classes
        if labels.dim() != 2 or labels.shape != logits.shape or labels.shape[1] != C:
            raise ValueError(f"MultiLabelMeter.update: labels {tuple(labels.shape)} and logits "
                             f"{tuple(logits.shape)} must both be [B, {C}]")
        if labels.device != self.device or logits.device != self.device:
            raise _lib.MvmlError(f"MultiLabelMeter.update: tensors must be on {self.device}")
        B = labels.shape[0]
        y, ldy = _rows_ld(labels, C)
        z, ldz = _rows_ld(logits, C)
        L = _lib.lib()
        wp, wn = _lib.ws_ptr_size(L.mvml_multilabel_metrics_workspace_size(B, C), self.device)
        call("mvml_multilabel_metrics", B, C, ptr(z), ldz, ptr(y), ldy, self._row_ptr(),
             ptr(self.class_counts), wp, wn, stream_ptr(self.device))
        self.n_batches += 1

    def compute(self, group=None, extra=None):
        """Synchronise once and return the result dict.  With ``group``, or when
        torch.distributed is initialised with more than one rank, the per-batch sums and the
        class counts are first summed over the ranks (reduce_metric_buffers), so a data-parallel
        batch is scored as the whole batch.  ``extra``: an optional 1-D device tensor that rides
        on the same copy (fit's loss sum); it comes back as ``result["extra"]``, a list."""
        n = self.n_batches
        sums, counts = self.sums[:n], self.class_counts
        if group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            sums, counts = reduce_metric_buffers(sums.clone(), counts.clone(), group)
        parts = [sums.reshape(-1), counts.reshape(-1).double()]  # counts < 2^53: exact in fp64
        if extra is not None:
            parts.append(extra.detach().reshape(-1).double())
        host = torch.cat(parts).cpu().tolist()
        C = self.num_classes
        rows = [host[8 * i:8 * i + 8] for i in range(n)]
        cc = host[8 * n:8 * n + 4 * C]
        out = summarize(rows, [[int(v) for v in cc[k * C:(k + 1) * C]] for k in range(4)])
        if extra is not None:
            out["extra"] = host[8 * n + 4 * C:]
        return out


def evaluate(label, output):
    """utils.py:126-135 on device tensors: (acc, precision, recall, f1score, acc_weight) of one
    batch; ``acc_weight`` is the CPU [B, C] float tensor whose every row is the per-class
    mismatch count (accuracy()'s class_weight).  One synchronisation, like the function it
    mirrors."""
    meter = MultiLabelMeter(label.shape[1], label.device, capacity=1)
    meter.update(label, output)
    r = meter.compute()
    cc = r["class_counts"]
    weight = torch.tensor([float(a + b) for a, b in zip(cc[1], cc[2])])
    acc_weight = torch.ones((label.shape[0], 1)).matmul(weight.unsqueeze(0))
    return r["acc"], r["precision"], r["recall"], r["f1_score"], acc_weight


def evaluate_class_wise(label, output, verbose=True):
    """utils.py:138-173 for any number of classes: [acc_list, pre_list, rec_list, f1_list]."""
    meter = MultiLabelMeter(label.shape[1], label.device, capacity=1)
    meter.update(label, output)
    lists = meter.compute()["class_wise"]
    if verbose:
        for c, (acc, pre, rec, f1) in enumerate(zip(*lists)):
            print('Class ' + str(c + 1) + ' Binary Classification Statistics:')
            print('Accuracy(Binary) %.4f, Precision(Binary) %.4f, Recall(Binary) %.4f, '
                  'F1-Score(Binary) %.4f\n' % (acc, pre, rec, f1))
    return lists
