"""mvml_multilabel_metrics and MultiLabelMeter on the GPU against the float64 restatement
(tests/_metrics_ref.py, itself checked against the reference's formulas in test_metrics_cpu.py).

Bars: class counts exact; the four fp64 sums within 1e-12 of the exactly rounded sums of the
restatement (B * 2^-53 <= 4.6e-13 at B = 4096 for terms in [0, 1], rounded up); two runs on the
same input bitwise equal."""
import functools

import numpy as np
import pytest
import torch

import _metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SHAPES = [(1, 1), (1, 11), (63, 11), (64, 11), (65, 11), (257, 11), (4096, 11), (300, 64), (300, 65),
          (70, 130)]


@functools.lru_cache(maxsize=None)
def _case(B, C):
    """Seeded (labels, logits, reference sums, reference counts); rows with no label, with no
    prediction and with neither are left in (the general case of the definitions)."""
    rng = np.random.default_rng(1000 * B + C)
    y, z = R.random_batch(rng, B, C, min_labels=0)
    sums, counts = R.batch_sums(y, z)
    return y, z, sums, counts


def _run(y, z):
    """One kernel call through the meter; (sums[8], class_counts [4][C]) on the host."""
    from mvml_gat import MultiLabelMeter
    meter = MultiLabelMeter(y.shape[1], DEV, capacity=1)
    meter.update(y, z)
    torch.cuda.synchronize()
    return meter.sums[0].cpu().numpy(), meter.class_counts.cpu().numpy()


def _padded_view(a, left=2, right=3):
    """a as a column slice of a wider device buffer (leading dimension C + left + right)."""
    B, C = a.shape
    wide = torch.full((B, C + left + right), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, left:left + C] = torch.as_tensor(a, device=DEV)
    return wide[:, left:left + C]


def _check(got, want_sums, want_counts):
    sums, counts = got
    assert np.array_equal(counts, want_counts)
    err = np.abs(sums[:4] - want_sums[:4]).max()
    print(f"max |sum - ref| = {err:.3e}")
    assert err <= TOL
    assert sums[4] == want_sums[4] and sums[5] == want_sums[5] and sums[6] == 0 and sums[7] == 0


@pytest.mark.parametrize("B,C", SHAPES)
def test_kernel_matches_restatement_contiguous(B, C):
    y, z, sums, counts = _case(B, C)
    _check(_run(torch.as_tensor(y, device=DEV), torch.as_tensor(z, device=DEV)), sums, counts)


@pytest.mark.parametrize("B,C", SHAPES)
def test_kernel_matches_restatement_strided_views(B, C):
    from mvml_gat.metrics import _rows_ld
    y, z, sums, counts = _case(B, C)
    yv, zv = _padded_view(y), _padded_view(z, 1, 6)
    if B > 1:  # passed in place by their leading dimension, not copied
        assert _rows_ld(yv, C)[0] is yv and _rows_ld(yv, C)[1] == C + 5 and _rows_ld(zv, C)[1] == C + 7
    _check(_run(yv, zv), sums, counts)
    # a layout with no unit column stride is made contiguous
    yt = torch.as_tensor(np.ascontiguousarray(y.T), device=DEV).t()
    zt = torch.as_tensor(np.ascontiguousarray(z.T), device=DEV).t()
    _check(_run(yt, zt), sums, counts)


def test_empty_rows_and_nan_acc():
    """Rows with no predicted label, no true label and neither: sklearn's zeros, the counted
    empty unions, and acc NaN for the batch (the reference's 0 / 0)."""
    from mvml_gat import MultiLabelMeter
    y = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    z = np.array([[-1, -1, -1, -1], [2, -1, 3, -1], [-1, -1, -1, -1], [1, -2, 3, -4], [-5, -5, -5, -5]],
                 dtype=np.float32)
    sums, counts = _run(torch.as_tensor(y, device=DEV), torch.as_tensor(z, device=DEV))
    # rows: (no prediction) 0 0 0 0 | (no label) 0 0 0 0 | (neither) 0 0 0 0, empty |
    # t = 1, a = 2, b = 2, union 3: 1/3, 1/2, 1/2, 1/2 | (neither)
    assert sums.tolist() == [1 / 3, 0.5, 0.5, 0.5, 5.0, 2.0, 0.0, 0.0]
    assert counts.tolist() == [[1, 0, 0, 0], [1, 0, 2, 0], [1, 1, 1, 0], [2, 4, 2, 5]]
    want_s, want_c = R.batch_sums(y, z)
    assert sums.tolist() == want_s.tolist() and np.array_equal(counts, want_c)
    meter = MultiLabelMeter(4, DEV)
    meter.update(torch.as_tensor(y[3:4], device=DEV), torch.as_tensor(z[3:4], device=DEV))
    meter.update(torch.as_tensor(y, device=DEV), torch.as_tensor(z, device=DEV))
    r = meter.compute()
    assert np.isnan(r["acc"]) and r["n_empty_union"] == 2
    assert r["acc_per_sample"] == (1 / 3 + 1 / 3) / 6 and r["precision"] == (0.5 + 0.5 / 5) / 2


def test_prediction_rule_boundary_values():
    """p = (z >= 0): 0 and -0.0 give 1, the smallest denormals follow their sign, NaN gives 0."""
    z = torch.tensor([[0.0, -0.0, 1e-45, -1e-45, -1e-3, 1e-3, float("inf"), float("-inf"), float("nan")]],
                     dtype=torch.float32)
    assert z[0, 2].item() > 0 and z[0, 3].item() < 0  # (denormals, not flushed on the way in)
    want = [1, 1, 1, 0, 0, 1, 1, 0, 0]
    assert R.predict(z.numpy())[0].tolist() == want
    sums, counts = _run(torch.ones_like(z).to(DEV), z.to(DEV))
    assert counts[0].tolist() == want and counts[2].tolist() == [1 - p for p in want]
    assert counts[1].tolist() == [0] * 9 and counts[3].tolist() == [0] * 9
    sums, counts = _run(torch.zeros_like(z).to(DEV), z.to(DEV))
    assert counts[1].tolist() == want and counts[3].tolist() == [1 - p for p in want]
    # labels: positive iff y >= 0.5
    yb = torch.tensor([[0.0, 0.49999997, 0.5, 1.0, float("nan"), -1.0, 2.0, 0.25, 0.75]], dtype=torch.float32)
    _, counts = _run(yb.to(DEV), torch.ones_like(z).to(DEV))
    assert counts[0].tolist() == [0, 0, 1, 1, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("B,C", [(4096, 11), (70, 130)])
def test_two_runs_bitwise_equal(B, C):
    y, z, _, _ = _case(B, C)
    yd, zd = torch.as_tensor(y, device=DEV), torch.as_tensor(z, device=DEV)
    a, ca = _run(yd, zd)
    b, cb = _run(yd, zd)
    assert a.tobytes() == b.tobytes() and np.array_equal(ca, cb)


def test_zero_rows():
    sums, counts = _run(torch.zeros(0, 11, device=DEV), torch.zeros(0, 11, device=DEV))
    assert sums.tolist() == [0.0] * 8 and not counts.any()


def _kegg_like_batches():
    rng = np.random.default_rng(5)
    return [R.random_batch(rng, n, 11) for n in (64, 64, 36)]  # KEGG's short last batch


def _assert_result(got, want):
    for k in ("acc", "precision", "recall", "f1_score"):
        # per-batch sums within TOL (above) divided by >= 36 rows
        assert abs(got[k] - want[k]) <= TOL and abs(got[k + "_per_sample"] - want[k + "_per_sample"]) <= TOL
    assert got["n_batches"] == want["n_batches"] and got["n_samples"] == want["n_samples"]
    assert got["class_counts"] == want["class_counts"]
    for a, b in zip(got["class_wise"], want["class_wise"]):
        assert a == b


def test_meter_batches_growth_and_reset():
    from mvml_gat import MultiLabelMeter
    batches = _kegg_like_batches()
    want = R.meter_ref(batches)
    assert want["f1_score"] != want["f1_score_per_sample"]  # the two rules differ on this input
    dev = [(torch.as_tensor(y, device=DEV), torch.as_tensor(z, device=DEV)) for y, z in batches]
    meter = MultiLabelMeter(11, DEV, capacity=2)
    for y, z in dev:
        meter.update(y, z)
    assert meter.capacity == 4 and meter.n_batches == 3  # grew past the initial capacity
    _assert_result(meter.compute(), want)
    _assert_result(meter.compute(), want)  # compute() does not consume the buffers
    extra = meter.compute(extra=torch.tensor([1.5, 2.5], device=DEV))["extra"]
    assert extra == [1.5, 2.5]
    meter.reset()
    assert meter.n_batches == 0 and not meter.class_counts.any() and not meter.sums.any()
    for y, z in dev[1:]:
        meter.update(y, z)
    _assert_result(meter.compute(), R.meter_ref(batches[1:]))
    for _ in range(3):  # 5 batches: a second doubling
        meter.update(*dev[0])
    assert meter.capacity == 8
    _assert_result(meter.compute(), R.meter_ref(batches[1:] + [batches[0]] * 3))


def test_update_does_not_synchronize():
    from mvml_gat import MultiLabelMeter
    y, z = (torch.as_tensor(a, device=DEV) for a in _kegg_like_batches()[0])
    meter = MultiLabelMeter(11, DEV, capacity=1)
    meter.update(y, z)  # warm-up: library load, workspace allocation
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"this torch build rejects set_sync_debug_mode on HIP: {e}")
    try:
        meter.update(y, z)                   # grows the buffer: a device copy in stream order
        meter.update(_padded_view_nosync(y), z)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert meter.n_batches == 3
    r = meter.compute()
    assert r["n_samples"] == 192 and r["acc"] == r["acc_per_sample"]


def _padded_view_nosync(t):
    wide = torch.zeros(t.shape[0], t.shape[1] + 4, dtype=t.dtype, device=t.device)
    wide[:, 1:1 + t.shape[1]].copy_(t)
    return wide[:, 1:1 + t.shape[1]]


def test_drop_in_evaluate_and_class_wise(capsys):
    from mvml_gat import evaluate, evaluate_class_wise
    y, z = _kegg_like_batches()[2]
    yd, zd = torch.as_tensor(y, device=DEV), torch.as_tensor(z, device=DEV)
    sums, counts = R.batch_sums(y, z)
    want = R.batch_means(sums)
    acc, pre, rec, f1, acc_weight = evaluate(yd, zd)
    for g, w in zip((acc, pre, rec, f1), want):
        assert isinstance(g, float) and abs(g - w) <= TOL
    assert acc_weight.device.type == "cpu" and acc_weight.dtype == torch.float32
    assert tuple(acc_weight.shape) == (36, 11)
    assert torch.equal(acc_weight, torch.as_tensor(counts[1] + counts[2]).float().expand(36, 11))
    lists = evaluate_class_wise(yd, zd)
    assert lists == R.class_wise(counts)
    out = capsys.readouterr().out
    assert out.count("Binary Classification Statistics:") == 11
    assert ("Class 1 Binary Classification Statistics:\nAccuracy(Binary) %.4f, Precision(Binary) %.4f, "
            "Recall(Binary) %.4f, F1-Score(Binary) %.4f\n" % tuple(l[0] for l in lists)) in out
    assert evaluate_class_wise(yd, zd, verbose=False) == lists and capsys.readouterr().out == ""
