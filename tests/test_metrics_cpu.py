"""CPU tests of the metrics / training-driver feature: the float64 restatement against the literal
reference formulas (utils.py:109-135), EarlyStopping's sequence and checkpoint format, the C
ABI's argument validation without a GPU, the CLI defaults (config.py) and the two-rank gloo
reduction of the per-batch sums and class counts."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _metrics_ref as R


# ------------------------------------------------------------------ restatement vs reference
def _reference_evaluate(y, z):
    """utils.py:109-135 literally, on float64 logits (|z| >= 1e-3: sigmoid(z) >= 0.5 is z >= 0)."""
    from sklearn.metrics import f1_score, precision_score, recall_score
    zs = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    ts = y.astype(int)
    preds = np.array([(x >= 0.5).astype(int) for x in zs]).astype(int)
    count = 0
    for i in range(ts.shape[0]):
        p = sum(np.logical_and(ts[i], preds[i]))
        q = sum(np.logical_or(ts[i], preds[i]))
        count += p / q
    counts = [sum(ts[:, i] ^ preds[:, i]) for i in range(ts.shape[1])]
    return (count / ts.shape[0],
            precision_score(ts, preds, average="samples", zero_division=0),
            recall_score(ts, preds, average="samples", zero_division=0),
            f1_score(ts, preds, average="samples", zero_division=0), counts)


@pytest.mark.parametrize("B", [1, 64, 257])
def test_restatement_matches_reference_formulas(B):
    rng = np.random.default_rng(100 + B)
    y, z = R.random_batch(rng, B, 11)
    sums, counts = R.batch_sums(y, z)
    acc, pre, rec, f1, mism = _reference_evaluate(y, z)
    got = R.batch_means(sums)
    # float64 sums of < 300 terms in [0, 1]
    assert abs(got[0] - acc) <= 1e-15 and abs(got[1] - pre) <= 1e-15
    assert abs(got[2] - rec) <= 1e-15 and abs(got[3] - f1) <= 1e-15
    assert sums[4] == B and sums[5] == 0
    assert (counts[1] + counts[2]).tolist() == [int(c) for c in mism]
    assert (counts.sum(0) == B).all()


def test_restatement_class_wise_matches_sklearn_binary():
    from sklearn.metrics import accuracy_score, f1_score, precision_score, recall_score
    rng = np.random.default_rng(7)
    y, z = R.random_batch(rng, 64, 11)
    y[:, 3] = 0  # a class with no positive label: precision / recall / F1 fall to 0
    p = R.predict(z)
    _, counts = R.batch_sums(y, z)
    got = R.class_wise(counts)
    for c in range(11):
        t = y[:, c].astype(int)
        want = [accuracy_score(t, p[:, c]), precision_score(t, p[:, c], zero_division=0),
                recall_score(t, p[:, c], zero_division=0), f1_score(t, p[:, c], zero_division=0)]
        for k in range(4):
            assert abs(got[k][c] - want[k]) <= 1e-15, (c, k)


def test_host_summary_is_mean_over_batches_of_batch_means():
    """MultiLabelMeter's host half (metrics.summarize) on the restatement's sums: a short last
    batch weighs as much as a full one; the per-sample variants weigh rows; an empty-union row
    makes that batch's acc NaN."""
    from mvml_gat.metrics import summarize
    rng = np.random.default_rng(3)
    batches = [R.random_batch(rng, n, 11) for n in (64, 64, 36)]
    pairs = [R.batch_sums(y, z) for y, z in batches]
    got = summarize([s.tolist() for s, _ in pairs], sum(c for _, c in pairs).tolist())
    want = R.meter_ref(batches)
    for k in ("acc", "precision", "recall", "f1_score"):
        assert got[k] == want[k] and got[k + "_per_sample"] == want[k + "_per_sample"]
        assert got[k] != got[k + "_per_sample"]
    assert got["n_batches"] == 3 and got["n_samples"] == 164
    assert got["class_counts"] == want["class_counts"] and got["class_wise"] == want["class_wise"]
    y, z = batches[2]
    y[5], z[5] = 0.0, -1.0
    s, c = R.batch_sums(y, z)
    assert s[5] == 1
    bad = summarize([pairs[0][0].tolist(), s.tolist()], (pairs[0][1] + c).tolist())
    assert np.isnan(bad["acc"]) and np.isfinite(bad["acc_per_sample"]) and bad["n_empty_union"] == 1
    assert np.isfinite(bad["f1_score"])


# ------------------------------------------------------------------ EarlyStopping
def test_early_stopping_sequence_and_checkpoint(tmp_path):
    from mvml_gat.train import EarlyStopping
    path = str(tmp_path / "net_0.pkl")
    stopper = EarlyStopping(mode='higher', patience=2, filename=path)
    model = torch.nn.Linear(3, 2)
    saved, stops, counters = [], [], []
    write = stopper.save_checkpoint
    stopper.save_checkpoint = lambda m: (saved.append(stopper.timestep), write(m))
    for step, score in enumerate([0.5, 0.6, 0.6, 0.55, 0.7], 1):
        with torch.no_grad():
            model.weight.fill_(float(step))
        stops.append(stopper.step(score, model))
        counters.append(stopper.counter)
    assert saved == [1, 2, 5]
    assert counters[2] == 1          # a tie is not better
    assert stops == [False, False, False, True, True] and stopper.early_stop
    assert stopper.best_score == 0.7
    ckpt = torch.load(path)
    assert list(ckpt) == ["model_state_dict"]
    fresh = torch.nn.Linear(3, 2)
    stopper.load_checkpoint(fresh)
    assert torch.equal(fresh.weight, torch.full((2, 3), 5.0)) and torch.equal(fresh.bias, model.bias)
    # a checkpoint written the reference's way (dgllife: the same key) loads too
    torch.save({'model_state_dict': torch.nn.Linear(3, 2).state_dict(), 'timestep': 3}, path)
    stopper.load_checkpoint(fresh)


# ------------------------------------------------------------------ C ABI
def test_metrics_abi_validation_without_gpu():
    from mvml_gat import _lib
    L = _lib.lib()
    f = L.mvml_multilabel_metrics
    assert f(-1, 11, None, 11, None, 11, None, None, None, 0, None) == 1
    assert b"negative" in L.mvml_last_error()
    assert f(4, 0, None, 11, None, 11, None, None, None, 0, None) == 1
    assert b"classes" in L.mvml_last_error()
    assert f(4, 11, None, 10, None, 11, None, None, None, 0, None) == 1
    assert b"leading" in L.mvml_last_error()
    assert f(4, 11, None, 11, None, 10, None, None, None, 0, None) == 1
    need = L.mvml_multilabel_metrics_workspace_size(4, 11)
    assert need > 0 and L.mvml_multilabel_metrics_workspace_size(0, 11) == 0
    assert L.mvml_multilabel_metrics_workspace_size(1 << 40, 11) == L.mvml_multilabel_metrics_workspace_size(65536, 11)
    assert f(4, 11, None, 11, None, 11, None, None, None, 0, None) == 3
    assert b"workspace" in L.mvml_last_error()
    buf = (np.zeros(need, dtype=np.uint8)).ctypes.data
    assert f(4, 11, None, 11, None, 11, None, None, buf, need - 1, None) == 3


# ------------------------------------------------------------------ CLI
def test_cli_defaults_match_reference_config():
    from mvml_gat.train import parse
    a = parse(["--data", "d.csv", "--index", "i.txt"])
    assert vars(a) == dict(data="d.csv", index="i.txt", output="./output/", class_num=11, iterations=10,
                           epoch=100, seed=1, hidden_feats=[192, 384], rnn_embed_dim=128,
                           rnn_hidden_dim=384, rnn_layers=2, fp_dim=512, head=12, p=0.5, lr=1e-3,
                           weight_decay=1e-4, batch_size=64)
    with pytest.raises(SystemExit):
        parse([])


def test_read_index_and_collate(tmp_path):
    """The split file format of main.py:68-73, and collate_mvp's (batch_smiles, batch_graph, fps_t,
    labels) of dataset.py:52-59 on the first golden molecules."""
    from mvml_gat.fingerprints import FP_SIZE, kegg_pool
    from mvml_gat.train import MVPDataSet, collate_mvp, read_index
    p = tmp_path / "data_index.txt"
    p.write_text("[0, 2, 4]\n[1]\n[3, 5]\n")
    assert read_index(str(p)) == [[0, 2, 4], [1], [3, 5]]
    here = os.path.dirname(os.path.abspath(__file__))
    ds = MVPDataSet(os.path.join(here, "golden", "kegg_test_split.csv"), fps=kegg_pool())
    smiles, graph, fps_t, labels = collate_mvp([ds[i] for i in (0, 2, 4)])
    assert smiles["smiles"].shape[0] == 3 and smiles["seq_len"] == [len(ds.smiles[i]) for i in (0, 2, 4)]
    assert graph.batch_size == 3 and graph.ndata["h"].shape[1] == ds.feat_size == 74
    assert fps_t.shape == (3, FP_SIZE) and fps_t.dtype == torch.float32
    assert labels.shape == (3, 11) and labels.dtype == torch.float32 and (labels.sum(1) >= 1).all()


# ------------------------------------------------------------------ two-rank reduction
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_SIZES = (64, 64, 36)
_CUTS = (40, 17, 36)  # rank 0 holds the first _CUTS[i] rows of batch i; rank 1's last shard is empty


def _batches():
    rng = np.random.default_rng(11)
    return [R.random_batch(rng, n, 11) for n in _SIZES]


def _reduce_worker(rank, world, port, out):
    from mvml_gat.metrics import reduce_metric_buffers, summarize
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sums, counts = [], np.zeros((4, 11), dtype=np.int64)
    for (y, z), cut in zip(_batches(), _CUTS):
        sl = slice(0, cut) if rank == 0 else slice(cut, None)
        s, c = R.batch_sums(y[sl], z[sl])
        sums.append(s)
        counts += c
    sums, counts = reduce_metric_buffers(torch.as_tensor(np.stack(sums)), torch.as_tensor(counts))
    if rank == 0:
        out.put(summarize(sums.tolist(), counts.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_metric_reduction_matches_whole_batches():
    want = R.meter_ref(_batches())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert got["n_batches"] == 3 and got["n_samples"] == sum(_SIZES)
    assert got["class_counts"] == want["class_counts"] and got["class_wise"] == want["class_wise"]
    for k in ("acc", "precision", "recall", "f1_score"):
        # two shard sums added instead of one sum over the batch: <= 2 ulp of a sum <= 64
        # (2.8e-14) over >= 36 rows
        assert abs(got[k] - want[k]) <= 1e-15, k
        assert abs(got[k + "_per_sample"] - want[k + "_per_sample"]) <= 1e-15, k
