"""The reference's training driver (main.py:18-116) on this library.

    python -m mvml_gat.train --data kegg_dataset.csv --index data_index.txt

runs main.py's protocol: per iteration a fresh MVP, FlatAdam (main.py:88's Adam),
ExponentialLR(gamma=0.95), EarlyStopping(mode='higher', patience=15) on the validation F1, the
test pass on the best checkpoint, and ``10_test_results.csv`` at the end.  The per-batch
``evaluate(labels, pred)`` of main.py:32 / 52 / 105 is a MultiLabelMeter update (one kernel on
the stream), so a phase synchronises once, when its metrics are read.

The pieces are usable on their own: EarlyStopping (dgllife 0.3.0's behaviour and checkpoint
format, so a reference ``net_i.pkl`` loads here and ours loads there), MVPDataSet / collate_mvp
(dataset.py:16-59 from the restated featuriser, tokeniser and fingerprints), run_epoch,
evaluate_loader and fit.
"""
import argparse
import ast
import csv
import os

import numpy as np
import torch

from .featurize import FEAT_SIZE, MolDataSet
from .featurize import collate as collate_graphs
from .fingerprints import fingerprints
from .metrics import MultiLabelMeter
from .mvp import MVP, train_step
from .optim import FlatAdam
from .smiles import collate_smiles, tokens_struct

_METRICS = ("acc", "precision", "recall", "f1_score")


class EarlyStopping:
    """dgllife.utils.EarlyStopping (0.3.0) as main.py:90 uses it.  ``step(score, model)`` saves
    on the first call; afterwards it saves and resets the counter whenever the score is
    strictly better (mode 'higher': larger), otherwise counts up and sets ``early_stop`` once
    ``counter >= patience``; it returns ``early_stop``.  The checkpoint is
    ``torch.save({'model_state_dict': model.state_dict()}, filename)``."""

    def __init__(self, mode='higher', patience=10, filename=None):
        if mode not in ('higher', 'lower'):
            raise ValueError(f"EarlyStopping: mode 'higher' or 'lower', got {mode!r}")
        if filename is None:
            filename = os.path.join(os.getcwd(), 'early_stop.pth')
        self.mode = mode
        self.patience = patience
        self.filename = filename
        self.counter = 0
        self.timestep = 0
        self.best_score = None
        self.early_stop = False

    def _better(self, score, best):
        return score > best if self.mode == 'higher' else score < best

    def step(self, score, model):
        self.timestep += 1
        if self.best_score is None:
            self.best_score = score
            self.save_checkpoint(model)
        elif self._better(score, self.best_score):
            self.best_score = score
            self.save_checkpoint(model)
            self.counter = 0
        else:
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True
        return self.early_stop

    def save_checkpoint(self, model):
        torch.save({'model_state_dict': model.state_dict()}, self.filename)

    def load_checkpoint(self, model):
        model.load_state_dict(torch.load(self.filename, map_location='cpu')['model_state_dict'])


class MVPDataSet:
    """dataset.py:16-49: rows of a (smiles, label) CSV as the three views' inputs.
    ``ds[i]`` -> (smiles string, MolGraph with ndata['h'], fingerprint f32[2513], multi-hot
    label f32[num_classes]).  The graphs are built once and cached (featurize.MolDataSet) and
    the fingerprints are computed once, at construction (``fps``: precomputed [len, 2513]
    fingerprints of the rows, to skip that)."""

    def __init__(self, data_path, labels_split=',', num_classes=11, fps=None):
        self.mols = MolDataSet(data_path, labels_split, num_classes)
        self.smiles = self.mols.smiles
        self.num_classes = num_classes
        self.fps = np.asarray(fingerprints(self.smiles) if fps is None else fps, dtype=np.float32)
        if self.fps.shape[0] != len(self.smiles):
            raise ValueError("MVPDataSet: one fingerprint row per molecule")
        self.feat_size = FEAT_SIZE

    def __len__(self):
        return len(self.smiles)

    def __getitem__(self, index):
        graph, y = self.mols[index]
        return self.smiles[index], graph, self.fps[index], y


_VOCAB = tokens_struct()


def collate_mvp(samples):
    """dataset.py:52-59: (batch_smiles {'smiles', 'seq_len'}, batch_graph, fps_t, labels)."""
    smiles, graphs, fps, labels = zip(*samples)
    batch_graph, y = collate_graphs(list(zip(graphs, labels)))
    return collate_smiles(list(smiles), _VOCAB), batch_graph, torch.as_tensor(np.stack(fps)), y.float()


def to_device(batch, device):
    """main.py:25-30: a collate_mvp batch as train_step's (smiles, graphs, atom_feats, fp_t,
    labels) on the device."""
    batch_smiles, batch_graph, fps_t, labels = batch
    g = batch_graph.to(device)
    smiles = {"smiles": batch_smiles["smiles"].to(device), "seq_len": batch_smiles["seq_len"]}
    return smiles, g, g.ndata["h"].to(device), fps_t.to(device), labels.to(device)


def run_epoch(model, optimizer, loader, meter, reducer=None, device=None):
    """main.py:24-36: one training pass over the loader, every batch scored into ``meter``.
    Returns (the sum of the batch losses as a device tensor, the number of batches): nothing is
    read back here."""
    device = device or meter.device
    model.train()
    loss_sum, n = torch.zeros((), dtype=torch.float64, device=device), 0
    for batch in loader:
        loss = train_step(model, optimizer, to_device(batch, device), reducer, meter=meter)
        loss_sum += loss.detach().reshape(())
        n += 1
    return loss_sum, n


def evaluate_loader(model, loader, meter, device=None):
    """main.py:41-53: eval mode under no_grad, every batch scored into ``meter`` (reset first);
    returns meter.compute()."""
    device = device or meter.device
    model.eval()
    meter.reset()
    with torch.no_grad():
        for batch in loader:
            smiles, g, atom_feats, fp_t, labels = to_device(batch, device)
            meter.update(labels, model(smiles, g, atom_feats, fp_t))
    return meter.compute()


def _num_classes(model):
    return [m for m in model.mlp if isinstance(m, torch.nn.Linear)][-1].out_features


def fit(model, optimizer, scheduler, stopper, train_loader, val_loader, epochs, device, log=print,
        reducer=None):
    """main.py:18-61.  Per epoch: the training pass, one meter.compute() for it (the loss sum
    rides on the same copy), the validation pass and its compute(), scheduler.step(), then
    stopper.step(val['f1_score'], model).  Returns the history, one dict per epoch: ``epoch``,
    ``lr`` (the rate the epoch trained with), ``loss`` (mean batch loss), ``train`` and ``val``
    (the meter's results) and ``saved`` (the stopper wrote a checkpoint after this epoch)."""
    meter = MultiLabelMeter(_num_classes(model), device)
    history = []
    for epoch in range(epochs):
        cur_lr = optimizer.param_groups[0]["lr"]
        meter.reset()
        loss_sum, n = run_epoch(model, optimizer, train_loader, meter, reducer, device)
        train = meter.compute(extra=loss_sum)
        loss = train.pop("extra")[0] / n if n else float("nan")
        val = evaluate_loader(model, val_loader, meter, device)
        scheduler.step()
        early_stop = stopper.step(val["f1_score"], model)
        saved = stopper.counter == 0  # (a step that does not save counts up)
        history.append({"epoch": epoch, "lr": cur_lr, "loss": loss, "train": train, "val": val, "saved": saved})
        if log is not None:
            log(f"epoch:{epoch}---loss:{loss}---train_acc:{train['acc']}---validation---acc:{val['acc']}"
                f"---precision:{val['precision']}---recall:{val['recall']}---f1_score:{val['f1_score']}"
                f"----lr:{cur_lr}")
        if early_stop:
            break
    return history


# ------------------------------------------------------------------------------------------ CLI
class _Args(argparse.Namespace):
    """parse()'s namespace: defaults of the options that are not in config.py."""
    READOUTS = ("set2set", "weighted_sum_max")
    graph_readout = "set2set"
    CONVS = ("gat", "gatv2")
    graph_conv = "gat"


def parse(argv=None):
    """config.py's flags and defaults, plus --data / --index (the dataset CSV and the split
    file, data_index.txt: three Python lists of row indices, are not shipped)."""
    p = argparse.ArgumentParser(prog="python -m mvml_gat.train", description=__doc__.split("\n\n")[0])
    p.add_argument("--data", type=str, required=True, help="the (smiles, label) CSV (kegg_dataset.csv)")
    p.add_argument("--index", type=str, required=True,
                   help="the split file: train / validation / test row indices, one list per line")
    p.add_argument("-o", "--output", type=str, default="./output/", help="the path of output model")
    p.add_argument("-c", "--class_num", type=int, default=11, help="the dimension of output")
    p.add_argument("-i", "--iterations", type=int, default=10, help="the number of running model")
    p.add_argument("-e", "--epoch", type=int, default=100, help="the max number of epoch")
    p.add_argument("-s", "--seed", type=int, default=1, help="random seed")
    p.add_argument("--hidden_feats", type=int, nargs="+", default=[192, 384],
                   help="the size of node representations after the i-th GAT layer (the last one, "
                        "the fusion head's width: a multiple of 4 in [16, 384])")
    p.add_argument("--rnn_embed_dim", type=int, default=128, help="the embedding size of each SMILES token")
    p.add_argument("--rnn_hidden_dim", type=int, default=384,
                   help="the number of features in the RNN hidden state")
    p.add_argument("--rnn_layers", type=int, default=2, help="the number of rnn layers")
    p.add_argument("--fp_dim", type=int, default=512, help="the hidden size of fingerprints module")
    p.add_argument("--head", type=int, default=12, help="the head size of attention; must be 12 (the reference's Conv2d(12, 12, 3) is "
                        "fixed whatever this says)")
    p.add_argument("--p", type=float, default=0.5, help="dropout probability")
    p.add_argument("--lr", type=float, default=1e-3, help="learning rate")
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--batch_size", type=int, default=64)
    # not one of config.py's flags: the default lives on the namespace's class, so the parsed
    # attributes of a reference command line are config.py's and nothing else (vars(args))
    p.add_argument("--graph_readout", type=str, default=argparse.SUPPRESS, choices=list(_Args.READOUTS),
                   help="the graph view's readout: set2set (the reference's, the default) or "
                        "weighted_sum_max (dgllife's WeightedSumAndMax: one pass over the atom rows, no LSTM)")
    p.add_argument("--graph_conv", type=str, default=argparse.SUPPRESS, choices=list(_Args.CONVS),
                   help="the graph view's convolution: gat (the reference's, the default) or gatv2 "
                        "(dgllife's GATv2: dynamic attention, scored from the whole source row per edge)")
    return p.parse_args(argv, namespace=_Args())


def read_index(path):
    """data_index.txt (main.py:68-73): one Python list of row indices per line."""
    with open(path) as f:
        return [list(ast.literal_eval(line)) for line in f if line.strip()]


def set_random_seed(seed):
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def main(args, log=print):
    """main.py:64-116.  Returns the per-iteration test results (acc, precision, recall, f1)."""
    from torch.utils.data import DataLoader, Subset
    if not torch.cuda.is_available():
        raise RuntimeError("mvml_gat.train needs a GPU (there is no CPU fallback)")
    device = "cuda:0"
    set_random_seed(args.seed)
    os.makedirs(args.output, exist_ok=True)
    dataset = MVPDataSet(args.data, num_classes=args.class_num)
    index = read_index(args.index)
    loaders = [DataLoader(Subset(dataset, idx), batch_size=args.batch_size, collate_fn=collate_mvp)
               for idx in index[:3]]
    train_loader, val_loader, test_loader = loaders
    mean_results = []
    out_csv = os.path.join(args.output, "10_test_results.csv")
    for iteration in range(args.iterations):
        model = MVP(num_classes=args.class_num, in_feats=dataset.feat_size, hidden_feats=args.hidden_feats,
                    rnn_embed_dim=args.rnn_embed_dim, blstm_dim=args.rnn_hidden_dim,
                    blstm_layers=args.rnn_layers, fp_2_dim=args.fp_dim, dropout=args.p,
                    num_heads=args.head, device=device, graph_readout=args.graph_readout,
                    graph_conv=args.graph_conv).to(device)
        optimizer = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
        scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.95)
        stopper = EarlyStopping(mode='higher', filename=os.path.join(args.output, f'net_{iteration}.pkl'),
                                patience=15)
        fit(model, optimizer, scheduler, stopper, train_loader, val_loader, args.epoch, device,
            log=None if log is None else (lambda s, it=iteration: log(f"[iter:{it}] {s}")))
        stopper.load_checkpoint(model)
        r = evaluate_loader(model, test_loader, MultiLabelMeter(args.class_num, device), device)
        if log is not None:
            log(f"test_---acc:{r['acc']}---precision:{r['precision']}---recall:{r['recall']}"
                f"---f1_score:{r['f1_score']}")
        mean_results.append([r[k] for k in _METRICS])
        m = np.mean(mean_results, axis=0)
        if log is not None:
            log(f"mean_test_---acc:{m[0]}---precision:{m[1]}---recall:{m[2]}---f1_score:{m[3]}")
        with open(out_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(_METRICS)
            w.writerows([[repr(float(v)) for v in row] for row in mean_results])
    return mean_results


if __name__ == "__main__":
    main(parse())
