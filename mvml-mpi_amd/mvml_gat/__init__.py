"""mvml_gat — MI355X-native molecular-graph (GAT) view of MVML-MPI.

Drop-in for the reference's graph view (model.py:77-95) on the HIP path:

    from mvml_gat import GNNModule, batch
    bg = batch(graphs).to("cuda")                 # dgl.batch + device-side CSR build
    emb = GNNModule(74, [192, 384], 0.5, 6, 3).cuda()(bg, bg.ndata["h"])   # (B, 384)

All arithmetic of the training step runs in hand-written HIP kernels (libmvml_gat.so, C ABI in
include/mvml_gat.h); main.py:88's optimizer is ``FlatAdam(model.parameters(), lr=...,
weight_decay=...)`` (Adam on the device, one gradient all-reduce), main.py:32's per-batch
``evaluate`` is ``MultiLabelMeter.update`` (one kernel, no host read-back) and main.py's loop is
``mvml_gat.train``.  There is no CPU fallback: ops raise if the library is missing or the
tensors are not on the GPU.
"""
from ._lib import MvmlError, lib
from .batching import BatchedMolGraph, MolGraph, batch, bigraph_from_bonds, from_arrays, graph
from .fusion import FPNModule, MVFusion, bce_with_logits
from .smiles import RNNModule, collate_smiles, tokens_struct
from .nn import GAT, GATConv, GATLayer, GATv2, GATv2Conv, GATv2Layer, GNNModule, GraphNorm, Set2Set, WeightAndSum, WeightedSumAndMax
from .nn import GATPredictor, GATv2Predictor, MLPPredictor
from .nn import GCN, GCNLayer, GCNPredictor, GraphConv
from .nn import GraphSAGE, GraphSAGEPredictor, SAGEConv
from .nn import GIN, GINLayer, GINPredictor
from .optim import FlatAdam
from .mvp import MVP
from .metrics import MultiLabelMeter, evaluate, evaluate_class_wise

__all__ = ["MultiLabelMeter", "evaluate", "evaluate_class_wise","GNNModule", "MVFusion", "FPNModule", "RNNModule", "tokens_struct", "collate_smiles", "bce_with_logits", "GAT", "GATLayer", "GATConv", "GATv2", "GATv2Layer", "GATv2Conv", "Set2Set", "WeightAndSum", "WeightedSumAndMax", "GATPredictor", "GATv2Predictor", "MLPPredictor", "GraphConv", "GCNLayer", "GCN", "GCNPredictor", "SAGEConv", "GraphSAGE", "GraphSAGEPredictor", "GINLayer", "GIN", "GINPredictor", "GraphNorm", "BatchedMolGraph",
           "MolGraph", "batch", "graph", "bigraph_from_bonds", "from_arrays", "lib", "MvmlError", "FlatAdam", "MVP"]
__version__ = "0.1.0"
