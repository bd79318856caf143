"""PNALocal (reference models/legacy/pna_local.py; `model_type: 'PNALocal'` of configs/old_configs/contrastive_local.yml) on the
MI355X kernels: the PNA message-passing stack without a readout - every atom keeps an embedding, relu(projection_head(feat)) over
all N node rows - for the local-global contrastive loss (losses.NTXentLocalGlobal).

Same constructor kwargs (`node_dim`, `edge_dim` accepted, unknown ones swallowed), sub-module names (`node_gnn`,
`projection_head`) and side effect (`ndata['feat']` holds the returned [N, target_dim] tensor): a reference checkpoint loads strict.
The BatchNorm of the projection head takes its statistics over the nodes.  The ReLU is the post-activation of the head's last
block (layers.FCSpec.post_act): the activation kernel behind the block's GEMM, one launch.

The model runs as one tape node (tape.run_model), as PNA._forward does; the whole-model sequencer of PNA (pna_native) is built around
the per-graph readout and does not apply.
"""
from typing import Callable, List, Union

from torch import nn

from . import tape
from .graph import as_batched_graph
from .layers import MLP, bn_counter_scope
from .pna import PNAGNN


class PNALocal(nn.Module):
    """reference models/legacy/pna_local.py:13-69.  forward(g) -> [N, target_dim]; g: BatchedMolGraph or a DGL graph of bond graphs."""

    def __init__(self, node_dim=None, edge_dim=None, hidden_dim=None, target_dim=None, aggregators: List[str] = None,
                 scalers: List[str] = None, readout_batchnorm: bool = True, readout_hidden_dim=None, readout_layers: int = 2,
                 residual: bool = True, pairwise_distances: bool = False, activation: Union[Callable, str] = "relu",
                 last_activation: Union[Callable, str] = "none", mid_batch_norm: bool = False, last_batch_norm: bool = False,
                 propagation_depth: int = 5, dropout: float = 0.0, posttrans_layers: int = 1, pretrans_layers: int = 1, **kwargs):
        super().__init__()
        if hidden_dim is None or target_dim is None or aggregators is None or scalers is None:
            raise TypeError('PNALocal needs hidden_dim, target_dim, aggregators and scalers')
        self.node_gnn = PNAGNN(hidden_dim=hidden_dim, aggregators=aggregators, scalers=scalers, residual=residual,
                               pairwise_distances=pairwise_distances, activation=activation, last_activation=last_activation,
                               mid_batch_norm=mid_batch_norm, last_batch_norm=last_batch_norm,
                               propagation_depth=propagation_depth, dropout=dropout, posttrans_layers=posttrans_layers,
                               pretrans_layers=pretrans_layers)
        if readout_hidden_dim is None:
            readout_hidden_dim = hidden_dim
        self.projection_head = MLP(in_dim=hidden_dim, hidden_size=readout_hidden_dim, mid_batch_norm=readout_batchnorm,
                                   out_dim=target_dim, layers=readout_layers)

    def forward(self, graph, *unused):
        g = as_batched_graph(graph)
        with bn_counter_scope():
            out = tape.run_model(self, lambda: self._forward(g))      # one autograd node for the whole model
        g.ndata['feat'] = out                                         # reference side effect (:65-66): the returned tensor itself
        return out

    def _forward(self, g):
        self.node_gnn(g)
        return self.projection_head(g.ndata['feat'], post_act='relu')
