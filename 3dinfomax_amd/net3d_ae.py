"""Net3DAE (the 3D autoencoder variant of 3D-Infomax) on the MI355X kernels - drop-in for reference models/net3d_VAE.py:15-135.

Same constructor kwargs (unknown ones swallowed), same sub-module names (`edge_input`, `node_embedding` / `atom_encoder`,
`encoder_layers`, `decoder_layers`, `node_wise_output_network`, `node_projection_net`, `distance_net`), hence the same state_dict keys
and shapes: reference checkpoints load strict.  forward(graph, pairwise_indices) -> (latent_vector [B, H * len(readout_aggregators)],
distances [P, 1]); as in the reference, graph.ndata['feat'] is left holding the node state the pair head read and graph.edata['d'] is
overwritten (edge-id order).

The trunk is Net3D's (Net3DLayer.step, ReadoutFn, the tape and the composites), encoder and decoder layers on one node / edge state,
the latent vector read out in between (no output MLP).  The pair head:
  * distance_net=False: node_projection_net (if any), then ||p_i - p_j||                       (pair_head._PairNormFn)
  * distance_net of one Linear:  u = (W_a + W_b) h per node, softplus(u_i + u_j + 2b)          (pair_head._PairSumHeadFn)
  * distance_net of two layers (every reference configuration: Linear -> ReLU -> BatchNorm -> Linear(D -> 1)): the fused head of
    csrc/pairmlp.hip (pair_head._PairMLPHeadFn) - nothing of size [P, 2H] or [P, D] is written
  * deeper, wider than the kernel is built for, or with options it does not carry (dropout, synchronised statistics): the composed
    path - both [P, 2H] concatenations, the MLP on each (two sets of batch statistics), softplus of the sum.
FUSED_PAIR_HEAD = False forces the composed path (same arithmetic up to summation order; the tests cross-check the two).

The reference's quirks are kept: `node_wise_encoder_layers` and `node_wise_output_layers` both assign `node_wise_output_network` (the
later assignment wins), and that network runs only when node_wise_encoder_layers > 0, after the encoder.
"""
from typing import List

import torch
import torch.nn as nn

from . import ops, streams, tape
from .graph import as_batched_graph
from .layers import MLP, ReadoutFn, bn_counter_scope
from .mol_encoder import AtomEncoder
from .net3d import Net3DLayer, _BroadcastRowFn
from .pair_head import (_PairConcatFn, _PairMLPHeadFn, _PairNormFn, _PairSumHeadFn, _SoftplusSumToPairsFn, pair_index)

FUSED_PAIR_HEAD = True


class Net3DAE(nn.Module):
    """reference models/net3d_VAE.py:15-135."""

    def __init__(self, node_dim, edge_dim, hidden_dim, readout_aggregators: List[str], batch_norm=False, node_wise_encoder_layers=0,
                 node_wise_output_layers=0, batch_norm_momentum=0.1, reduce_func='sum', dropout=0.0, encoder_depth: int = 4,
                 decoder_depth: int = 4, projection_dim=3, distance_net=True, projection_layers=1, fourier_encodings=0,
                 activation: str = 'SiLU', update_net_layers=2, message_net_layers=2, use_node_features=False, **kwargs):
        super().__init__()
        if encoder_depth < 0 or decoder_depth < 0:
            raise ValueError(f'encoder_depth={encoder_depth}, decoder_depth={decoder_depth}: depths cannot be negative')
        if distance_net and projection_layers > 1 and projection_dim <= 0:
            raise ValueError(f'distance_net with projection_layers={projection_layers} needs projection_dim > 0 (the hidden width of '
                             'distance_net)')
        unknown_readout = [a for a in readout_aggregators if a not in ('sum', 'mean', 'max', 'min')]
        if unknown_readout:
            raise NotImplementedError(f'readout_aggregators={unknown_readout}: dgl.readout_nodes takes sum, mean, max and min')
        self.fourier_encodings = fourier_encodings
        edge_in_dim = 1 if fourier_encodings == 0 else 2 * fourier_encodings + 1
        self.edge_input = MLP(in_dim=edge_in_dim, hidden_size=hidden_dim, out_dim=hidden_dim, mid_batch_norm=batch_norm,
                              last_batch_norm=batch_norm, batch_norm_momentum=batch_norm_momentum, layers=1,
                              mid_activation=activation, dropout=dropout, last_activation=activation)
        self.use_node_features = use_node_features
        if self.use_node_features:
            self.atom_encoder = AtomEncoder(hidden_dim)
        else:
            self.node_embedding = nn.Parameter(torch.empty((hidden_dim,)))
            nn.init.normal_(self.node_embedding)

        def layer():
            return Net3DLayer(edge_dim=hidden_dim, hidden_dim=hidden_dim, batch_norm=batch_norm, batch_norm_momentum=batch_norm_momentum,
                              dropout=dropout, mid_activation=activation, reduce_func=reduce_func,
                              message_net_layers=message_net_layers, update_net_layers=update_net_layers)
        self.encoder_layers = nn.ModuleList([layer() for _ in range(encoder_depth)])
        self.decoder_layers = nn.ModuleList([layer() for _ in range(decoder_depth)])

        def node_wise(layers):
            return MLP(in_dim=hidden_dim, hidden_size=hidden_dim, out_dim=hidden_dim, mid_batch_norm=batch_norm,
                       last_batch_norm=batch_norm, batch_norm_momentum=batch_norm_momentum, layers=layers,
                       mid_activation=activation, dropout=dropout, last_activation='None')
        # reference :50-64: both options assign the same attribute; the later assignment wins
        self.node_wise_encoder_layers = node_wise_encoder_layers
        if self.node_wise_encoder_layers > 0:
            self.node_wise_output_network = node_wise(node_wise_encoder_layers)
        self.node_wise_output_layers = node_wise_output_layers
        if self.node_wise_output_layers > 0:
            self.node_wise_output_network = node_wise(node_wise_output_layers)
        self.readout_aggregators = readout_aggregators
        self._readout_codes = [ops.AGG[a] for a in readout_aggregators]
        if projection_dim > 0 and not distance_net:
            self.node_projection_net = MLP(in_dim=hidden_dim, hidden_size=32, mid_batch_norm=True, out_dim=projection_dim,
                                           layers=projection_layers)
        else:
            self.node_projection_net = None
        if distance_net:
            self.distance_net = MLP(in_dim=hidden_dim * 2, hidden_size=projection_dim, mid_batch_norm=True, out_dim=1,
                                    layers=projection_layers)
        else:
            self.distance_net = None

    def forward(self, graph, pairwise_indices):
        g = as_batched_graph(graph)
        pidx = pair_index(pairwise_indices, g)
        side = None
        if self.training and torch.is_grad_enabled() and g.device.type == 'cuda':
            side = streams.side_stream_for(getattr(g, 'ready_event', None), g.device)
        if side is None:
            with bn_counter_scope():
                return tape.run_model(self, lambda: self._forward(g, pidx))
        # next to the 2D network on a side stream, as Net3D.forward; the caller's stream waits before anything is handed back
        main = torch.cuda.current_stream(g.device)
        with torch.cuda.stream(side):
            with bn_counter_scope():
                latent, dist = tape.run_model(self, lambda: self._forward(g, pidx))
        for t in (latent, dist, g.ndata.get('feat'), g.edata.get('d')):
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(main)
        main.wait_stream(side)
        return latent, dist

    def _forward(self, g, pidx):
        idx = g.index()
        if self.use_node_features:
            h = self.atom_encoder(g.ndata['feat'])
        else:
            h = tape.apply(_BroadcastRowFn, self.node_embedding, g.number_of_nodes())
        d = g.edata['d']
        with torch.no_grad():
            d = ops.gather_rows(d.reshape(-1, 1).contiguous().float(), idx.perm)
            if self.fourier_encodings > 0:
                d = ops.fourier_encode(d.view(-1), self.fourier_encodings)
        d = self.edge_input(d, post_act='silu')                                  # reference :134-135
        n_layers = len(self.encoder_layers) + len(self.decoder_layers)
        done = 0
        for mp_layer in self.encoder_layers:
            done += 1
            h, d = mp_layer.step(h, d, idx, need_edge_update=done < n_layers)    # the last layer's edge update is dead
        if self.node_wise_encoder_layers > 0:
            h = self.node_wise_output_network(h)
        latent = tape.apply(ReadoutFn, h, idx, self._readout_codes)              # reference :95-96
        for mp_layer in self.decoder_layers:
            done += 1
            h, d = mp_layer.step(h, d, idx, need_edge_update=done < n_layers)
        if self.node_projection_net is not None and self.distance_net is None:
            h = self.node_projection_net(h)
        g.ndata['feat'] = h
        g.edata['d'] = ops.gather_rows(d.detach().contiguous(), idx.inv_perm)    # side effect, edge-id order
        return latent, self._pair_head(h, pidx)

    def fused_head_refusal(self):
        """None when the fused two-layer head applies, else the reason (by option name) the composed path is taken"""
        if not FUSED_PAIR_HEAD:
            return 'net3d_ae.FUSED_PAIR_HEAD is off'
        if self.distance_net is None:
            return 'distance_net=False: the head is the norm of the projected difference'
        fcs = self.distance_net.fully_connected
        if len(fcs) != 2:
            return f'projection_layers={len(fcs)}: the fused head is the two-layer distance_net'
        f0, f1 = fcs
        if not ops.pair_mlp_supported(f0.out_dim):
            return f'projection_dim={f0.out_dim} above {ops.PAIR_MLP_MAX_WIDTH}'
        if f0.activation != 'relu' or f0.batch_norm is None or f1.activation is not None or f1.batch_norm is not None or f1.out_dim != 1:
            return 'distance_net is not Linear -> ReLU -> BatchNorm -> Linear(D -> 1)'
        if not (f0.bias and f1.bias):
            return 'distance_net without bias'
        s0, s1 = f0.spec(), f1.spec()
        if s0.dropout > 0.0 or s1.dropout > 0.0:
            return 'dropout inside distance_net'
        if s0.bn.sync_group is not None:
            return 'synchronised BatchNorm statistics in distance_net'
        if s0.bn.momentum is None:
            return 'BatchNorm momentum None (cumulative average) in distance_net'
        return None

    def _pair_head(self, h, pidx):
        if self.distance_net is None:
            return tape.apply(_PairNormFn, h, pidx)
        fcs = self.distance_net.fully_connected
        if len(fcs) == 1:
            W, b = fcs[0].hot()[:2]
            return tape.apply(_PairSumHeadFn, h, W, b, pidx)
        if self.fused_head_refusal() is None:
            W1, b1, gamma, beta, spec = fcs[0].hot()[:5]
            W2, b2 = fcs[1].hot()[:2]
            return tape.apply(_PairMLPHeadFn, h, W1, b1, gamma, beta, W2, b2, pidx, spec.bn)
        # the reference's two calls on the [P, 2H] concatenations, two sets of statistics
        y1 = self.distance_net(tape.apply(_PairConcatFn, h, pidx, False))
        y2 = self.distance_net(tape.apply(_PairConcatFn, h, pidx, True))
        return tape.apply(_SoftplusSumToPairsFn, y1, y2, pidx)
