"""EGNN (the E(n)-style 3D encoder of reference models/egnn.py; `model3d_type: 'EGNN'` of configs/0.yml) on the MI355X kernels.

Same constructor kwargs (unknown ones swallowed), sub-module / parameter names (`input`, `mp_layers.{l}.message_network |
update_network | soft_edge_network`, `node_wise_output_network`, `output`) and side effect (`ndata['feat']` overwritten with the final
node features): a reference checkpoint loads strict.

Per layer (reference models/egnn.py:124-140):
  * message_network on [h_src | h_dst | |x_src - x_dst|^2] is the node-level P trick of layers.EdgeFCFn plus fused Linear + BatchNorm
    blocks; the squared distances [E, 1] are computed once per forward (csrc/pack.hip: i3d_edge_sqdist) - coordinates are data;
  * the soft-edge gate, the sum / mean over the in-edges and `m_sum + feat` are ONE kernel per direction (csrc/egnn.hip): the gated
    message never exists as an [E, H] tensor;
  * update_network with the residual `+ feat` folded into its last block.

EGCLayer.fused_gate_reduce = False composes the middle step from the 3D network's Functions (SoftEdgeFn, SegmentReduceFn, _AddFn):
the in-tree cross-check, and what a width outside the kernel's range (H % 4 != 0 or H > 512) takes by itself.

The reference's train.py builds every 3D model with node_dim=0 (train.py: `node_dim=0` for model3d), which gives EGNN's `input` a
Linear with no input columns and fails in the reference's own forward; here node_dim must be the width of ndata['feat'].
"""
from typing import List

import torch
import torch.nn as nn

from . import ops, tape
from .graph import as_batched_graph
from .layers import MLP, ReadoutFn, act_name, bn_counter_scope
from .net3d import SegmentReduceFn, SoftEdgeFn, _AddFn

_READOUTS = ('sum', 'mean', 'max', 'min')


def _coordinates(g):
    x = g.ndata['x'] if 'x' in g.ndata else None
    if x is None or x.dim() != 2 or x.shape[1] != 3 or x.shape[0] != g.number_of_nodes():
        raise ValueError("EGNN needs the atom coordinates in ndata['x'] of shape [N, 3] (complete_graph(mol, coordinates=True)); got "
                         + ('nothing' if x is None else str(tuple(x.shape))))
    return x


def edge_sqdist(x, index):
    """[E, 1] squared end-point distances in destination-sorted order (reference models/egnn.py:129); data: no gradient"""
    x = x.contiguous().float()
    out = torch.empty(index.num_edges, 1, dtype=torch.float32, device=x.device)
    ops.check(ops._lib.load().i3d_edge_sqdist(x.data_ptr(), index.src_s.data_ptr(), index.dst_s.data_ptr(), index.num_edges,
                                              out.data_ptr(), 1, 0, 0, ops._stream()), 'i3d_edge_sqdist')
    return out


class GateReduceFn(torch.autograd.Function):
    """u = h + red_j m[j] sigmoid(Linear_{H->1}(m[j])) over the in-edges, red = sum or mean (reference models/egnn.py:132-133, :125,
    :137) - one launch per direction (csrc/egnn.hip).  A shape the kernel does not take runs the composed chain in here."""

    @staticmethod
    def forward(ctx, m, ws, bs, h, index, mean):
        m, h = m.contiguous(), h.contiguous()
        ctx.cfg, ctx.sub = (index, mean), None
        res = ops.gate_reduce_fwd(m, ws.contiguous(), bs.contiguous(), index.in_ptr, h, mean)
        if res is None:
            gate, red = tape.SubCtx(), tape.SubCtx()
            m_sum = SegmentReduceFn.forward(red, SoftEdgeFn.forward(gate, m, ws, bs), index, mean)
            ctx.sub = (gate, red)
            return ops.add(m_sum, h)
        u, w = res
        ctx.save_for_backward(m, w, ws)
        return u

    @staticmethod
    def backward(ctx, gu):
        gu = gu.contiguous()
        if ctx.sub is not None:
            gate, red = ctx.sub
            gm, gws, gbs = SoftEdgeFn.backward(gate, SegmentReduceFn.backward(red, gu)[0])
            return gm, gws, gbs, gu, None, None
        m, w, ws = ctx.saved_tensors
        index, mean = ctx.cfg
        gm, gws, gbs = ops.gate_reduce_bwd(gu, m, w, ws.contiguous(), index.in_ptr, mean)
        return gm, gws.view_as(ws), gbs, gu, None, None


class EGCLayer(nn.Module):
    """reference models/egnn.py:88-140."""

    # False: the gate, the reduction and the add composed of the 3D network's kernels, [E, H] tensors materialised (cross-check)
    fused_gate_reduce = True

    def __init__(self, node_dim, reduce_func, edge_dim, hidden_dim, batch_norm, batch_norm_momentum, dropout, mid_activation):
        super().__init__()
        self.message_network = MLP(in_dim=hidden_dim * 2 + edge_dim, hidden_size=hidden_dim, out_dim=hidden_dim,
                                   mid_batch_norm=batch_norm, last_batch_norm=batch_norm,
                                   batch_norm_momentum=batch_norm_momentum, layers=2, mid_activation=mid_activation,
                                   dropout=dropout, last_activation=mid_activation)
        if reduce_func not in ('sum', 'mean'):
            raise ValueError('reduce function not supported (reduce_func): ', reduce_func)
        self.reduce_mean = reduce_func == 'mean'
        self.update_network = MLP(in_dim=hidden_dim, hidden_size=hidden_dim, out_dim=hidden_dim, mid_batch_norm=batch_norm,
                                  last_batch_norm=batch_norm, batch_norm_momentum=batch_norm_momentum, layers=2,
                                  mid_activation=mid_activation, dropout=dropout, last_activation='None')
        self.soft_edge_network = nn.Linear(hidden_dim, 1)
        act_name(mid_activation)

    def step(self, h, sqdist, idx):
        m = self.message_network.forward_edge(h, sqdist, idx)                                       # :129-131
        ws, bs = self.soft_edge_network.weight, self.soft_edge_network.bias
        if self.fused_gate_reduce:
            u = tape.apply(GateReduceFn, m, ws, bs, h, idx, self.reduce_mean)                       # :132-133, :125, :137
        else:
            m_sum = tape.apply(SegmentReduceFn, tape.apply(SoftEdgeFn, m, ws, bs), idx, self.reduce_mean)
            u = tape.apply(_AddFn, m_sum, h)
        return self.update_network(u, residual=h)                                                   # :138-140

    def forward(self, graph):
        g = as_batched_graph(graph)
        idx = g.index()
        g.ndata['feat'] = self.step(g.ndata['feat'], edge_sqdist(_coordinates(g), idx), idx)


class EGNN(nn.Module):
    """reference models/egnn.py:13-85.  forward(g) -> [B, target_dim]; g: BatchedMolGraph or a DGL graph of complete molecular
    graphs with float features [N, node_dim] in ndata['feat'] and coordinates [N, 3] in ndata['x']."""

    def __init__(self, node_dim, edge_dim, hidden_dim, target_dim, readout_aggregators: List[str], batch_norm=False,
                 readout_batchnorm=True, batch_norm_momentum=0.1, reduce_func='sum', dropout=0.0, propagation_depth: int = 4,
                 readout_layers: int = 2, readout_hidden_dim=None, fourier_encodings=0, mid_activation: str = 'SiLU', **kwargs):
        super().__init__()
        if fourier_encodings > 0:
            raise NotImplementedError(f'fourier_encodings={fourier_encodings}: not offered (the reference sizes message_network for '
                                      '2 * fourier_encodings + 1 distance columns but feeds the one squared distance, '
                                      'models/egnn.py:36, :129-130, and fails in its own forward)')
        if node_dim is None or node_dim < 1:
            raise ValueError(f"node_dim={node_dim}: EGNN's input layer needs the width of ndata['feat'] (the reference's train.py "
                             'passes node_dim=0 for 3D models, which fails in the reference as well)')
        unknown = [a for a in readout_aggregators if a not in _READOUTS]
        if unknown or not readout_aggregators:
            raise ValueError(f'readout_aggregators={list(readout_aggregators)}: each of {_READOUTS}')
        self.fourier_encodings = fourier_encodings
        self.node_dim = node_dim
        self.input = MLP(in_dim=node_dim, hidden_size=hidden_dim, out_dim=hidden_dim, mid_batch_norm=batch_norm,
                         last_batch_norm=batch_norm, batch_norm_momentum=batch_norm_momentum, layers=1,
                         mid_activation=mid_activation, dropout=dropout, last_activation='None')
        self.mp_layers = nn.ModuleList()
        for _ in range(propagation_depth):
            self.mp_layers.append(EGCLayer(node_dim, edge_dim=1, hidden_dim=hidden_dim, batch_norm=batch_norm,
                                           batch_norm_momentum=batch_norm_momentum, dropout=dropout, mid_activation=mid_activation,
                                           reduce_func=reduce_func))
        self.node_wise_output_network = MLP(in_dim=hidden_dim, hidden_size=hidden_dim, out_dim=hidden_dim,
                                            mid_batch_norm=batch_norm, last_batch_norm=batch_norm,
                                            batch_norm_momentum=batch_norm_momentum, layers=2, mid_activation=mid_activation,
                                            dropout=dropout, last_activation='None')
        if readout_hidden_dim is None:
            readout_hidden_dim = hidden_dim
        self.readout_aggregators = readout_aggregators
        self._readout_codes = ops.agg_codes(readout_aggregators)
        self.output = MLP(in_dim=hidden_dim * len(self.readout_aggregators), hidden_size=readout_hidden_dim,
                          mid_batch_norm=readout_batchnorm, batch_norm_momentum=batch_norm_momentum, out_dim=target_dim,
                          layers=readout_layers)

    def forward(self, graph, *unused):
        g = as_batched_graph(graph)
        with bn_counter_scope():
            return tape.run_model(self, lambda: self._forward(g))

    def _forward(self, g):
        idx = g.index()
        feat = g.ndata['feat']
        if feat.dim() != 2 or feat.shape[1] != self.node_dim:
            raise ValueError(f"ndata['feat'] has shape {tuple(feat.shape)}; this EGNN was built with node_dim={self.node_dim}")
        with torch.no_grad():
            sqdist = edge_sqdist(_coordinates(g), idx)
        h = self.input(feat.float().contiguous(), post_act='silu')                                  # :81-82
        for mp_layer in self.mp_layers:
            h = mp_layer.step(h, sqdist, idx)
        h = self.node_wise_output_network(h)                                                        # :78-79
        g.ndata['feat'] = h
        readout = tape.apply(ReadoutFn, h, idx, self._readout_codes)                                # :74-75
        return self.output(readout)
