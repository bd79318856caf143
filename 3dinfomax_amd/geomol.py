"""GeoMol's message-passing network on OGB features - drop-in for reference models/geomol_mpnn_ogb_feat.py and the classes of
models/geomol_mpnn.py it is built from (`model_type: 'GeomolGNNWrapperOGBFeat'` of configs/geomolgnn_wrapper_ogb_feat.yml and the
tune_from_ot_* configs).

Same class names, constructor kwargs (unknown ones swallowed), sub-module and parameter names: a reference checkpoint loads strict.
`nn.Linear`, `nn.ReLU`, `nn.ModuleList` are PARAMETER CONTAINERS only; their forward is never called.

    x = node_init(AtomEncoder(z))            e = edge_init(BondEncoder(edge_attr))
    repeat depth times, the SAME weights (`update`):
        h = relu(edge(e) + node_in(x)[src] + node_out(x)[dst])
        e = (1 + edge_eps) e + mlp(h)
        x = (1 + node_eps) x + node_mlp_2( sum over the in-edges of node_mlp_1(e) )
    out = MLP_readout( per-graph mean of x )

Inside the network every edge tensor is in destination-sorted order (graph.GraphIndex.perm); the modules below take the GraphIndex
where the reference takes `edge_index`.  Per step (FUSED_STEP, csrc/geomol.hip):
  * node_in | node_out are ONE [N, 2H] product, their weight gradients one product; edge(e) one [E, H] product;
  * the three-way gather-add-ReLU is one launch, its backward - the gated gradient, its sum over the out-edges of every node and its
    sum over the in-edges - one launch as well;
  * both residuals `(1 + eps) a + b` are one launch, eps read on the device; deps is accumulated in fp64;
  * the last layer of node_mlp_1 is linear, so sum_in (u W^T + b) = (sum_in u) W^T + indeg b: the hidden activation u is summed
    over the in-edges and the last Linear runs on N rows instead of E.

FUSED_STEP = False composes the step from the older kernels (edge_combine_fwd, act_fwd / act_bwd, segment_sum, row_scale, add,
colsum) with node_mlp_1's last Linear on the E edge rows, the reference's way: the in-tree cross-check.

Kept quirks of the reference: GeomolMLP's hidden width is in_dim when out_dim < 10, else out_dim; node_init / edge_init always have
num_layers = 2 whatever n_layers says; `batch_norm_momentum` is accepted and unused inside the network (no normalisation on this
path); edge_eps / node_eps belong to `update`, of which there is one whatever `depth` is; the readout keeps momentum 0.1.

A batch without any edge leaves the edge model out of the step (the aggregate is a zero row for every node): its parameters get no
gradient where the reference would give zeros.
"""
import torch
from torch import nn

from . import ops, tape
from .gin import _EpsCombineFn, _ReluFn
from .graph import BatchedMolGraph, as_batched_graph
from .layers import MLP, FCFn, FCSpec, ReadoutFn, act_name, bn_counter_scope
from .mol_encoder import AtomEncoder, BondEncoder
from .net3d import SegmentReduceFn

# False: the step composed of the older kernels, node_mlp_1's last Linear on the edge rows (cross-check)
FUSED_STEP = True

_LINEAR = FCSpec(None, None)


def as_geomol_graph(data):
    """BatchedMolGraph of a batch: a BatchedMolGraph / DGL-like graph as it is (graph.as_batched_graph), a PyG-style object with
    `z` [N, 9], `edge_index` [2, E], `edge_attr` [E, 3] and a non-decreasing `batch` [N] converted once (cached on the object)."""
    if isinstance(data, BatchedMolGraph) or not (hasattr(data, 'edge_index') and hasattr(data, 'z')):
        return as_batched_graph(data)
    cached = getattr(data, '_amd_batched', None)
    if cached is not None:
        return cached
    z, edge_index, batch = data.z, data.edge_index, data.batch
    n = int(z.shape[0])
    if batch.dim() != 1 or batch.shape[0] != n:
        raise ValueError(f'batch has shape {tuple(batch.shape)}; one graph id per node ({n}) expected')
    if n > 1 and bool((batch[1:] < batch[:-1]).any()):
        raise ValueError('batch is not non-decreasing: the nodes of a graph must be contiguous (torch_geometric batching order)')
    if n and int(batch[0]) < 0:
        raise ValueError('batch holds a negative graph id')
    bnn = torch.bincount(batch.long(), minlength=1) if n else torch.zeros(1, dtype=torch.long)
    bg = BatchedMolGraph(edge_index[0], edge_index[1], n, bnn, ndata={'feat': z}, edata={'feat': data.edge_attr})
    try:
        data._amd_batched = bg
    except Exception:
        pass
    return bg


def _indeg(index):
    """float in-degrees [N], once per batch index"""
    d = index.__dict__.get('_indeg_f32')
    if d is None:
        d = index.__dict__['_indeg_f32'] = (index.in_ptr[1:] - index.in_ptr[:-1]).float().contiguous()
    return d


# ---- Functions ------------------------------------------------------------------------------------------------------------------
class _NodeProjFn(torch.autograd.Function):
    """PQ [N, 2H] = x [W_in | W_out]^T as one product; `packed` [2H, H] is the two weights stacked (built once per forward).
    backward: dx = dPQ packed, d[W_in; W_out] = dPQ^T x as one product, handed out as its two halves."""

    @staticmethod
    def forward(ctx, x, w_in, w_out, packed):
        x = x.contiguous()
        ctx.save_for_backward(x, packed)
        return ops.gemm(x, packed, trans_b=True)

    @staticmethod
    def backward(ctx, g):
        x, packed = ctx.saved_tensors
        g = g.contiguous()
        H = x.shape[1]
        gw = ops.gemm(g, x, trans_a=True)
        gx = ops.gemm(g, packed) if ctx.needs_input_grad[0] else None
        return gx, gw[:H], gw[H:], None


class _EdgeGateFn(torch.autograd.Function):
    """h = relu(F + P[src] + Q[dst]), one launch per direction (csrc/geomol.hip)"""

    @staticmethod
    def forward(ctx, F, PQ, index):
        h = ops.geomol_edge_fwd(F.contiguous(), PQ.contiguous(), index.src_s, index.dst_s)
        ctx.index = index
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, g):
        (h,) = ctx.saved_tensors
        idx = ctx.index
        dF, dPQ = ops.geomol_edge_bwd(g.contiguous(), h, idx.in_ptr, idx.out_ptr, idx.out_epos)
        return dF, dPQ, None


class _EdgeCombineFn(torch.autograd.Function):
    """the composed path's pre-activation F + P[src] + Q[dst]; backward: dF is the incoming gradient, dP | dQ two segmented sums"""

    @staticmethod
    def forward(ctx, F, PQ, index):
        ctx.index = index
        return ops.edge_combine_fwd(PQ.contiguous(), F.contiguous(), None, index.src_s, index.dst_s)

    @staticmethod
    def backward(ctx, g):
        idx = ctx.index
        g = g.contiguous()
        H = g.shape[1]
        dPQ = torch.empty(idx.num_nodes, 2 * H, dtype=torch.float32, device=g.device)
        ops.segment_sum(g, idx.out_ptr, idx.out_epos, idx.num_nodes, out=dPQ[:, :H])
        ops.segment_sum(g, idx.in_ptr, None, idx.num_nodes, out=dPQ[:, H:])
        return g, dPQ, None


class _ResidualFn(torch.autograd.Function):
    """(1 + eps) a + b (csrc/geomol.hip); backward: da, deps from one call, db the incoming gradient itself"""

    @staticmethod
    def forward(ctx, a, b, eps):
        a = a.contiguous()
        ctx.save_for_backward(a, eps)
        return ops.geomol_residual_fwd(a, b.contiguous(), eps)

    @staticmethod
    def backward(ctx, g):
        a, eps = ctx.saved_tensors
        g = g.contiguous()
        da, deps = ops.geomol_residual_bwd(g, a, eps)
        return da, g, deps


class _DegLinearFn(torch.autograd.Function):
    """s W^T + indeg b on the node rows: the last Linear of node_mlp_1 after the sum over the in-edges.  backward: ds = g W,
    dW = g^T s, db = sum_v indeg(v) g[v] (the weighted column sum)."""

    @staticmethod
    def forward(ctx, s, W, b, indeg):
        s = s.contiguous()
        ctx.save_for_backward(s, W, indeg)
        out = ops.gemm(s, W, trans_b=True)
        return ops.row_axpy(ops.broadcast_row(b.contiguous(), s.shape[0]), indeg, out)

    @staticmethod
    def backward(ctx, g):
        s, W, indeg = ctx.saved_tensors
        g = g.contiguous()
        gW = ops.gemm(g, s, trans_a=True, out=tape.grad_like(W))
        gb = ops.colsum(g, indeg, out=tape.grad_for_bias_of(W, W.shape[0]))
        return ops.gemm(g, W), gW, gb, None


class _GatherRowsFn(torch.autograd.Function):
    """out[j] = x[idx[j]] for a permutation idx with inverse inv; backward = the gather through inv"""

    @staticmethod
    def forward(ctx, x, idx, inv):
        ctx.inv = inv
        return ops.gather_rows(x.contiguous(), idx)

    @staticmethod
    def backward(ctx, g):
        return ops.gather_rows(g.contiguous(), ctx.inv), None, None


# ---- modules --------------------------------------------------------------------------------------------------------------------
class GeomolMLP(nn.Module):
    """reference models/geomol_mpnn.py:12-45: `layers` = Linear, activation, ..., Linear (keys layers.0, layers.2, ...)"""

    def __init__(self, in_dim, out_dim, num_layers, activation=None, layer_norm=False, batch_norm=False, batch_norm_momentum=0.1):
        super().__init__()
        if layer_norm or batch_norm:
            raise NotImplementedError('GeomolMLP with layer_norm / batch_norm: no configuration of the reference builds one, and '
                                      'there is no HIP path for it')
        activation = nn.ReLU() if activation is None else activation
        self._act = act_name(activation)
        self.layers = nn.ModuleList()
        h_dim = in_dim if out_dim < 10 else out_dim
        for layer in range(num_layers):
            self.layers.append(nn.Linear(in_dim if layer == 0 else h_dim, h_dim))
            self.layers.append(activation)
        self.layers.append(nn.Linear(h_dim, out_dim))

    def _linears(self):
        return [m for m in self.layers if isinstance(m, nn.Linear)]

    @property
    def last(self):
        return self.layers[len(self.layers) - 1]

    def hidden(self, x):
        """everything in front of the last Linear"""
        spec = FCSpec(self._act, None)
        for lin in self._linears()[:-1]:
            x = tape.apply(FCFn, x, lin.weight, lin.bias, None, None, None, spec)
        return x

    def forward(self, x):
        lin = self.last
        return tape.apply(FCFn, self.hidden(x), lin.weight, lin.bias, None, None, None, _LINEAR)


class EdgeModel(nn.Module):
    """reference models/geomol_mpnn.py:79-99.  forward(x, edge_attr, index): index the GraphIndex of the batch, edge_attr [E, H] in
    its destination-sorted order."""

    def __init__(self, hidden_dim, n_layers, batch_norm_momentum=0.1):
        super().__init__()
        self.edge = nn.Linear(hidden_dim, hidden_dim)
        self.node_in = nn.Linear(hidden_dim, hidden_dim, bias=False)
        self.node_out = nn.Linear(hidden_dim, hidden_dim, bias=False)
        self.mlp = GeomolMLP(hidden_dim, hidden_dim, n_layers, batch_norm_momentum=batch_norm_momentum)

    def packed_node_weight(self):
        """[2H, H]: node_in.weight over node_out.weight (data only: the gradient goes to the two parameters)"""
        return torch.cat([self.node_in.weight.detach(), self.node_out.weight.detach()], 0)

    def forward(self, x, edge_attr, index, packed=None):
        packed = self.packed_node_weight() if packed is None else packed
        PQ = tape.apply(_NodeProjFn, x, self.node_in.weight, self.node_out.weight, packed)
        F = tape.apply(FCFn, edge_attr, self.edge.weight, self.edge.bias, None, None, None, _LINEAR)
        if FUSED_STEP:
            h = tape.apply(_EdgeGateFn, F, PQ, index)
        else:
            h = tape.apply(_ReluFn, tape.apply(_EdgeCombineFn, F, PQ, index))
        return self.mlp(h)


class GeomolNodeModel(nn.Module):
    """reference models/geomol_mpnn.py:102-118.  forward(x, index, edge_attr, batch): as EdgeModel; `batch` is unused, as there."""

    def __init__(self, hidden_dim, n_layers, batch_norm_momentum=0.1):
        super().__init__()
        self.node_mlp_1 = GeomolMLP(hidden_dim, hidden_dim, n_layers, batch_norm_momentum=batch_norm_momentum)
        self.node_mlp_2 = GeomolMLP(hidden_dim, hidden_dim, n_layers, batch_norm_momentum=batch_norm_momentum)

    def forward(self, x, index, edge_attr, batch=None):
        if FUSED_STEP:
            lin = self.node_mlp_1.last
            s = tape.apply(SegmentReduceFn, self.node_mlp_1.hidden(edge_attr), index, False)
            agg = tape.apply(_DegLinearFn, s, lin.weight, lin.bias, _indeg(index))
        else:
            agg = tape.apply(SegmentReduceFn, self.node_mlp_1(edge_attr), index, False)
        return self.node_mlp_2(agg)


class GeomolMetaLayer(nn.Module):
    """reference models/geomol_mpnn.py:48-76.  forward(x, index, edge_attr) -> (x, edge_attr), both residuals with their own eps."""

    def __init__(self, edge_model=None, node_model=None):
        super().__init__()
        self.edge_model = edge_model
        self.node_model = node_model
        self.edge_eps = nn.Parameter(torch.Tensor([0]))
        self.node_eps = nn.Parameter(torch.Tensor([0]))
        self.reset_parameters()

    def reset_parameters(self):
        for item in [self.node_model, self.edge_model]:
            if hasattr(item, 'reset_parameters'):
                item.reset_parameters()

    @staticmethod
    def _residual(a, b, eps):
        return tape.apply(_ResidualFn if FUSED_STEP else _EpsCombineFn, a, b, eps)

    def forward(self, x, index, edge_attr=None, batch=None, packed=None):
        if index.num_edges == 0:           # no edge anywhere in the batch: every aggregate is a zero row
            if self.node_model is not None:
                zero = torch.zeros_like(x)
                x = self._residual(x, self.node_model.node_mlp_2(zero), self.node_eps)
            return x, edge_attr
        if self.edge_model is not None:
            edge_attr = self._residual(edge_attr, self.edge_model(x, edge_attr, index, packed), self.edge_eps)
        if self.node_model is not None:
            x = self._residual(x, self.node_model(x, index, edge_attr, batch), self.node_eps)
        return x, edge_attr


class GeomolGNNOGBFeat(nn.Module):
    """reference models/geomol_mpnn_ogb_feat.py:14-36.  forward(g, x, edge_attr) -> (x [N, H], e [E, H]): g the batch (anything
    as_geomol_graph takes), x / edge_attr the integer atom / bond features in the caller's order; e comes back in the caller's edge
    order."""

    def __init__(self, hidden_dim=300, depth=3, n_layers=2, batch_norm_momentum=0.1, **kwargs):
        super().__init__()
        self.depth = depth
        self.hidden_dim = hidden_dim
        self.bond_encoder = BondEncoder(hidden_dim)
        self.atom_encoder = AtomEncoder(hidden_dim)
        self.node_init = GeomolMLP(hidden_dim, hidden_dim, num_layers=2, batch_norm_momentum=batch_norm_momentum)
        self.edge_init = GeomolMLP(hidden_dim, hidden_dim, num_layers=2, batch_norm_momentum=batch_norm_momentum)
        self.update = GeomolMetaLayer(EdgeModel(hidden_dim, n_layers, batch_norm_momentum=batch_norm_momentum),
                                      GeomolNodeModel(hidden_dim, n_layers, batch_norm_momentum=batch_norm_momentum))

    def forward(self, g, x, edge_attr, **kwargs):
        idx = as_geomol_graph(g).index()
        x = self.node_init(self.atom_encoder(x))
        if idx.num_edges > 0:
            e = self.edge_init(self.bond_encoder(edge_attr.long(), perm=idx.perm))          # destination-sorted order from here on
        else:
            e = torch.empty(0, self.hidden_dim, dtype=torch.float32, device=x.device)
        packed = self.update.edge_model.packed_node_weight()
        for _ in range(self.depth):
            x, e = self.update(x, idx, e, packed=packed)
        if idx.num_edges > 0:
            e = tape.apply(_GatherRowsFn, e, idx.inv_perm, idx.perm)
        return x, e


class GeomolGNNWrapperOGBFeat(nn.Module):
    """reference models/geomol_mpnn_ogb_feat.py:39-55.  forward(g) -> [B, target_dim]; g: a BatchedMolGraph or DGL graph with the
    integer atom / bond features in ndata['feat'] / edata['feat'], or a PyG-style object (z, edge_index, edge_attr, batch)."""

    def __init__(self, hidden_dim, target_dim, readout_hidden_dim=None, readout_layers=2, readout_batchnorm=True, **kwargs):
        super().__init__()
        if readout_hidden_dim is None:
            readout_hidden_dim = hidden_dim
        self.node_gnn = GeomolGNNOGBFeat(hidden_dim=hidden_dim, **kwargs)
        self._readout_codes = ops.agg_codes(['mean'])
        self.output = MLP(in_dim=hidden_dim, hidden_size=readout_hidden_dim, mid_batch_norm=readout_batchnorm, out_dim=target_dim,
                          layers=readout_layers, batch_norm_momentum=0.1)

    def forward(self, data):
        g = as_geomol_graph(data)
        with bn_counter_scope():
            return tape.run_model(self, lambda: self._forward(g))

    def _forward(self, g):
        x, _ = self.node_gnn(g, g.ndata['feat'], g.edata['feat'])
        pooled = tape.apply(ReadoutFn, x, g.index(), self._readout_codes)
        return self.output(pooled)
