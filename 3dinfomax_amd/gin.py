"""GIN with edge features and an optional virtual node - drop-in for reference models/gin.py (OGBGNN, the 2D baseline of
configs/26.yml .. 30.yml and gin_ogb_2.yml).

Same class names, constructor kwargs (unknown ones swallowed), sub-module names and hence state_dict keys: reference checkpoints load
strict.  `nn.Sequential`, `nn.Linear`, `nn.BatchNorm1d` and `nn.Embedding` are PARAMETER CONTAINERS only; their forward is never called.

Per layer (reference models/gin.py:274-305):
  * the message step - the virtual-node add, the bond embedding, copy_u, ReLU, the sum over the in-edges and (1 + eps) x - is ONE
    kernel per direction (csrc/gin.hip).  Bond features take prod(dims) = 60 joint values, so the bond embedding of an edge is a row of
    the [60, H] table of all combinations, built on the tape by the encoder's own EmbeddingSumFn (whose backward sends the table's
    gradient to the three embedding matrices); no [E, H] tensor exists in either direction;
  * mlp.0 -> mlp.1 -> ReLU is one fused Linear + BatchNorm block (layers.FCFn), mlp.3 -> batch_norms[l] -> ReLU (not on the last
    layer) -> + residual a second one;
  * the virtual-node MLP is two such blocks over the [B, H] rows of the per-graph sums.

Two quirks of the reference are kept: GNN_node_Virtualnode builds its convolutions with BatchNorm momentum 0.1 whatever
`batch_norm_momentum` says (models/gin.py:250), and the virtual-node embedding starts at 0 (:238).

FUSED_CONV = False takes the composed path on the older kernels (per-edge EmbeddingSumFn, gather_rows, add, act, segment_sum): the
in-tree cross-check, and what bond features with more than 256 combinations or of another dtype than int64 take.
"""
import torch
from torch import nn

from . import ops, tape
from .graph import as_batched_graph
from .layers import BNSpec, FCFn, FCSpec, ReadoutFn, bn_counter_scope, dropout as _dropout
from .mol_encoder import AtomEncoder, BondEncoder
from .net3d import SegmentReduceFn, _AddFn
from .pna_original import _GatherSrcFn

# False: the message step composed of the older kernels, [E, H] tensors materialised (cross-check)
FUSED_CONV = True
MAX_CODES = 256

_LINEAR = FCSpec(None, None)


def _bn_spec(bn, training, post_act):
    return FCSpec(None, BNSpec(bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps, training), post_act)


class _EdgeCodes:
    """what every layer of one forward shares: the kernel index, the joint bond code of every edge (destination-sorted order), the
    code-sorted edge list and the node -> graph map"""
    __slots__ = ('index', 'bond_idx', 'fused', 'num_codes', 'comb', 'codes', 'code_order', 'code_ptr', 'node_graph')


def _combinations(dims, device):
    """[prod(dims), C] int64: row v holds the categories with joint code v (first column fastest, ops.edge_codes)"""
    n = 1
    for d in dims:
        n *= d
    v = torch.arange(n, dtype=torch.int64)
    cols, stride = [], 1
    for d in dims:
        cols.append((v // stride) % d)
        stride *= d
    return torch.stack(cols, 1).contiguous().to(device)


def edge_context(g, dims):
    """the _EdgeCodes of a batch, cached on the graph object (a resident batch is sorted once)"""
    bond_idx = g.edata['feat']
    ent = g.__dict__.get('_gin_edge_codes')
    if ent is not None and ent.bond_idx is bond_idx and ent.fused == FUSED_CONV:
        return ent
    idx = g.index()
    c = _EdgeCodes()
    c.index, c.bond_idx = idx, bond_idx
    n_comb = 1
    for d in dims:
        n_comb *= d
    c.num_codes = n_comb
    c.fused = FUSED_CONV
    fused = FUSED_CONV and n_comb <= MAX_CODES and bond_idx.dtype == torch.int64
    c.comb = c.codes = c.code_order = c.code_ptr = None
    if fused:
        c.comb = _combinations(dims, bond_idx.device)
        if idx.num_edges > 0:
            c.codes, _ = ops.edge_codes(bond_idx.contiguous(), idx.perm, dims, (n_comb + 31) // 32 * 32)
        else:
            c.codes = torch.empty(0, dtype=torch.int32, device=bond_idx.device)
        c.code_order, c.code_ptr = ops.code_sorted_index(c.codes, n_comb)
    bnn = g.batch_num_nodes().to(idx.graph_ptr.device)
    c.node_graph = torch.repeat_interleave(torch.arange(bnn.shape[0], device=bnn.device), bnn).to(torch.int32)
    g.__dict__['_gin_edge_codes'] = c
    return c


class _GINInputFn(torch.autograd.Function):
    """x = h + vn[graph of the node] - written by the launch that also computes z (csrc/gin.hip: i3d_gin_conv_fwd); z waits in
    `holder` for _GINConvFn, which owns the gradients of T and eps.  backward: dh = dx, dvn = per-graph sums of dx."""

    @staticmethod
    def forward(ctx, h, vn, T, eps, ec, holder):
        idx = ec.index
        x, z = ops.gin_conv_fwd(h.contiguous(), vn.contiguous(), idx.graph_ptr, idx.num_graphs, T.contiguous(), ec.codes, idx.in_ptr,
                                idx.src_s, eps)
        holder['z'] = z
        ctx.index = idx
        return x

    @staticmethod
    def backward(ctx, gx):
        idx = ctx.index
        gx = gx.contiguous()
        return gx, ops.segment_sum(gx, idx.graph_ptr, None, idx.num_graphs), None, None, None, None


class _GINConvFn(torch.autograd.Function):
    """z = (1 + eps) x + sum over the in-edges of relu(x[src] + T[code]) (csrc/gin.hip); backward: dx, dT, deps with the ReLU gate
    recomputed.  `holder`: z already computed by _GINInputFn's launch."""

    @staticmethod
    def forward(ctx, x, T, eps, ec, holder):
        x, T = x.contiguous(), T.contiguous()
        if holder is None:
            idx = ec.index
            _, z = ops.gin_conv_fwd(x, None, None, 0, T, ec.codes, idx.in_ptr, idx.src_s, eps)
        else:
            z = holder.pop('z')
        ctx.ec = ec
        ctx.save_for_backward(x, T, eps)
        return z

    @staticmethod
    def backward(ctx, g):
        x, T, eps = ctx.saved_tensors
        ec = ctx.ec
        idx = ec.index
        dx, dT, deps = ops.gin_conv_bwd(g.contiguous(), x, T, ec.codes, idx.src_s, idx.dst_s, idx.out_ptr, idx.out_epos, ec.code_order,
                                        ec.code_ptr, eps, dT_out=None)
        return dx, dT, deps, None, None


# ---- the composed path (FUSED_CONV = False): the same arithmetic on the older kernels --------------------------------------------
class _GatherGraphRowsFn(torch.autograd.Function):
    """vn[graph of the node]; backward = per-graph sums"""

    @staticmethod
    def forward(ctx, vn, ec):
        ctx.index = ec.index
        return ops.gather_rows(vn.contiguous(), ec.node_graph)

    @staticmethod
    def backward(ctx, g):
        idx = ctx.index
        return ops.segment_sum(g.contiguous(), idx.graph_ptr, None, idx.num_graphs), None


class _ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m):
        m = m.contiguous()
        ctx.save_for_backward(m)
        return ops.act_fwd(m, 'relu')

    @staticmethod
    def backward(ctx, g):
        (m,) = ctx.saved_tensors
        return ops.act_bwd(g.contiguous(), m, 'relu')


class _EpsCombineFn(torch.autograd.Function):
    """(1 + eps) x + agg (agg None: no edges)"""

    @staticmethod
    def forward(ctx, x, agg, eps):
        x = x.contiguous()
        coef = (1 + eps.detach()).expand(x.shape[0]).contiguous()
        ctx.save_for_backward(x, coef)
        out = ops.row_scale(x, coef)
        return ops.add_inplace(out, agg.contiguous()) if agg is not None else out

    @staticmethod
    def backward(ctx, g):
        x, coef = ctx.saved_tensors
        g = g.contiguous()
        deps = ops.colsum(ops.mul(g, x)).sum().reshape(1)
        return ops.row_scale(g, coef), g, deps


class _GraphSumFn(torch.autograd.Function):
    """dgl SumPooling: per-graph sums of the node rows (ops.segment_sum over graph_ptr); backward = broadcast"""

    @staticmethod
    def forward(ctx, x, ec):
        ctx.ec = ec
        idx = ec.index
        return ops.segment_sum(x.contiguous(), idx.graph_ptr, None, idx.num_graphs)

    @staticmethod
    def backward(ctx, g):
        ec = ctx.ec
        return ops.segment_bcast(g.contiguous(), ec.index.graph_ptr, ec.node_graph, ec.index.num_nodes), None


class _BroadcastEmbeddingFn(torch.autograd.Function):
    """virtualnode_embedding(zeros(B)): the one row [1, H] for every graph; backward = column sum"""

    @staticmethod
    def forward(ctx, weight, n):
        return ops.broadcast_row(weight.contiguous().view(-1), n)

    @staticmethod
    def backward(ctx, g):
        return ops.colsum(g.contiguous()).view(1, -1), None


# ---- modules ------------------------------------------------------------------------------------------------------------------
class GINConv(nn.Module):
    """reference models/gin.py:85-110"""

    def __init__(self, hidden_dim, batch_norm_momentum=0.1):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.BatchNorm1d(hidden_dim, momentum=batch_norm_momentum),
                                 nn.ReLU(), nn.Linear(hidden_dim, hidden_dim))
        self.eps = nn.Parameter(torch.Tensor([0]))
        self.bond_encoder = BondEncoder(emb_dim=hidden_dim)

    def message(self, ec, h, vn=None):
        """-> (x, z): x = h + vn[graph] (h itself without a virtual node), z = (1 + eps) x + sum of relu(x[src] + bond_emb)"""
        idx = ec.index
        if ec.codes is not None:
            T = self.bond_encoder(ec.comb)                       # [V, H], on the tape: its gradient goes back through EmbeddingSumFn
            if vn is None:
                return h, tape.apply(_GINConvFn, h, T, self.eps, ec, None)
            holder = {}
            x = tape.apply(_GINInputFn, h, vn, T, self.eps, ec, holder)
            return x, tape.apply(_GINConvFn, x, T, self.eps, ec, holder)
        x = h if vn is None else tape.apply(_AddFn, h, tape.apply(_GatherGraphRowsFn, vn, ec))
        agg = None
        if idx.num_edges > 0:
            emb = self.bond_encoder(ec.bond_idx.long(), perm=idx.perm)           # [E, H], destination-sorted order
            m = tape.apply(_ReluFn, tape.apply(_AddFn, tape.apply(_GatherSrcFn, x, idx), emb))
            agg = tape.apply(SegmentReduceFn, m, idx, False)
        return x, tape.apply(_EpsCombineFn, x, agg, self.eps)

    def hidden(self, z):
        """mlp.0 -> mlp.1 -> ReLU"""
        lin, bn = self.mlp[0], self.mlp[1]
        return tape.apply(FCFn, z, lin.weight, lin.bias, bn.weight, bn.bias, None, _bn_spec(bn, self.training, 'relu'))

    def forward(self, g, x, edge_attr=None):
        g = as_batched_graph(g)
        ec = edge_context(g, self.bond_encoder.dims)
        _, z = self.message(ec, x)
        lin = self.mlp[3]
        return tape.apply(FCFn, self.hidden(z), lin.weight, lin.bias, None, None, None, _LINEAR)


def _check_gnn_type(gnn_type):
    if gnn_type == 'gcn':
        raise NotImplementedError("gnn_type='gcn': the GCN convolution of the reference has no HIP kernel; use gnn_type='gin'")
    if gnn_type != 'gin':
        raise ValueError(f'Undefined GNN type called {gnn_type}')


def _check_jk(JK):
    if JK not in ('last', 'sum'):
        raise ValueError(f"JK={JK!r}: 'last' or 'sum'")


class _NodeGNNBase(nn.Module):
    def _layer(self, ec, layer, h, vn):
        """-> (x, h_next): the message step, the two fused Linear + BatchNorm blocks, dropout, residual"""
        conv, bn = self.convs[layer], self.batch_norms[layer]
        x, z = conv.message(ec, h, vn)
        t = conv.hidden(z)
        lin = conv.mlp[3]
        last = layer == self.num_layers - 1
        drop = self.dropout if self.training else 0
        spec = _bn_spec(bn, self.training, None if last else 'relu')
        if drop:      # reference :281-288: dropout sits between the activation and the residual add
            y = _dropout(tape.apply(FCFn, t, lin.weight, lin.bias, bn.weight, bn.bias, None, spec), drop, True)
            return x, (tape.apply(_AddFn, y, x) if self.residual else y)
        return x, tape.apply(FCFn, t, lin.weight, lin.bias, bn.weight, bn.bias, x if self.residual else None, spec)

    def _jk(self, h_list):
        if self.JK == 'last':
            return h_list[-1]
        rep = h_list[0]           # reference :205-208, :310-313: range(num_layers) - the last layer's output is NOT in the sum
        for layer in range(1, self.num_layers):
            rep = tape.apply(_AddFn, rep, h_list[layer])
        return rep


class GNN_node(_NodeGNNBase):
    """reference models/gin.py:146-210"""

    def __init__(self, num_layers, hidden_dim, dropout=0.5, JK='last', residual=False, gnn_type='gin', batch_norm_momentum=0.1):
        super().__init__()
        _check_gnn_type(gnn_type)
        _check_jk(JK)
        if num_layers < 2:
            raise ValueError('Number of GNN layers must be greater than 1.')
        self.num_layers, self.dropout, self.JK, self.residual = num_layers, dropout, JK, residual
        self.atom_encoder = AtomEncoder(hidden_dim)
        self.convs = nn.ModuleList(GINConv(hidden_dim, batch_norm_momentum) for _ in range(num_layers))
        self.batch_norms = nn.ModuleList(nn.BatchNorm1d(hidden_dim, momentum=batch_norm_momentum) for _ in range(num_layers))

    def forward(self, g, x, edge_attr=None):
        g = as_batched_graph(g)
        ec = edge_context(g, self.convs[0].bond_encoder.dims)
        h_list = [self.atom_encoder(x)]
        for layer in range(self.num_layers):
            _, h = self._layer(ec, layer, h_list[layer], None)
            h_list.append(h)
        return self._jk(h_list)


class GNN_node_Virtualnode(_NodeGNNBase):
    """reference models/gin.py:214-315"""

    def __init__(self, num_layers, hidden_dim, dropout=0.5, JK='last', residual=False, gnn_type='gin', batch_norm_momentum=0.1):
        super().__init__()
        _check_gnn_type(gnn_type)
        _check_jk(JK)
        if num_layers < 2:
            raise ValueError('Number of GNN layers must be greater than 1.')
        self.num_layers, self.dropout, self.JK, self.residual = num_layers, dropout, JK, residual
        self.atom_encoder = AtomEncoder(hidden_dim)
        self.virtualnode_embedding = nn.Embedding(1, hidden_dim)
        nn.init.constant_(self.virtualnode_embedding.weight.data, 0)
        # reference :250: GINConv(hidden_dim) - the convolutions' BatchNorm keeps momentum 0.1 whatever batch_norm_momentum says
        self.convs = nn.ModuleList(GINConv(hidden_dim) for _ in range(num_layers))
        self.batch_norms = nn.ModuleList(nn.BatchNorm1d(hidden_dim, momentum=batch_norm_momentum) for _ in range(num_layers))
        self.mlp_virtualnode_list = nn.ModuleList(
            nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.BatchNorm1d(hidden_dim, momentum=batch_norm_momentum), nn.ReLU(),
                          nn.Linear(hidden_dim, hidden_dim), nn.BatchNorm1d(hidden_dim, momentum=batch_norm_momentum), nn.ReLU())
            for _ in range(num_layers - 1))

    def forward(self, g, x, edge_attr=None):
        g = as_batched_graph(g)
        ec = edge_context(g, self.convs[0].bond_encoder.dims)
        vn = tape.apply(_BroadcastEmbeddingFn, self.virtualnode_embedding.weight, ec.index.num_graphs)
        h_list = [self.atom_encoder(x)]
        drop = self.dropout if self.training else 0
        for layer in range(self.num_layers):
            h_list[layer], h = self._layer(ec, layer, h_list[layer], vn)
            h_list.append(h)
            if layer < self.num_layers - 1:
                t = tape.apply(_AddFn, tape.apply(_GraphSumFn, h_list[layer], ec), vn)
                mlp = self.mlp_virtualnode_list[layer]
                for lin, bn in ((mlp[0], mlp[1]), (mlp[3], mlp[4])):
                    t = tape.apply(FCFn, t, lin.weight, lin.bias, bn.weight, bn.bias, None, _bn_spec(bn, self.training, 'relu'))
                t = _dropout(t, drop, True) if drop else t
                vn = tape.apply(_AddFn, vn, t) if self.residual else t
        return self._jk(h_list)


class OGBGNN(nn.Module):
    """reference models/gin.py:17-81.  forward(g) -> [B, target_dim]; g: BatchedMolGraph or a DGL graph with the integer atom /
    bond features in ndata['feat'] / edata['feat']."""

    def __init__(self, target_dim=1, num_layers=5, hidden_dim=300, gnn_type='gin', virtual_node=True, residual=False, dropout=0,
                 JK='last', graph_pooling='sum', batch_norm_momentum=0.1, **kwargs):
        super().__init__()
        _check_gnn_type(gnn_type)
        if graph_pooling == 'max':
            raise NotImplementedError("graph_pooling='max': not offered (the reference assigns the MaxPooling class without "
                                      'instantiating it, models/gin.py:55, and fails at its first call)')
        if graph_pooling in ('attention', 'set2set'):
            raise NotImplementedError(f'graph_pooling={graph_pooling!r}: no HIP kernel; sum or mean')
        if graph_pooling not in ('sum', 'mean'):
            raise ValueError('Invalid graph pooling type.')
        if num_layers < 2:
            raise ValueError('Number of GNN layers must be greater than 1.')
        self.num_layers, self.dropout, self.JK = num_layers, dropout, JK
        self.hidden_dim, self.target_dim, self.graph_pooling = hidden_dim, target_dim, graph_pooling
        cls = GNN_node_Virtualnode if virtual_node else GNN_node
        self.node_gnn = cls(num_layers, hidden_dim, JK=JK, dropout=dropout, residual=residual, gnn_type=gnn_type,
                            batch_norm_momentum=batch_norm_momentum)
        self._readout_codes = ops.agg_codes([graph_pooling])
        self.graph_pred_linear = nn.Linear(hidden_dim, target_dim)

    def forward(self, g):
        g = as_batched_graph(g)
        with bn_counter_scope():
            return tape.run_model(self, lambda: self._forward(g))

    def _forward(self, g):
        h_node = self.node_gnn(g, g.ndata['feat'], g.edata['feat'])
        h_graph = tape.apply(ReadoutFn, h_node, g.index(), self._readout_codes)
        lin = self.graph_pred_linear
        return tape.apply(FCFn, h_graph, lin.weight, lin.bias, None, None, None, _LINEAR)
