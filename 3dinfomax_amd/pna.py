"""PNA 2D message-passing network on the MI355X kernels - drop-in for reference models/pna.py.

Same class names (`PNA`, `PNAGNN`, `PNALayer`, `PNA_AGGREGATORS`, `PNA_SCALERS`), constructor kwargs
(unknown kwargs swallowed like reference models/pna.py:115), sub-module names and therefore state_dict keys
(SURVEY.md 8b), same side effects on the graph (`ndata['feat']` / `edata['feat']` are overwritten with the
float embeddings, reference models/pna.py:162-163, 213).  The arithmetic is the reference's, re-associated for
the hardware:
  * edge tensors live in destination-sorted order, the gather/concat/first-Linear of pretrans is
    P = h [W_s|W_d]^T at node level + a gather-add per edge (layers.EdgeFCFn);
  * the four aggregators x three scalers are one segmented pass (csrc/aggregate.hip);
  * cat([h, agg]) -> posttrans is two accumulating GEMMs (layers.Concat2FCFn), BN + residual fused.
"""
import math
from typing import Callable, Dict, List, Union

import numpy as np

import torch
from torch import nn

from . import layer_native, ops, pna_native, streams, tape
from .graph import as_batched_graph
from .layers import (MLP, AggregateFn, Concat2FCFn, EdgeFCFn, EdgeTable, FCFn, GroupedConcat2FCFn, ReadoutFn,
                     bn_counter_scope)
from .mol_encoder import AtomEncoder, BondEncoder

EPS = 1e-5

# name tables kept for API compatibility (reference models/pna.py:71-87); values are the kernel codes
PNA_AGGREGATORS = {k: v for k, v in ops.AGG.items()}
PNA_SCALERS = {k: v for k, v in ops.SCALER.items()}


# I3D_EDGE_TABLE=0 materialises the [E, F] bond embeddings and multiplies them by W_q in every layer (reference shape)
EDGE_TABLE = True


def _scaler_coef(scaler_code, D, avg):
    """reference models/pna.py:57-68: np.log in float64, then cast to the fp32 tensor's dtype.  D = 0 (the group of nodes
    without in-edges, graph.group_nodes_by_degree): their aggregate is a zero row (DGL semantics), every coefficient 0."""
    if D == 0:
        return 0.0
    if scaler_code == ops.SCALER['amplification']:
        return float(np.float32(math.log(D + 1) / avg))
    if scaler_code == ops.SCALER['attenuation']:
        return float(np.float32(avg / math.log(D + 1)))
    return 1.0


def _codes(names, table, what):
    out = []
    for n in names:
        if str(n).startswith('moment'):
            # reference models/pna.py:40-46: sign(m) (|m| + eps)^(1/n) with m = mean((x - mean(x))^n).  For odd n, m of a node with
            # two in-edges is (a)^n + (-a)^n = 0 up to the rounding of the mean, so the reference's own output there is
            # +-eps^(1/n) = +-0.02 by the sign of rounding noise (0 exactly for in-degree 1): there is no value to be on a par
            # with except by repeating torch's instruction order bit for bit.  No configuration of the reference uses them.
            raise NotImplementedError(f'{what} {n!r}: the moment aggregators are not offered (discontinuous at m = 0, which every '
                                      'node of in-degree 2 hits up to rounding for odd n: DESIGN.md, out of scope)')
        if n not in table:
            raise NotImplementedError(f'{what} {n!r} has no HIP kernel yet (supported: {sorted(table)})')
        out.append(table[n])
    return out


class PNA(nn.Module):
    """Message Passing Neural Network that does not use 3D information (reference models/pna.py:90-135)."""

    def __init__(self, hidden_dim, target_dim, aggregators: List[str], scalers: List[str],
                 readout_aggregators: List[str], readout_batchnorm: bool = True, readout_hidden_dim=None,
                 readout_layers: int = 2, residual: bool = True, pairwise_distances: bool = False,
                 activation: Union[Callable, str] = "relu", last_activation: Union[Callable, str] = "none",
                 mid_batch_norm: bool = False, last_batch_norm: bool = False, propagation_depth: int = 5,
                 dropout: float = 0.0, posttrans_layers: int = 1, pretrans_layers: int = 1, batch_norm_momentum=0.1,
                 **kwargs):
        super().__init__()
        self.node_gnn = PNAGNN(hidden_dim=hidden_dim, aggregators=aggregators, scalers=scalers, residual=residual,
                               pairwise_distances=pairwise_distances, activation=activation,
                               last_activation=last_activation, mid_batch_norm=mid_batch_norm,
                               last_batch_norm=last_batch_norm, propagation_depth=propagation_depth, dropout=dropout,
                               posttrans_layers=posttrans_layers, pretrans_layers=pretrans_layers,
                               batch_norm_momentum=batch_norm_momentum)
        if readout_hidden_dim is None:
            readout_hidden_dim = hidden_dim
        self.readout_aggregators = readout_aggregators
        self._readout_codes = _codes(readout_aggregators, {k: ops.AGG[k] for k in ('mean', 'sum', 'max', 'min')},
                                     'readout aggregator')
        self.output = MLP(in_dim=hidden_dim * len(self.readout_aggregators), hidden_size=readout_hidden_dim,
                          mid_batch_norm=readout_batchnorm, out_dim=target_dim, layers=readout_layers,
                          batch_norm_momentum=batch_norm_momentum)

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float() replace the storage of parameters and buffers: the cached pointer descriptions of the
        # whole-model sequencer (pna_native) are stale
        self.__dict__.pop('_i3d_desc_fwd', None)
        self.__dict__.pop('_i3d_desc_bwd', None)
        return super()._apply(fn, *args, **kwargs)

    def forward(self, graph, *unused):
        g = as_batched_graph(graph)
        if self.training and g.device.type == 'cuda' and torch.is_grad_enabled():
            streams.note_step_start(g.device)       # lets an independent Net3D forward run next to this one
        if pna_native.eligible(self, g):      # the whole forward (and later the whole backward) from one C call
            out = pna_native.run(self, g)
            if out is not None:
                return out
        with bn_counter_scope():
            return tape.run_model(self, lambda: self._forward(g))     # one autograd node for the whole model

    def _forward(self, g):
        self.node_gnn(g)
        readout = tape.apply(ReadoutFn, g.ndata['feat'], g.index(), self._readout_codes)
        return self.output(readout)


class PNAGNN(nn.Module):
    """reference models/pna.py:138-166."""

    def __init__(self, hidden_dim, aggregators: List[str], scalers: List[str], residual: bool = True,
                 pairwise_distances: bool = False, activation: Union[Callable, str] = "relu",
                 last_activation: Union[Callable, str] = "none", mid_batch_norm: bool = False,
                 last_batch_norm: bool = False, batch_norm_momentum=0.1, propagation_depth: int = 5,
                 dropout: float = 0.0, posttrans_layers: int = 1, pretrans_layers: int = 1, **kwargs):
        super().__init__()
        self.mp_layers = nn.ModuleList()
        for _ in range(propagation_depth):
            self.mp_layers.append(
                PNALayer(in_dim=hidden_dim, out_dim=int(hidden_dim), in_dim_edges=hidden_dim, aggregators=aggregators,
                         scalers=scalers, pairwise_distances=pairwise_distances, residual=residual, dropout=dropout,
                         activation=activation, last_activation=last_activation, mid_batch_norm=mid_batch_norm,
                         last_batch_norm=last_batch_norm, avg_d={"log": 1.0}, posttrans_layers=posttrans_layers,
                         pretrans_layers=pretrans_layers, batch_norm_momentum=batch_norm_momentum))
        self.atom_encoder = AtomEncoder(emb_dim=hidden_dim)
        self.bond_encoder = BondEncoder(emb_dim=hidden_dim)

    def forward(self, graph):
        g = as_batched_graph(graph)
        idx = g.index()
        g.ndata['feat'] = self.atom_encoder(g.ndata['feat'])
        bond_idx = g.edata['feat']
        dims = self.bond_encoder.dims
        n_comb = 1
        for d in dims:
            n_comb *= d
        pairwise = any(l.pairwise_distances for l in self.mp_layers)
        if pairwise:
            # reference models/pna.py:243-245: every layer's edge input gets the squared distance of the end points' coordinates
            # (ndata['x']) as one more column - a per-edge value, so the bond-table form (60 joint values) does not apply: the
            # materialised embeddings [E, F], one column wider, built once for all layers
            ef_sorted = self.bond_encoder(bond_idx, perm=idx.perm)
            q = tape.apply(_AppendSqDistFn, ef_sorted, g.ndata['x'], idx)
            for mp_layer in self.mp_layers:
                mp_layer(g, ef_sorted=q if mp_layer.pairwise_distances else ef_sorted, dist_appended=True)
            g.edata['feat'] = ops.gather_rows(ef_sorted.detach(), idx.inv_perm)
            return
        if EDGE_TABLE and n_comb <= 256 and idx.num_edges > 0 and bond_idx.dtype == torch.int64:
            # the bond embedding takes n_comb (60) distinct values: every layer's  e_feat W_q^T  is a gather from the
            # [n_comb, F] table of all combinations times W_q^T (layers.EdgeTable) instead of an [E, F] x [F, F] product
            v_pad = (n_comb + 31) // 32 * 32
            table = self.bond_encoder(self._combinations(dims, bond_idx.device))
            codes, onehot = ops.edge_codes(bond_idx.contiguous(), idx.perm, dims, v_pad)
            qmap = EdgeTable(codes, onehot, n_comb, v_pad)
            for mp_layer in self.mp_layers:
                mp_layer(g, ef_sorted=table, qmap=qmap)
            with torch.no_grad(), tape.paused():   # reference side effect (models/pna.py:163): float bond embedding, edge-id order
                g.edata['feat'] = self.bond_encoder(bond_idx)
            return
        # bond embeddings are produced directly in destination-sorted (kernel) order
        ef_sorted = self.bond_encoder(bond_idx, perm=idx.perm)
        for mp_layer in self.mp_layers:
            mp_layer(g, ef_sorted=ef_sorted)
        # reference side effect (models/pna.py:163): edata['feat'] becomes the float bond embedding, edge-id order
        g.edata['feat'] = ops.gather_rows(ef_sorted.detach(), idx.inv_perm)

    def _combinations(self, dims, device):
        """[prod(dims), C] int64: row v holds the categories with joint code v (first column fastest, ops.edge_codes)."""
        key = (tuple(dims), str(device))
        cache = self.__dict__.setdefault('_comb_cache', {})
        if key not in cache:
            v = torch.arange(int(torch.tensor(dims).prod()), dtype=torch.int64)
            cols, stride = [], 1
            for d in dims:
                cols.append((v // stride) % d)
                stride *= d
            cache[key] = torch.stack(cols, 1).contiguous().to(device)
        return cache[key]


class _AppendSqDistFn(torch.autograd.Function):
    """[ef | d^2]: the edge features (destination-sorted, or None) with the squared end-point distance as last column
    (csrc/pack.hip: i3d_copy_cols + i3d_edge_sqdist; take_sqrt: the distance itself, the tower variant's use_3d); coordinates are
    data: the gradient is the crop."""

    @staticmethod
    def forward(ctx, ef, x, index, take_sqrt=False):
        E = index.num_edges
        x = x.contiguous().float()
        assert x.dim() == 2 and x.shape[1] == 3, "pairwise_distances=True needs the atom coordinates in ndata['x'] [N, 3]"
        F = ef.shape[1] if ef is not None else 0
        ctx.F = F
        out = torch.empty(E, F + 1, dtype=torch.float32, device=x.device)
        L = ops._lib.load()
        if ef is not None:
            ef = ef.contiguous()
            ops.check(L.i3d_copy_cols(ef.data_ptr(), E, F, out.data_ptr(), F + 1, ops._stream()), 'i3d_copy_cols')
        ops.check(L.i3d_edge_sqdist(x.data_ptr(), index.src_s.data_ptr(), index.dst_s.data_ptr(), E, out.data_ptr(), F + 1, F,
                                    int(take_sqrt), ops._stream()), 'i3d_edge_sqdist')
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.F == 0:
            return None, None, None, None
        g = g.contiguous()
        out = torch.empty(g.shape[0], ctx.F, dtype=torch.float32, device=g.device)
        ops.check(ops._lib.load().i3d_copy_cols(g.data_ptr(), g.shape[0], g.shape[1], out.data_ptr(), ctx.F, ops._stream()),
                  'i3d_copy_cols')
        return out, None, None, None


class _LayerPlan:
    """Non-tensor configuration of one PNALayerFn call (built by PNALayer.forward)."""
    __slots__ = ('pre_specs', 'post_specs', 'aggregators', 'agg_scalers', 'avg', 'coef', 'grouped', 'residual')


class PNALayerFn(torch.autograd.Function):
    """One PNA layer (reference models/pna.py:199-216) as ONE autograd node: pretrans edge MLP -> aggregation ->
    posttrans MLP (+ residual).  The steps are the forward/backward bodies of the block Functions of layers.py run back
    to back; the three contributions to dL/dh (edge MLP, posttrans, residual) are summed by i3d_add_inplace here
    instead of by autograd's accumulation (a torch add costs ~35 us of host time on this stack, an autograd node ~30 us;
    the host is on the critical path of the step).  params = (W, b, gamma, beta) of every pretrans FC layer, then of
    every posttrans FC layer."""

    @staticmethod
    def forward(ctx, h, q, index, qmap, plan, *params):
        ctx.native = None
        if layer_native.eligible(h, q, index, qmap, plan, params):      # the whole layer from one C call per direction
            return layer_native.forward(ctx, h, q, index, qmap, plan, params)
        k = 0
        subs = []
        W, b, ga, be = params[k:k + 4]
        k += 4
        c = tape.SubCtx((True, ctx.needs_input_grad[1]) + (True,) * 10)
        e = EdgeFCFn.forward(c, h, q, W, b, ga, be, index, plan.pre_specs[0], qmap)
        subs.append(c)
        for spec in plan.pre_specs[1:]:
            W, b, ga, be = params[k:k + 4]
            k += 4
            c = tape.SubCtx()
            e = FCFn.forward(c, e, W, b, ga, be, None, spec)
            subs.append(c)
        c = tape.SubCtx()
        a = AggregateFn.forward(c, e, index, plan.aggregators, plan.agg_scalers, plan.avg)
        subs.append(c)
        n_post = len(plan.post_specs)
        W, b, ga, be = params[k:k + 4]
        k += 4
        res0 = h if (plan.residual and n_post == 1) else None
        c = tape.SubCtx()
        if plan.grouped:
            x = GroupedConcat2FCFn.forward(c, h, a, W, b, ga, be, res0, index, plan.coef, plan.post_specs[0])
        else:
            x = Concat2FCFn.forward(c, h, a, W, b, ga, be, res0, plan.post_specs[0])
        subs.append(c)
        for i, spec in enumerate(plan.post_specs[1:]):
            W, b, ga, be = params[k:k + 4]
            k += 4
            c = tape.SubCtx()
            x = FCFn.forward(c, x, W, b, ga, be, h if (plan.residual and i == n_post - 2) else None, spec)
            subs.append(c)
        ctx.subs, ctx.plan = subs, plan
        return x

    @staticmethod
    def backward(ctx, grad):
        if ctx.native is not None:
            return layer_native.backward(ctx, grad)
        plan, subs = ctx.plan, list(ctx.subs)
        n_pre, n_post = len(plan.pre_specs), len(plan.post_specs)
        grad = grad.contiguous()
        post_grads, pre_grads = [], []
        g = grad
        for _ in range(n_post - 1):                       # plain posttrans layers, last first
            gx, gW, gb, gg, gbe, _, _ = FCFn.backward(subs.pop(), g)
            post_grads.insert(0, (gW, gb, gg, gbe))
            g = gx
        if plan.grouped:
            gh, gagg, gW, gb, gg, gbe = GroupedConcat2FCFn.backward(subs.pop(), g)[:6]
        else:
            gh, gagg, gW, gb, gg, gbe = Concat2FCFn.backward(subs.pop(), g)[:6]
        post_grads.insert(0, (gW, gb, gg, gbe))
        ge = AggregateFn.backward(subs.pop(), gagg)[0]
        for _ in range(n_pre - 1):
            gx, gW, gb, gg, gbe, _, _ = FCFn.backward(subs.pop(), ge)
            pre_grads.insert(0, (gW, gb, gg, gbe))
            ge = gx
        gh_edge, gq, gW, gb, gg, gbe = EdgeFCFn.backward(subs.pop(), ge)[:6]
        pre_grads.insert(0, (gW, gb, gg, gbe))
        ops.add_inplace(gh, gh_edge)                      # gh is a fresh buffer of the posttrans backward
        if plan.residual:
            ops.add_inplace(gh, grad)
        flat = [t for quad in pre_grads + post_grads for t in quad]
        return (gh, gq, None, None, None) + tuple(flat)


class PNALayer(nn.Module):
    """reference models/pna.py:169-252."""

    def __init__(self, in_dim: int, out_dim: int, in_dim_edges: int, aggregators: List[str], scalers: List[str],
                 activation: Union[Callable, str] = "relu", last_activation: Union[Callable, str] = "none",
                 dropout: float = 0.0, residual: bool = True, pairwise_distances: bool = False,
                 mid_batch_norm: bool = False, last_batch_norm: bool = False, batch_norm_momentum=0.1,
                 avg_d: Dict[str, float] = {"log": 1.0}, posttrans_layers: int = 2, pretrans_layers: int = 1):
        super().__init__()
        self.aggregators = _codes(aggregators, ops.AGG, 'aggregator')
        self.scalers = _codes(scalers, ops.SCALER, 'scaler')
        self.edge_features = in_dim_edges > 0
        self.activation = activation
        self.avg_d = avg_d
        self.pairwise_distances = pairwise_distances
        self.residual = residual
        if in_dim != out_dim:
            self.residual = False
        # (pairwise_distances: one more input column, the squared distance of the edge's end points, reference :243-249)
        self.pretrans = MLP(in_dim=2 * in_dim + in_dim_edges + (1 if pairwise_distances else 0), hidden_size=in_dim, out_dim=in_dim,
                            mid_batch_norm=mid_batch_norm, last_batch_norm=last_batch_norm, layers=pretrans_layers,
                            mid_activation=activation, dropout=dropout, last_activation=last_activation,
                            batch_norm_momentum=batch_norm_momentum)
        self.posttrans = MLP(in_dim=(len(aggregators) * len(scalers) + 1) * in_dim, hidden_size=out_dim,
                             out_dim=out_dim, layers=posttrans_layers, mid_activation=activation,
                             last_activation=last_activation, dropout=dropout, mid_batch_norm=mid_batch_norm,
                             last_batch_norm=last_batch_norm, batch_norm_momentum=batch_norm_momentum)

    def forward(self, g, ef_sorted=None, qmap=None, dist_appended=False):
        g = as_batched_graph(g)
        idx = g.index()
        h = g.ndata['feat']
        if ef_sorted is None and self.edge_features:
            ef_sorted = tape.apply(_GatherRowsFn, g.edata['feat'], idx.perm, idx.inv_perm)
        has_q = self.edge_features
        if self.pairwise_distances:
            if not dist_appended:       # stand-alone use: PNAGNN appends the column once for all its layers
                ef_sorted = tape.apply(_AppendSqDistFn, ef_sorted if self.edge_features else None, g.ndata['x'], idx)
            has_q, qmap = True, None
        avg = float(self.avg_d["log"])
        # degree-grouped posttrans; one scaler or an odd width: the reference-shaped path ([N, 12F] aggregate + K = 13F GEMM)
        grouped = len(self.scalers) > 1 and h.shape[1] % 4 == 0
        # per call: only the per-degree scaler coefficients depend on the batch (cached on its index: the layers of a
        # model share them); specs and parameters come from the FC layers' hot caches
        fcs = self.__dict__.get('_i3d_fcs')
        mods = (self.pretrans.fully_connected._modules, self.posttrans.fully_connected._modules)
        if fcs is None or any(len(k) != len(m) or any(m.get(n) is not fc for n, fc in k)
                              for k, m in zip(fcs[2], mods)):      # a replaced / added FC layer drops the cache
            keyed = tuple(tuple(m.items()) for m in mods)
            fcs = self.__dict__['_i3d_fcs'] = ([fc for _, fc in keyed[0]], [fc for _, fc in keyed[1]], keyed)
        pre, post = fcs[0], fcs[1]
        hots = [fc.hot() for fc in pre + post]
        plan = _LayerPlan()
        plan.pre_specs, plan.post_specs = [t[4] for t in hots[:len(pre)]], [t[4] for t in hots[len(pre):]]
        plan.aggregators, plan.avg, plan.grouped, plan.residual = self.aggregators, avg, grouped, self.residual
        plan.agg_scalers = [ops.SCALER['identity']] if grouped else self.scalers
        plan.coef = None
        if grouped:
            key = (tuple(self.scalers), avg)
            cache = idx.__dict__.setdefault('_i3d_coef', {})
            plan.coef = cache.get(key)
            if plan.coef is None:
                plan.coef = cache[key] = [[_scaler_coef(s, D, avg) for s in self.scalers]
                                          for D, _, _ in idx.degree_groups()[2]]
        params = [t for hot in hots for t in hot[:4]]
        h_new = tape.apply(PNALayerFn, h, ef_sorted if has_q else None, idx, qmap if has_q else None, plan, *params)
        g.ndata['feat'] = h_new
        return h_new


class _GatherRowsFn(torch.autograd.Function):
    """edge-id order -> destination-sorted order (standalone PNALayer use with a float edata['feat'])."""

    @staticmethod
    def forward(ctx, x, perm, inv_perm):
        ctx.inv_perm = inv_perm
        return ops.gather_rows(x.contiguous(), perm)

    @staticmethod
    def backward(ctx, g):
        return ops.gather_rows(g.contiguous(), ctx.inv_perm), None, None
