"""SAN, the spectral-attention graph transformer - drop-in for reference models/san.py (model_type 'SAN', configs/san.yml and
configs/san_ogbg.yml).

Same class names, constructor kwargs (unknown ones swallowed), sub-module names and hence state_dict keys - the unused
`embedding_e_fake` included: reference checkpoints load strict.  On the device nn.Linear / nn.BatchNorm1d / nn.LayerNorm / nn.Embedding
are PARAMETER CONTAINERS only; their forward is never called.

Per layer (reference models/san.py:147-256):
  * Q / K / V / Q_2 / K_2 are ONE stacked product [N, 5H] through the package's GEMM (_StackedLinearFn);
  * the edge features never change across the layers and a bond takes prod(dims) = 60 joint values, so E(e) and E_2(e) of an edge
    are rows of the two [60, H] tables TE = E(T0), TE2 = E_2(T0), T0 the bond embedding of all combinations, built once per
    forward by the encoder's own EmbeddingSumFn (whose backward sends the tables' gradients to the three embedding matrices);
  * score, clamp, exp, gamma weighting, weighted sum and normaliser of a destination are one launch per direction (csrc/san.hip): no
    [E, H] tensor exists in either direction, nh floats per edge and direction do (the scores, their gradients);
  * O_h with the residual added BEFORE batch_norm1_h / layer_norm1_h (:230-237): a Linear with a residual and no BatchNorm, then the
    norm as a step of its own (_BatchNormFn, distance_predictor._LayerNormResFn) - the fused Linear + BatchNorm + residual block
    of layers.py has the other order and is left as it is; the FFN is a fused Linear + ReLU, a Linear with the residual, the norm.

The learned positional encoding (linear_A, PE_Transformer, the NaN mask and nansum, :314-325; [m <= 10, N, 16], not the hot path)
runs on torch's own nn.TransformerEncoder, called exactly as the reference calls it, as one step of the tape: torch's module keeps
the reference's dropout stream (nn.TransformerEncoderLayer defaults to dropout 0.1).  The reference overwrites the NaNs of
g.ndata['pos_enc'] in place (:317); here the encoding is copied first and the caller's tensor is left as it was.

FUSED_ATTENTION = False is the composed path: the attention in torch ops on [E, nh, dh] tensors with the per-edge projections
E(e), E_2(e) materialised, as the reference computes it.  It is the in-tree cross-check, and what a layer takes - its `path`
attribute says 'composed' - when the kernel's lane map does not cover (H, heads) (csrc/san.hip), the bond features have more than
256 combinations or are not int64.  With the tensors on the host the whole model runs in torch (composed path only: the fixture
check that needs no device); there FUSED_ATTENTION = True is an error, not a fall-back.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import ops, tape
from .distance_predictor import _LayerNormResFn
from .gin import _combinations
from .graph import as_batched_graph
from .layers import MLP, BNSpec, FCFn, FCSpec, ReadoutFn, _Tail, bn_counter_scope, dropout as _dropout
from .mol_encoder import AtomEncoder, BondEncoder

# False: the attention composed of torch ops, [E, H] tensors materialised (cross-check)
FUSED_ATTENTION = True
MAX_CODES = 256

_LINEAR = FCSpec(None, None)
_RELU = FCSpec('relu', None)


def composed_attention(Y, Ee, Ee2, src, dst, real, num_heads, gamma, full_graph):
    """reference models/san.py:111-177 in torch ops: Y = Q | K | V (| Q_2 | K_2) [N, 3H or 5H], Ee / Ee2 [E, H] the edge projections,
    src / dst [E] int64, real [E] bool -> [N, H]"""
    N, E = Y.shape[0], src.shape[0]
    H = Y.shape[1] // (5 if full_graph else 3)
    dh = H // num_heads
    blocks = Y.split(H, 1)
    Q, K, V = blocks[:3]
    score = K[src] * Q[dst] / math.sqrt(dh) * Ee
    coef = None
    if full_graph:
        Q2, K2 = blocks[3:]
        sel = real[:, None]
        score = torch.where(sel, score, K2[src] * Q2[dst] / math.sqrt(dh) * Ee2)
        coef = torch.where(real, 1.0 / (gamma + 1.0), gamma / (gamma + 1.0)).to(Y.dtype)[:, None]
    w = torch.exp(score.view(E, num_heads, dh).sum(-1).clamp(-5, 5))
    if coef is not None:
        w = w * coef
    wV = torch.zeros(N, num_heads, dh, dtype=Y.dtype, device=Y.device).index_add_(0, dst, V[src].view(E, num_heads, dh) * w[:, :, None])
    z = torch.zeros(N, num_heads, dtype=Y.dtype, device=Y.device).index_add_(0, dst, w)
    return (wV / (z[:, :, None] + 1e-6)).reshape(N, H)


# ---- steps of the tape ----------------------------------------------------------------------------------------------------------
class _TorchSectionFn(torch.autograd.Function):
    """run(*inputs) in torch ops as ONE step: the section's own autograd graph is kept from the forward (a dropout inside draws its
    mask once) and walked by torch.autograd.grad in the backward.  Parameters go in as they are, other tensors detached."""

    @staticmethod
    def forward(ctx, run, *inputs):
        with torch.enable_grad():
            xs = [a if isinstance(a, nn.Parameter) else a.detach().requires_grad_() for a in inputs]
            out = run(*xs)
        ctx.section = (out, xs)
        return out.detach()

    @staticmethod
    def backward(ctx, g):
        out, xs = ctx.section
        live = [x for x in xs if x.requires_grad]
        grads = iter(torch.autograd.grad(out, live, g, allow_unused=True))
        return (None, *[next(grads) if x.requires_grad else None for x in xs])


def _torch_section(run, *inputs):
    if tape.active() is None and not torch.is_grad_enabled():      # (inside a model's tape grad mode is off, and the tape records)
        return run(*inputs)
    return tape.apply(_TorchSectionFn, run, *inputs)


class _StackedLinearFn(torch.autograd.Function):
    """x [N, in] -> x W^T (+ b) [N, n H] with W the n weights [H, in] stacked: the projections of a layer as one product"""

    @staticmethod
    def forward(ctx, x, n, *wb):
        x = x.contiguous()
        W = torch.cat(wb[:n], 0)
        b = torch.cat(wb[n:]) if len(wb) > n else None
        ctx.n, ctx.rows, ctx.has_bias = n, [w.shape[0] for w in wb[:n]], b is not None
        ctx.save_for_backward(x, W)
        return ops.gemm(x, W, trans_b=True, bias=b)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        g = g.contiguous()
        gW = ops.gemm(g, x, trans_a=True).split(ctx.rows, 0)
        gb = ops.colsum(g).split(ctx.rows) if ctx.has_bias else ()
        gx = ops.gemm(g, W) if ctx.needs_input_grad[0] else None
        return (gx, None, *gW, *gb)


class _SANAttnFn(torch.autograd.Function):
    """csrc/san.hip: the attention of one layer from the stacked projections and the two tables, one launch forward, four backward"""

    @staticmethod
    def forward(ctx, Y, TE, TE2, ec, heads, gamma, full_graph):
        Y, TE = Y.contiguous(), TE.contiguous()
        TE2 = TE2.contiguous() if full_graph else None
        idx = ec.index
        res = ops.san_attn_fwd(Y, TE, TE2, ec.codes, ec.real, idx.in_ptr, idx.src_s, heads, gamma, full_graph)
        if res is None:
            raise RuntimeError(f'the SAN attention kernel does not take H={TE.shape[1]}, heads={heads}, {TE.shape[0]} codes '
                               '(csrc/san.hip); the composed path does')
        out, s, z = res
        ctx.cfg = (ec, heads, gamma, full_graph)
        ctx.save_for_backward(Y, TE, TE2, out, s, z)
        return out

    @staticmethod
    def backward(ctx, g):
        Y, TE, TE2, out, s, z = ctx.saved_tensors
        ec, heads, gamma, full_graph = ctx.cfg
        dY, dte, dte2 = ops.san_attn_bwd(g.contiguous(), out, z, s, Y, TE, TE2, ec.codes, ec.real, ec.index, ec.code_order, ec.code_ptr,
                                         heads, gamma, full_graph)
        return dY, dte, dte2, None, None, None, None


class _BatchNormFn(torch.autograd.Function):
    """nn.BatchNorm1d on its own (the statistics / apply kernels of the fused blocks, layers._Tail, without a Linear in front)"""

    @staticmethod
    def forward(ctx, x, gamma, beta, spec):
        y, ctx.saved = _Tail.forward(x.contiguous(), gamma, beta, spec)
        ctx.spec = spec
        ctx.save_for_backward(gamma, beta)
        return y

    @staticmethod
    def backward(ctx, g):
        gamma, beta = ctx.saved_tensors
        gx, gg, gb = _Tail.backward(ctx.saved, g.contiguous(), gamma, beta, ctx.spec)
        return gx, gg, gb, None


class _CatFn(torch.autograd.Function):
    """torch.cat((a, b), 1)"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.widths = (a.shape[1], b.shape[1])
        return torch.cat((a, b), 1)

    @staticmethod
    def backward(ctx, g):
        ga, gb = g.split(ctx.widths, 1)
        return ga.contiguous(), gb.contiguous()


class _EdgeContext:
    """what every layer of one forward shares: the kernel index; for the kernels the joint bond codes, the real flags and the
    code-sorted edge list (None: composed only); for the composed path the edge list, real flags and bond features in
    destination-sorted order as int64 / bool tensors, built when first asked for (the fused path never reads them)"""

    def __init__(self, index, bond_idx, real_in, full_graph):
        self.index, self.bond_idx, self.real_in, self.full_graph = index, bond_idx, real_in, full_graph
        self.comb = self.codes = self.real = self.code_order = self.code_ptr = None
        self._lazy = {}

    def _once(self, key, make):
        if key not in self._lazy:
            self._lazy[key] = make()
        return self._lazy[key]

    @property
    def perm(self):
        return self._once('perm', lambda: self.index.perm.long())

    @property
    def src(self):
        return self._once('src', lambda: self.index.src_s.long())

    @property
    def dst(self):
        return self._once('dst', lambda: self.index.dst_s.long())

    @property
    def real_b(self):
        return self._once('real_b', lambda: self.real_in[self.perm] != 0) if self.full_graph else None

    @property
    def bond_s(self):
        return self._once('bond_s', lambda: self.bond_idx[self.perm].long())


def edge_context(g, dims, full_graph):
    """the _EdgeContext of a batch, cached on its kernel index (a resident batch is coded and sorted once; the index, unlike the
    graph object, is shared by BatchedMolGraph.local_copy())"""
    bond_idx = g.edata['feat']
    real_in = g.edata['real'] if full_graph else None
    idx = g.index()
    ent = idx.__dict__.get('_san_edge_context')
    if ent is not None and ent.bond_idx is bond_idx and ent.real_in is real_in and ent.full_graph == full_graph:
        return ent
    c = _EdgeContext(idx, bond_idx, real_in, full_graph)
    n_comb = 1
    for d in dims:
        n_comb *= d
    if (bond_idx.is_cuda and n_comb <= MAX_CODES and bond_idx.dtype == torch.int64
            and (real_in is None or real_in.dtype == torch.int64)):
        c.comb = _combinations(dims, bond_idx.device)
        c.codes, c.real = ops.san_edge_codes(bond_idx.contiguous(), real_in, idx.perm, dims)
        c.code_order, c.code_ptr = ops.code_sorted_index(c.codes, n_comb)
    idx.__dict__['_san_edge_context'] = c
    return c


def _composed_context(g, full_graph):
    """the context of the reference-signature entries (arbitrary edge features: no codes, composed only)"""
    return _EdgeContext(g.index(), None, g.edata['real'] if full_graph else None, full_graph)


def _bn_spec(bn, training):
    return FCSpec(None, BNSpec(bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps, training))


def _lin(x, lin, spec=_LINEAR, residual=None):
    return tape.apply(FCFn, x, lin.weight, lin.bias, None, None, residual, spec)


# ---- modules ------------------------------------------------------------------------------------------------------------------
class MultiHeadAttentionLayer(nn.Module):
    """reference models/san.py:78-177.  `path` names what the last forward took: 'fused' (csrc/san.hip) or 'composed'."""

    def __init__(self, gamma, in_dim, out_dim, num_heads, full_graph, use_bias):
        super().__init__()
        self.out_dim, self.num_heads, self.gamma, self.full_graph = out_dim, num_heads, gamma, full_graph
        width = out_dim * num_heads
        self.Q = nn.Linear(in_dim, width, bias=use_bias)
        self.K = nn.Linear(in_dim, width, bias=use_bias)
        self.E = nn.Linear(in_dim, width, bias=use_bias)
        if full_graph:
            self.Q_2 = nn.Linear(in_dim, width, bias=use_bias)
            self.K_2 = nn.Linear(in_dim, width, bias=use_bias)
            self.E_2 = nn.Linear(in_dim, width, bias=use_bias)
        self.V = nn.Linear(in_dim, width, bias=use_bias)
        self.path = None

    def _projections(self):
        return [self.Q, self.K, self.V] + ([self.Q_2, self.K_2] if self.full_graph else [])

    def takes_fused(self, ec):
        return (FUSED_ATTENTION and ec.codes is not None
                and ops.san_attn_takes(self.out_dim * self.num_heads, self.num_heads, ec.comb.shape[0]))

    def attend(self, ec, h, T0, emb):
        """-> [N, heads * out_dim]; T0 [V, in_dim]: the bond embedding of every combination (fused), emb() -> [E, in_dim]: the edges'
        own (composed), destination-sorted"""
        if not h.is_cuda:
            return self._attend_host(ec, h, emb())
        lins = self._projections()
        biases = [m.bias for m in lins] if lins[0].bias is not None else []
        Y = tape.apply(_StackedLinearFn, h, len(lins), *[m.weight for m in lins], *biases)
        if self.takes_fused(ec):
            self.path = 'fused'
            TE = _lin(T0, self.E)
            TE2 = _lin(T0, self.E_2) if self.full_graph else None
            return tape.apply(_SANAttnFn, Y, TE, TE2, ec, self.num_heads, self.gamma, self.full_graph)
        self.path = 'composed'
        e = emb()
        Ee = _lin(e, self.E) if e.shape[0] else e.new_zeros(0, Y.shape[1] // len(lins))
        Ee2 = (_lin(e, self.E_2) if e.shape[0] else Ee) if self.full_graph else Ee
        return _torch_section(lambda y, a, b: composed_attention(y, a, b, ec.src, ec.dst, ec.real_b, self.num_heads, self.gamma,
                                                                 self.full_graph), Y, Ee, Ee2)

    def _attend_host(self, ec, h, e):
        if FUSED_ATTENTION:
            raise RuntimeError('san.FUSED_ATTENTION = True needs the tensors on the device (csrc/san.hip has no host form); '
                               'set san.FUSED_ATTENTION = False for the composed path in torch')
        self.path = 'composed'
        Y = torch.cat([m(h) for m in self._projections()], 1)
        return composed_attention(Y, self.E(e), self.E_2(e) if self.full_graph else None, ec.src, ec.dst, ec.real_b, self.num_heads,
                                  self.gamma, self.full_graph)

    def forward(self, g, h, e):
        """the reference's signature: e [E, in_dim] are the edges' features in edge-id order -> [N, heads, out_dim].  Arbitrary edge
        features have no table: this entry is the composed path; the models call attend()."""
        g = as_batched_graph(g)
        ec = _composed_context(g, self.full_graph)
        perm = ec.perm
        if not h.is_cuda:
            out = self._attend_host(ec, h, e[perm])
        else:
            out = self.attend(ec, h, None, lambda: e[perm].contiguous())
        return out.view(-1, self.num_heads, self.out_dim)


class GraphTransformerLayer(nn.Module):
    """reference models/san.py:180-256"""

    def __init__(self, gamma, in_dim, out_dim, num_heads, full_graph, dropout=0.0, layer_norm=False, batch_norm=True, residual=True,
                 use_bias=False):
        super().__init__()
        if out_dim % num_heads:
            raise ValueError(f'num_heads={num_heads} does not divide out_dim={out_dim}')
        if residual and in_dim != out_dim:
            raise ValueError(f'residual=True with in_dim={in_dim} != out_dim={out_dim} (the reference fails at models/san.py:231)')
        self.in_channels, self.out_channels, self.num_heads, self.dropout = in_dim, out_dim, num_heads, dropout
        self.residual, self.layer_norm, self.batch_norm = residual, layer_norm, batch_norm
        self.attention = MultiHeadAttentionLayer(gamma, in_dim, out_dim // num_heads, num_heads, full_graph, use_bias)
        self.O_h = nn.Linear(out_dim, out_dim)
        if layer_norm:
            self.layer_norm1_h = nn.LayerNorm(out_dim)
        if batch_norm:
            self.batch_norm1_h = nn.BatchNorm1d(out_dim)
        self.FFN_h_layer1 = nn.Linear(out_dim, out_dim * 2)
        self.FFN_h_layer2 = nn.Linear(out_dim * 2, out_dim)
        if layer_norm:
            self.layer_norm2_h = nn.LayerNorm(out_dim)
        if batch_norm:
            self.batch_norm2_h = nn.BatchNorm1d(out_dim)

    def _residual_norm(self, x, lin, res, ln, bn, spec=_LINEAR):
        """norms(res + lin(x)): the residual inside the Linear's launch, or inside the LayerNorm's when there is one"""
        res = res if self.residual else None
        if not self.layer_norm:
            y = _lin(x, lin, spec, res)
        else:
            y = _lin(x, lin, spec)
            y = tape.apply(_LayerNormResFn, y, res if res is not None else torch.zeros_like(y), ln.weight, ln.bias, ln.eps)
        if self.batch_norm:
            y = tape.apply(_BatchNormFn, y, bn.weight, bn.bias, _bn_spec(bn, self.training))
        return y

    def step(self, ec, h, T0, emb):
        if not h.is_cuda:
            return self._step_host(ec, h, emb)
        att = _dropout(self.attention.attend(ec, h, T0, emb), self.dropout, self.training)
        h = self._residual_norm(att, self.O_h, h, getattr(self, 'layer_norm1_h', None), getattr(self, 'batch_norm1_h', None))
        f = _dropout(_lin(h, self.FFN_h_layer1, _RELU), self.dropout, self.training)
        return self._residual_norm(f, self.FFN_h_layer2, h, getattr(self, 'layer_norm2_h', None), getattr(self, 'batch_norm2_h', None))

    def _step_host(self, ec, h, emb):
        """the reference's lines in torch (tensors on the host)"""
        h_in1 = h
        h = F.dropout(self.attention.attend(ec, h, None, emb), self.dropout, training=self.training)
        h = self.O_h(h)
        if self.residual:
            h = h_in1 + h
        if self.layer_norm:
            h = self.layer_norm1_h(h)
        if self.batch_norm:
            h = self.batch_norm1_h(h)
        h_in2 = h
        h = F.dropout(F.relu(self.FFN_h_layer1(h)), self.dropout, training=self.training)
        h = self.FFN_h_layer2(h)
        if self.residual:
            h = h_in2 + h
        if self.layer_norm:
            h = self.layer_norm2_h(h)
        if self.batch_norm:
            h = self.batch_norm2_h(h)
        return h

    def forward(self, g, h, e):
        """the reference's signature (e [E, in_dim] in edge-id order): the composed path of MultiHeadAttentionLayer.forward"""
        g = as_batched_graph(g)
        ec = _composed_context(g, self.attention.full_graph)
        perm = ec.perm
        return self.step(ec, h, None, lambda: e[perm].contiguous()), e


class SAN_NodeLPE(nn.Module):
    """reference models/san.py:278-334.  forward(g) leaves the final node state in g.ndata['feat']; g.ndata['pos_enc'] [N, m, 2] is
    read through a copy (the reference zeroes its NaNs in place)."""

    def __init__(self, node_dim=None, edge_dim=None, batch_norm_momentum=0.1, residual=True, in_feat_dropout=0.0, dropout=0.0,
                 layer_norm=False, batch_norm=True, gamma=1e-6, full_graph=True, GT_hidden_dim=64, GT_n_heads=4, GT_out_dim=64,
                 GT_layers=10, LPE_n_heads=4, LPE_layers=3, LPE_dim=16, **kwargs):
        super().__init__()
        if GT_hidden_dim % GT_n_heads or GT_out_dim % GT_n_heads:
            raise ValueError(f'GT_n_heads={GT_n_heads} does not divide GT_hidden_dim={GT_hidden_dim} / GT_out_dim={GT_out_dim}')
        if residual and GT_out_dim != GT_hidden_dim:
            raise ValueError(f'GT_out_dim={GT_out_dim} != GT_hidden_dim={GT_hidden_dim} with residual=True: the last layer cannot add '
                             'its input (the reference fails at models/san.py:231)')
        self.residual, self.layer_norm, self.batch_norm = residual, layer_norm, batch_norm
        self.full_graph = full_graph
        self.in_feat_dropout = nn.Dropout(in_feat_dropout)
        self.embedding_h = AtomEncoder(emb_dim=GT_hidden_dim - LPE_dim)
        self.embedding_e_real = BondEncoder(emb_dim=GT_hidden_dim)
        self.embedding_e_fake = BondEncoder(emb_dim=GT_hidden_dim)      # unused, as in the reference: kept for the state_dict
        self.linear_A = nn.Linear(2, LPE_dim)
        encoder_layer = nn.TransformerEncoderLayer(d_model=LPE_dim, nhead=LPE_n_heads)
        self.PE_Transformer = nn.TransformerEncoder(encoder_layer, num_layers=LPE_layers)
        self.layers = nn.ModuleList([GraphTransformerLayer(gamma, GT_hidden_dim, GT_hidden_dim, GT_n_heads, full_graph, dropout,
                                                           layer_norm, batch_norm, residual) for _ in range(GT_layers - 1)])
        self.layers.append(GraphTransformerLayer(gamma, GT_hidden_dim, GT_out_dim, GT_n_heads, full_graph, dropout, layer_norm,
                                                 batch_norm, residual))

    def _learned_pe(self, pos_enc):
        """reference :314-325 on a copy of pos_enc, torch's modules called as the reference calls them -> [N, LPE_dim]"""
        pos = pos_enc.clone()
        empty_mask = torch.isnan(pos)
        pos[empty_mask] = 0

        def run(*_params):
            x = torch.transpose(pos, 0, 1).float()
            x = self.linear_A(x)
            x = self.PE_Transformer(src=x, src_key_padding_mask=empty_mask[:, :, 0])
            x[torch.transpose(empty_mask, 0, 1)[:, :, 0]] = float('nan')
            return torch.nansum(x, 0, keepdim=False)

        if not pos.is_cuda:
            return run()
        return _torch_section(run, *self.linear_A.parameters(), *self.PE_Transformer.parameters())

    def forward(self, g):
        g = as_batched_graph(g)
        with bn_counter_scope():
            return tape.run_model(self, lambda: self._forward(g))

    def _forward(self, g):
        atom_idx = g.ndata['feat']
        ec = edge_context(g, self.embedding_e_real.dims, self.full_graph)
        pe = self._learned_pe(g.ndata['pos_enc'])
        if not atom_idx.is_cuda:
            h = sum(emb(atom_idx[:, k].long()) for k, emb in enumerate(self.embedding_h.atom_embedding_list))
            h = self.in_feat_dropout(torch.cat((h, pe), 1))
            e = sum(emb(ec.bond_s[:, k]) for k, emb in enumerate(self.embedding_e_real.bond_embedding_list)) if ec.bond_s.shape[0] \
                else pe.new_zeros(0, h.shape[1])
            T0, emb_fn = None, (lambda: e)
        else:
            # (GT_hidden_dim == LPE_dim: an atom embedding of width 0, the node state is the learned encoding alone)
            h = tape.apply(_CatFn, self.embedding_h(atom_idx), pe) if self.embedding_h.atom_embedding_list[0].embedding_dim else pe
            h = _dropout(h, self.in_feat_dropout.p, self.training)
            T0 = self.embedding_e_real(ec.comb) if ec.comb is not None else None
            cache = []

            def emb_fn():       # the composed path's [E, H] bond embedding, built when the first layer asks for it
                if not cache:
                    cache.append(self.embedding_e_real(ec.bond_s.contiguous()) if ec.bond_s.shape[0]
                                 else h.new_zeros(0, h.shape[1]))
                return cache[0]
        for conv in self.layers:
            h = conv.step(ec, h, T0, emb_fn)
        g.ndata['feat'] = h
        return h


def _mlp_host(mlp, x):
    """layers.MLP in torch (tensors on the host): Linear -> activation -> dropout -> BatchNorm per FCLayer"""
    for fc in mlp.fully_connected:
        x = fc.linear(x)
        if fc.activation is not None:
            x = F.leaky_relu(x) if fc.activation == 'leakyrelu' else getattr(F, fc.activation)(x)
        if fc.dropout is not None:
            x = fc.dropout(x)
        if fc.batch_norm is not None:
            x = fc.batch_norm(x)
    return x


class SAN(nn.Module):
    """reference models/san.py:259-275.  forward(g) -> [B, target_dim]; g: BatchedMolGraph or a DGL graph with the integer atom / bond
    features in ndata['feat'] / edata['feat'] ([E, 3] int64), edata['real'] [E] and ndata['pos_enc'] [N, m, 2] (graph.san_graph)."""

    def __init__(self, GT_out_dim, readout_hidden_dim, readout_batchnorm, readout_aggregators, target_dim, readout_layers,
                 batch_norm_momentum, **kwargs):
        super().__init__()
        self.readout_aggregators = readout_aggregators
        self.gnn = SAN_NodeLPE(GT_out_dim=GT_out_dim, batch_norm_momentum=batch_norm_momentum, **kwargs)
        self.output = MLP(in_dim=GT_out_dim * len(self.readout_aggregators), hidden_size=readout_hidden_dim,
                          mid_batch_norm=readout_batchnorm, out_dim=target_dim, layers=readout_layers,
                          batch_norm_momentum=batch_norm_momentum)
        self._readout_codes = ops.agg_codes(readout_aggregators)

    def forward(self, g):
        g = as_batched_graph(g)
        with bn_counter_scope():
            return tape.run_model(self, lambda: self._forward(g))

    def _forward(self, g):
        h = self.gnn._forward(g)
        if not h.is_cuda:
            parts = torch.split(h, g.batch_num_nodes().tolist())
            red = {'sum': lambda s: s.sum(0), 'mean': lambda s: s.mean(0), 'max': lambda s: s.max(0)[0], 'min': lambda s: s.min(0)[0]}
            readout = torch.cat([torch.stack([red[a](s) for s in parts]) for a in self.readout_aggregators], -1)
            return _mlp_host(self.output, readout)
        return self.output(tape.apply(ReadoutFn, h, g.index(), self._readout_codes))
