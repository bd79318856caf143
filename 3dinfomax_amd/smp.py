"""SMP - SphereNet's spherical message passing (reference models/spherical_message_passing.py, commons/spherical_encoding.py): the
reference's class names, constructor arguments and state_dict keys, so a reference checkpoint loads strict.

What runs where
  geometry + bases  once per batch in csrc/smp.hip (ops.smp_geometry, ops.smp_bases): the radius graph inside each molecule, the
                    triplet lists k -> j -> i grouped by ji and regrouped by kj, angle and torsion per triplet and the two raw bases
                    sbf [T, n k], t [T, n n k], evaluated in fp64 and stored fp32.  The reference builds them through about fifty
                    sympy-lambdified torch expressions and a SparseTensor round trip per batch.
  dist_emb          a torch expression: its freq is trained.
  dense layers      torch Linear + silu.  The first edge layer (init.lin, [3 H -> H] on [x_i | x_j | rbf]) is applied by column
                    blocks: the two node blocks as one [N, H] x [H, 2 H] product gathered to the edges, not an [E, 3 H] concatenation.
  triplet step      update_e's  scatter(x_kj[idx_kj] * lin_sbf2(lin_sbf1(sbf)) * lin_t2(lin_t1(t)), idx_ji)  as ONE launch per layer
                    (four in the backward) that never holds a [T, int_emb] tensor: the two wide products lin_sbf1, lin_t1 stay GEMMs
                    ([T, basis_emb] results), the two narrow ones are applied inside the kernel.  ops.smp_triplets_takes(I, Bs) states
                    the shapes the kernels take; any other shape runs the composed torch chain and update_e.path says 'composed'.
                    FUSED_TRIPLETS = False selects the composed chain everywhere (the cross-check of the tests).

Choices where the reference leaves room
  neighbour cap   32 in-neighbours per atom, torch_cluster's default max_num_neighbors; when more atoms are within the cutoff the 32
                  LOWEST INDICES are kept (the device kernel of torch_cluster stops scanning at the cap), so j -> i may exist without
                  i -> j.  The reference's xyztodat assumes symmetry; here a triplet is any in-edge k -> j of an edge j -> i with k != i.
  isolated atoms  always get a zero row of v (dim_size = N); the reference omits dim_size and fails when the last atom has no edge.
  refused         energy_and_force=True (needs gradients through the geometry, which is forward only) and any act but swish.
  precondition    `batch` is non-decreasing (what a PyG Batch and graph.GeometricBatch give): a molecule is a contiguous range of
                  atoms.  It is not checked on the device; CHECK_INPUTS = True checks it at the price of a host synchronisation.

Kept as the reference has them, on purpose: no envelope on sbf and t; the n^2 real harmonics ordered per l as [m = 0, cos m = 1..l,
sin m = l..1] (the reference's negative indexing); flat harmonic index f multiplied with the Bessel order f % n, not with its own l.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .mol_encoder import AtomEncoder

FUSED_TRIPLETS = True
CHECK_INPUTS = False
MAX_SPHERICAL, MAX_RADIAL = 7, 64


def swish(x):
    return F.silu(x)


def _is_swish(act):
    return act is swish or act is F.silu or isinstance(act, nn.SiLU) or (isinstance(act, str) and act.lower() in ('swish', 'silu'))


def _check_act(act, who):
    if not _is_swish(act):
        raise ValueError(f'{who}: act={act!r} is not supported, only swish (x * sigmoid(x)) is')
    return swish


def glorot_orthogonal(tensor, scale):
    """torch_geometric.nn.inits.glorot_orthogonal: an orthogonal matrix rescaled to variance scale / (fan_in + fan_out)"""
    if tensor is not None:
        torch.nn.init.orthogonal_(tensor.data)
        s = scale / ((tensor.size(-2) + tensor.size(-1)) * tensor.var())
        tensor.data *= s.sqrt()


# How the reference initialises a Linear (models/spherical_message_passing.py:53-57, 79-84, 130-153, 204-212):
#   'glorot'       weight glorot-orthogonal with scale 2, the bias - where there is one - zero
#   'glorot_w'     weight glorot-orthogonal with scale 2, the bias left at torch's default (update_v.lin_up)
#   'torch'        torch's own Linear default (init.lin_rbf_0, init.lin; the output matrix under an unknown output_init)
#   'zeros'        a zero weight (the output matrix under output_init='zeros')
def _linear(n_in, n_out, bias, how):
    lin = nn.Linear(n_in, n_out, bias=bias)
    lin.smp_init = how
    _reset_linear(lin)
    return lin


def _reset_linear(lin):
    how = lin.smp_init
    if how == 'torch':
        lin.reset_parameters()
    elif how == 'zeros':
        lin.weight.data.zero_()
    else:
        glorot_orthogonal(lin.weight, scale=2.0)
        if how == 'glorot' and lin.bias is not None:
            lin.bias.data.zero_()


def _reset_all(module):
    """every Linear of `module` below it that _linear built, by its own rule"""
    for m in module.modules():
        if isinstance(m, nn.Linear) and hasattr(m, 'smp_init'):
            _reset_linear(m)


# ---- the constants of the two bases, built on the host at construction time -------------------------------------------------
def _sph_jn(l, x):
    """spherical Bessel function of the first kind in fp64, upward recurrence (used at x >= pi, l <= 7 only)"""
    j0 = math.sin(x) / x
    if l == 0:
        return j0
    j1 = math.sin(x) / (x * x) - math.cos(x) / x
    for m in range(1, l):
        j0, j1 = j1, (2 * m + 1) / x * j1 - j0
    return j1


def _root(l, a, b):
    fa = _sph_jn(l, a)
    for _ in range(200):
        m = 0.5 * (a + b)
        fm = _sph_jn(l, m)
        if (fa < 0) == (fm < 0):
            a, fa = m, fm
        else:
            b = m
    return 0.5 * (a + b)


def bessel_zeros(n, k):
    """[n, k] the first k positive zeros of j_0 .. j_(n-1), by bracketing between the zeros of the order below, rounded to fp32 as
    the reference's Jn_zeros array is"""
    zeros = np.zeros((n, k), dtype=np.float32)
    zeros[0] = np.arange(1, k + 1) * np.pi
    points = [float(p) for p in np.arange(1, k + n) * np.pi]
    for l in range(1, n):
        points = [_root(l, points[j], points[j + 1]) for j in range(k + n - 1 - l)]
        zeros[l] = np.array(points[:k], dtype=np.float32)
        points = [float(np.float32(p)) for p in points]          # the reference brackets with its fp32 array
    return zeros


def bessel_normalizers(zeros):
    """[n, k] fp64 values of 1 / sqrt(j_(l+1)(z_lk)^2 / 2) from the fp32-rounded zeros, rounded as the reference rounds them.  The
    reference evaluates Jn(r, n) = sqrt(pi / (2 r)) * jv(n + 0.5, r) on its float32 zeros, and with NumPy >= 2 (a float32 scalar no
    longer promotes against a Python float) every step from there to 1 / x ** 0.5 stays float32; its basis functions carry those
    rounded values, up to 1e-7 off the exact ones.  The same steps in the same precision here, so the bases equal the reference's
    to fp64 rounding.  (Under NumPy 1.x the reference's steps promote to float64 and its normalisers are the exact ones: a
    checkpoint trained there sees bases up to 1e-7 off here.)"""
    f = np.float32
    n, k = zeros.shape
    half = np.zeros((n, k), dtype=f)
    for l in range(n):
        for q in range(k):
            r = f(zeros[l, q])
            jv = f(math.sqrt(2.0 * float(r) / math.pi) * _sph_jn(l + 1, float(r)))          # J_(l + 3/2)(r) in fp64, rounded once
            jn = f(np.sqrt(f(f(np.pi) / f(f(2) * r))) * jv)
            half[l, q] = f(f(0.5) * f(jn * jn))
    return (f(1) / half ** f(0.5)).astype(np.float64)


def harmonic_prefactors(n):
    """[n^2] fp64 in the list order of the bases: per l  [m = 0, cos m = 1..l, sin m = l..1]; sqrt(2) folded in for m > 0"""
    out = []
    for l in range(n):
        pre = [math.sqrt((2 * l + 1) * math.factorial(l - m) / (4 * math.pi * math.factorial(l + m))) for m in range(l + 1)]
        out += [pre[0]] + [2 ** 0.5 * pre[m] for m in range(1, l + 1)] + [2 ** 0.5 * pre[m] for m in range(l, 0, -1)]
    return np.array(out)


# ---- the radial embedding ---------------------------------------------------------------------------------------------------------
class dist_emb(nn.Module):
    """rbf[e, q] = u(x) sin(freq_q x), x = d_e / cutoff (reference commons/spherical_encoding.py:159-191), with DimeNet's envelope of
    exponent p = envelope_exponent + 1,
        u(x) = 1 / x - x^(p - 1) ((p + 1)(p + 2) / 2 - p (p + 2) x + p (p + 1) / 2 x^2),
    which goes to zero at the cutoff with two vanishing derivatives.  freq starts at pi (1 .. k) and is trained; no other state."""

    def __init__(self, num_radial, cutoff=5.0, envelope_exponent=5):
        super().__init__()
        self.cutoff = cutoff
        p = envelope_exponent + 1
        self.power = p - 1
        self.poly = ((p + 1) * (p + 2) / 2.0, -float(p * (p + 2)), p * (p + 1) / 2.0)          # ascending in x
        self.freq = nn.Parameter(torch.empty(num_radial))
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.freq.copy_(math.pi * torch.arange(1, self.freq.numel() + 1, dtype=self.freq.dtype))

    def forward(self, dist):
        x = dist.reshape(-1, 1) / self.cutoff
        c0, c1, c2 = self.poly
        envelope = x.reciprocal() - x.pow(self.power) * (c0 + x * (c1 + x * c2))
        return envelope * torch.sin(self.freq * x)


class _BasisTables:
    """the fp64 tables of ops.smp_bases, built once on the host and kept per device; no module state (the reference keeps none for
    its two basis modules), so no dtype cast of the model rounds them"""

    def __init__(self, num_spherical, num_radial, cutoff):
        if not (1 <= num_spherical <= MAX_SPHERICAL and 1 <= num_radial <= MAX_RADIAL):
            raise ValueError(f'num_spherical={num_spherical} outside 1..{MAX_SPHERICAL} or num_radial={num_radial} outside 1..{MAX_RADIAL}')
        self.num_spherical, self.num_radial, self.cutoff = num_spherical, num_radial, cutoff
        zeros = bessel_zeros(num_spherical, num_radial)
        self.host = (zeros.astype(np.float64), bessel_normalizers(zeros), harmonic_prefactors(num_spherical))
        self._on = {}

    def on(self, device):
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in self.host)
        return self._on[device]


class emb(nn.Module):
    def __init__(self, num_spherical, num_radial, cutoff, envelope_exponent):
        super().__init__()
        self.dist_emb = dist_emb(num_radial, cutoff, envelope_exponent)
        self.tables = _BasisTables(num_spherical, num_radial, cutoff)

    def reset_parameters(self):
        self.dist_emb.reset_parameters()

    def forward(self, pos, geo):
        """-> (rbf [E, k] differentiable in freq, sbf [T, n k], t [T, n n k]) and (angle, torsion) of the batch's geometry"""
        tb = self.tables
        angle, torsion, sbf, t = ops.smp_bases(pos, geo, tb.num_spherical, tb.num_radial, tb.cutoff, *tb.on(pos.device))
        return (self.dist_emb(geo.dist), sbf, t), (angle, torsion)


# ---- dense blocks -----------------------------------------------------------------------------------------------------------------
class ResidualLayer(nn.Module):
    """x + act(lin2(act(lin1(x)))) (reference models/spherical_message_passing.py:44-60)"""

    def __init__(self, hidden_channels, act=swish):
        super().__init__()
        self.act = _check_act(act, 'ResidualLayer')
        for name in ('lin1', 'lin2'):
            setattr(self, name, _linear(hidden_channels, hidden_channels, True, 'glorot'))

    def reset_parameters(self):
        _reset_all(self)

    def forward(self, x):
        inner = self.act(self.lin1(x))
        return torch.add(x, self.act(self.lin2(inner)))


def _residual_stack(layers, h):
    for layer in layers:
        h = layer(h)
    return h


class init(nn.Module):
    """The first edge state (reference :63-96): e1 = act(lin([x_i | x_j | act(lin_rbf_0(rbf))])), e2 = lin_rbf_1(rbf) * e1, x the atom
    embedding or, without node features, one trained row for every atom.  lin's weight [H, 3 H] is used by column blocks W_i | W_j |
    W_r:  x W_i^T and x W_j^T are one product over the N atoms, gathered by edge end and added to the rbf block's product - the same
    sum as the concatenated [E, 3 H] row times the weight, in another order, on E / N times fewer rows."""

    def __init__(self, num_radial, hidden_channels, act=swish, use_node_features=True):
        super().__init__()
        self.act = _check_act(act, 'init')
        self.use_node_features = use_node_features
        self.hidden_channels = hidden_channels
        if use_node_features:
            self.emb = AtomEncoder(emb_dim=hidden_channels)
        else:
            self.node_embedding = nn.Parameter(torch.randn(hidden_channels))
        self.lin_rbf_0 = _linear(num_radial, hidden_channels, True, 'torch')
        self.lin = _linear(3 * hidden_channels, hidden_channels, True, 'torch')
        self.lin_rbf_1 = _linear(num_radial, hidden_channels, False, 'glorot')
        if use_node_features:
            self.emb.reset_parameters()

    def reset_parameters(self):
        if self.use_node_features:
            self.emb.reset_parameters()
        _reset_all(self)

    def forward(self, x, emb, i, j):
        rbf = emb[0]
        H = self.hidden_channels
        w_nodes, w_rbf = self.lin.weight[:, :2 * H], self.lin.weight[:, 2 * H:]
        if self.use_node_features:
            both = F.linear(self.emb(x), torch.cat([w_nodes[:, :H], w_nodes[:, H:]], 0))          # [N, 2 H]: x W_i^T | x W_j^T
            ends = both[:, :H][i] + both[:, H:][j]
        else:
            ends = F.linear(self.node_embedding, w_nodes[:, :H] + w_nodes[:, H:])                # every atom is the same row
        e1 = self.act(ends + F.linear(self.act(self.lin_rbf_0(rbf)), w_rbf, self.lin.bias))
        return e1, self.lin_rbf_1(rbf) * e1


class _TripletFn(torch.autograd.Function):
    """ops.smp_triplets_fwd / _bwd: out [E, I] from x_down [E, I], sbf8, t8 [T, Bs] and the weights of lin_sbf2, lin_t2 [I, Bs]"""

    @staticmethod
    def forward(ctx, x, s8, t8, w1, w2, geo):
        x, s8, t8, w1, w2 = (a.detach().contiguous() for a in (x, s8, t8, w1, w2))
        out = ops.smp_triplets_fwd(x, s8, t8, w1, w2, geo)
        if out is None:
            raise RuntimeError(f'the triplet kernels do not take int_emb={x.shape[1]}, basis_emb={w1.shape[1]} (ops.smp_triplets_takes)')
        ctx.save_for_backward(x, s8, t8, w1, w2)
        ctx.geo = geo
        return out

    @staticmethod
    def backward(ctx, g):
        return ops.smp_triplets_bwd(g.contiguous(), *ctx.saved_tensors, ctx.geo) + (None,)


def triplets_composed(x, s8, t8, w1, w2, geo):
    """the reference's chain in torch ops; holds three [T, I] tensors"""
    x_kj = x[geo.idx_kj.long()] * F.linear(s8, w1)
    x_kj = x_kj * F.linear(t8, w2)
    return torch.zeros_like(x).index_add_(0, geo.idx_ji.long(), x_kj)


class update_e(nn.Module):
    """One interaction block (reference :99-187).  With H = hidden_channels, I = int_emb_size, Bs = basis_emb_size:
      down    x = act(lin_down(act(lin_kj(e1)) * lin_rbf2(lin_rbf1(rbf))))                                     [E, I]
      gather  agg[e] = sum over the triplets of e of x[idx_kj] * lin_sbf2(lin_sbf1(sbf)) * lin_t2(lin_t1(t))   [E, I]: the triplet step
      up      h = act(lin_ji(e1)) + act(lin_up(agg)), residual layers, h = e1 + act(lin(h)), residual layers   [E, H]
      out     (h, lin_rbf(rbf) * h)"""

    def __init__(self, hidden_channels, int_emb_size, basis_emb_size, num_spherical, num_radial, num_before_skip, num_after_skip,
                 act=swish):
        super().__init__()
        self.act = _check_act(act, 'update_e')
        H, I, Bs, k, n = hidden_channels, int_emb_size, basis_emb_size, num_radial, num_spherical
        # name, in, out, bias - in the reference's order, which is the order of the state_dict
        for name, n_in, n_out, bias in (('lin_rbf1', k, Bs, False), ('lin_rbf2', Bs, H, False), ('lin_sbf1', n * k, Bs, False),
                                        ('lin_sbf2', Bs, I, False), ('lin_t1', n * n * k, Bs, False), ('lin_t2', Bs, I, False),
                                        ('lin_rbf', k, H, False), ('lin_kj', H, H, True), ('lin_ji', H, H, True),
                                        ('lin_down', H, I, False), ('lin_up', I, H, False)):
            setattr(self, name, _linear(n_in, n_out, bias, 'glorot'))
        self.layers_before_skip = nn.ModuleList(ResidualLayer(H, act) for _ in range(num_before_skip))
        self.lin = _linear(H, H, True, 'glorot')
        self.layers_after_skip = nn.ModuleList(ResidualLayer(H, act) for _ in range(num_after_skip))
        self.path = None          # 'fused' or 'composed': what the last forward ran

    def reset_parameters(self):
        _reset_all(self)

    def forward(self, x, emb, geo):
        rbf, sbf, t = emb
        e1 = x[0]
        x_down = self.act(self.lin_down(self.act(self.lin_kj(e1)) * self.lin_rbf2(self.lin_rbf1(rbf))))

        s8, t8 = self.lin_sbf1(sbf), self.lin_t1(t)
        w1, w2 = self.lin_sbf2.weight, self.lin_t2.weight
        fused = FUSED_TRIPLETS and ops.smp_triplets_takes(w1.shape[0], w1.shape[1])
        self.path = 'fused' if fused else 'composed'
        agg = _TripletFn.apply(x_down, s8, t8, w1, w2, geo) if fused else triplets_composed(x_down, s8, t8, w1, w2, geo)

        h = _residual_stack(self.layers_before_skip, self.act(self.lin_ji(e1)) + self.act(self.lin_up(agg)))
        h = _residual_stack(self.layers_after_skip, e1 + self.act(self.lin(h)))
        return h, self.lin_rbf(rbf) * h


class update_v(nn.Module):
    """Atom output of an edge state (reference :190-221): the second edge tensor summed over every atom's in-edges (a zero row for an
    atom without edges), lin_up, num_output_layers x act(Linear), the bias-free output matrix `lin`.  output_init: 'zeros' or
    'GlorotOrthogonal' for that matrix; any other value leaves torch's default, as the reference does."""

    def __init__(self, hidden_channels, out_emb_size, out_channels, num_output_layers, act, output_init):
        super().__init__()
        self.act = _check_act(act, 'update_v')
        self.output_init = output_init
        self.lin_up = _linear(hidden_channels, out_emb_size, True, 'glorot_w')
        self.lins = nn.ModuleList(_linear(out_emb_size, out_emb_size, True, 'glorot') for _ in range(num_output_layers))
        self.lin = _linear(out_emb_size, out_channels, False, {'zeros': 'zeros', 'GlorotOrthogonal': 'glorot'}.get(output_init, 'torch'))

    def reset_parameters(self):
        bias = self.lin_up.bias.data.clone()          # the reference's reset leaves this bias as it is
        _reset_all(self)
        self.lin_up.bias.data.copy_(bias)

    def forward(self, e, i, num_nodes):
        per_atom = e[1].new_zeros(num_nodes, e[1].shape[1]).index_add_(0, i, e[1])
        v = self.lin_up(per_atom)
        for lin in self.lins:
            v = self.act(lin(v))
        return self.lin(v)


class update_u(nn.Module):
    def forward(self, u, v, batch):
        return u.index_add(0, batch, v)


class SMP(nn.Module):
    def __init__(self, energy_and_force, cutoff, propagation_depth, hidden_channels, target_dim, int_emb_size, basis_emb_size,
                 out_emb_size, num_spherical, num_radial, envelope_exponent=5, num_before_skip=1, num_after_skip=2,
                 num_output_layers=3, act=swish, output_init='GlorotOrthogonal', use_node_features=True, **kwargs):
        super().__init__()
        if energy_and_force:
            raise NotImplementedError('SMP: energy_and_force=True needs gradients through the geometry; the geometry and the bases are '
                                      'forward only here')
        act = _check_act(act, 'SMP')
        self.cutoff = cutoff
        self.energy_and_force = energy_and_force
        self.target_dim = target_dim

        def output():
            return update_v(hidden_channels, out_emb_size, target_dim, num_output_layers, act, output_init)

        self.init_e = init(num_radial, hidden_channels, act, use_node_features=use_node_features)
        self.init_v = output()
        self.init_u = update_u()
        self.emb = emb(num_spherical, num_radial, cutoff, envelope_exponent)
        self.update_vs = nn.ModuleList(output() for _ in range(propagation_depth))
        self.update_es = nn.ModuleList(update_e(hidden_channels, int_emb_size, basis_emb_size, num_spherical, num_radial,
                                                num_before_skip, num_after_skip, act) for _ in range(propagation_depth))
        self.update_us = nn.ModuleList(update_u() for _ in range(propagation_depth))

    def reset_parameters(self):
        for block in [self.init_e, self.init_v, self.emb, *self.update_es, *self.update_vs]:
            block.reset_parameters()

    def geometry(self, batch_data, pos=None):
        """(SmpGeometry, number of molecules) of a batch: any object with pos [N, 3] and a non-decreasing batch [N]; `pos`: the
        positions as a contiguous fp32 tensor when the caller already has them"""
        batch = batch_data.batch
        if pos is None:
            pos = batch_data.pos.detach().float().contiguous()
        if CHECK_INPUTS and batch.numel() > 1 and not bool((batch[1:] >= batch[:-1]).all()):
            raise ValueError('SMP: `batch` is not non-decreasing: the atoms of a molecule have to be contiguous')
        num_graphs = getattr(batch_data, 'num_graphs', None)
        if num_graphs is None:
            num_graphs = int(batch[-1]) + 1 if batch.numel() else 0
        return ops.smp_geometry(pos, batch, int(num_graphs), self.cutoff), int(num_graphs)

    def forward(self, batch_data):
        z, batch = batch_data.z, batch_data.batch.long()
        pos = batch_data.pos.detach().float().contiguous()
        geo, num_graphs = self.geometry(batch_data, pos)
        num_nodes = z.size(0)
        emb, _ = self.emb(pos, geo)
        i, j = geo.dst.long(), geo.src.long()

        e = self.init_e(z, emb, i, j)
        v = self.init_v(e, i, num_nodes)
        u = self.init_u(v.new_zeros(num_graphs, v.shape[1]), v, batch)
        for ue, uv, uu in zip(self.update_es, self.update_vs, self.update_us):
            e = ue(e, emb, geo)
            v = uv(e, i, num_nodes)
            u = uu(u, v, batch)
        return u
