"""Fixture of SMP / SphereNet (reference models/spherical_message_passing.py, commons/spherical_encoding.py): the unmodified reference on
seeded small molecules, forward + L1 loss + backward, once in fp32 and once in fp64 (model.double(), fp64 positions) ->
tests/golden/smp.npz.

    python tests/golden/gen_golden_smp.py          (imports the reference checkout, as gen_golden.py does)

Per configuration the file holds the molecules (z, pos, sizes), what rebuilds the state_dict (names, shapes, the seed of fill_state, a
sum per tensor; state_from_npz), the target, and of BOTH runs: u, dist, angle, torsion, the index lists (asserted equal between the
runs, stored once), rows [::BASIS_STEP] of the two raw bases, and of every parameter gradient the view grad_view() (at most 128
elements, evenly strided: the sphere_net.yml sizes hold a million parameters, the file has to stay below 1 MiB).  Only data.

Four configurations:
  a  sphere_net.yml's sizes (hidden 128, int_emb 64, basis_emb 8, out_emb 256, 3 spherical, 6 radial, target 1) at depth 2
  b  num_spherical 7 (the contrastive config's 3D side), target_dim 8, hidden 32, int_emb 24, basis_emb 4
  c  use_node_features=False, 2 spherical, 3 radial, basis_emb 1
  d  output_init='zeros' (the output matrices stay zero, u is zero and only they get a gradient), basis_emb 20: outside the triplet
     kernels' lane map
Molecules: four of 5 - 9 atoms, coordinates N(0, 1.8 A) redrawn until no pair is closer than 0.8 A, so neighbourhoods inside the 5 A
cutoff vary from one atom to all others.  Every atom must have a neighbour (the reference's scatter without dim_size needs the last one
to) and some triplet must have k as its only candidate.  The torsion is a minimum over
candidates that jump by 2 pi at the 0 / 2 pi wrap, so the molecule seed is advanced until, in fp64 (tests/smp_reference.py), no candidate
lies within 1e-4 of the wrap, no triplet angle within 1e-2 of 0 or pi and no atom has more than 32 neighbours; asserted here.

The candidate k_n == k of the torsion minimum.  xyztodat takes the cross product of a plane normal with itself there and relies on it
being zero: atan2(0, |p|^2) = 0 -> 2 pi, the candidate never wins.  torch's vectorised CPU kernels contract a1 b2 - a2 b1 into a fused
multiply-add, the self-product becomes the rounding error of a1 a2 (1e-18, either sign) and half of the torsions collapse to 1e-18.
The run therefore selects torch's plain CPU kernels (ATEN_CPU_CAPABILITY=default, set below before torch loads), where the product is
exactly zero; asserted: every triplet whose j has no other neighbour has torsion exactly 2 pi in both runs.

Stand-ins, registered at run time, each restating documented semantics:
  torch_geometric.nn.acts.swish(x)                     x * sigmoid(x)
  torch_geometric.nn.inits.glorot_orthogonal(t, scale) orthogonal_(t), then t *= sqrt(scale / ((fan_in + fan_out) * var(t)))
  torch_geometric.nn.radius_graph(pos, r, batch)       edge_index [2, E] = (source j, target i) for every pair of one example with
                                                       |pos_i - pos_j| < r, no self loops, at most 32 sources per target (the first
                                                       by index), targets ascending, sources ascending inside a target
  torch_scatter.scatter(src, index, dim=0, dim_size=None, reduce='sum')   out[index[p]] (+)= src[p] over dim 0, dim_size defaulting to
                                                       index.max() + 1; reduce='min' the per-index minimum
  torch_sparse.SparseTensor(row, col, value, sparse_sizes)   entries sorted by (row, col); A[idx] (a LongTensor of row numbers) the
                                                       matrix of those rows in the order of idx; set_value(None); sum(dim=1) the
                                                       entries per row when there is no value; storage.row() / col() / value()
numpy 2 dropped the alias np.math the reference calls (np.math.factorial); it is set to the math module for the run.  The reference
model is constructed under torch.no_grad(): current torch refuses dist_emb.reset_parameters' arange(out=Parameter) in grad mode.  That
call leaves `freq` with requires_grad False, so every parameter is set to require a gradient afterwards: the fixture holds freq's.
"""
import copy
import math
import os
import sys
import types

if __name__ == '__main__':          # the generator run only (the tests import this module for its tables), before torch loads
    os.environ['ATEN_CPU_CAPABILITY'] = 'default'

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402
import smp_reference as R  # noqa: E402

BASE = dict(energy_and_force=False, cutoff=5.0, envelope_exponent=5, num_before_skip=1, num_after_skip=2, num_output_layers=3)
CONFIGS = {
    'a': dict(BASE, propagation_depth=2, hidden_channels=128, target_dim=1, int_emb_size=64, basis_emb_size=8, out_emb_size=256,
              num_spherical=3, num_radial=6),
    'b': dict(BASE, propagation_depth=1, hidden_channels=32, target_dim=8, int_emb_size=24, basis_emb_size=4, out_emb_size=32,
              num_spherical=7, num_radial=6),
    'c': dict(BASE, propagation_depth=1, hidden_channels=16, target_dim=2, int_emb_size=8, basis_emb_size=1, out_emb_size=16,
              num_spherical=2, num_radial=3, use_node_features=False),
    'd': dict(BASE, propagation_depth=1, hidden_channels=16, target_dim=2, int_emb_size=72, basis_emb_size=20, out_emb_size=16,
              num_spherical=2, num_radial=3, output_init='zeros'),
}
SIZES = {'a': (5, 9, 7, 6), 'b': (9, 5, 8, 6), 'c': (6, 7, 5, 9), 'd': (7, 5, 9, 6)}
BASIS_STEP = {'a': 8, 'b': 32, 'c': 1, 'd': 2}
GRAD_KEEP = 128
WRAP_MARGIN, ANGLE_MARGIN = 1e-4, 1e-2
ATOM_DIMS = G.synth.ATOM_FEATURE_DIMS


# ---- stand-ins -------------------------------------------------------------------------------------------------------------------
def swish(x):
    return x * x.sigmoid()


def glorot_orthogonal(tensor, scale):
    if tensor is not None:
        torch.nn.init.orthogonal_(tensor.data)
        scale /= ((tensor.size(-2) + tensor.size(-1)) * tensor.var())
        tensor.data *= scale.sqrt()


def radius_graph(x, r, batch=None, loop=False, max_num_neighbors=32, flow='source_to_target'):
    assert not loop and flow == 'source_to_target'
    batch = torch.zeros(x.shape[0], dtype=torch.long) if batch is None else batch
    src, dst = [], []
    for i in range(x.shape[0]):
        near = [j for j in range(x.shape[0]) if j != i and batch[j] == batch[i] and float((x[i] - x[j]).pow(2).sum()) < r * r]
        near = near[:max_num_neighbors]
        src += near
        dst += [i] * len(near)
    return torch.tensor([src, dst], dtype=torch.long)


def scatter(src, index, dim=0, out=None, dim_size=None, reduce='sum'):
    assert dim == 0 and out is None
    size = int(index.max()) + 1 if dim_size is None else dim_size
    base = torch.zeros((size,) + tuple(src.shape[1:]), dtype=src.dtype)
    if reduce in ('sum', 'add'):
        return base.index_add(0, index, src)
    assert reduce == 'min'
    idx = index.reshape((-1,) + (1,) * (src.dim() - 1)).expand_as(src)
    return base.scatter_reduce(0, idx, src, 'amin', include_self=False)


class SparseTensor:
    def __init__(self, row, col, value=None, sparse_sizes=None, is_sorted=False):
        if not is_sorted:
            perm = torch.argsort(row * sparse_sizes[1] + col, stable=True)
            row, col, value = row[perm], col[perm], None if value is None else value[perm]
        self._row, self._col, self._value, self._sizes = row, col, value, tuple(sparse_sizes)
        self.storage = self

    def row(self):
        return self._row

    def col(self):
        return self._col

    def value(self):
        return self._value

    def set_value(self, value, layout=None):
        return SparseTensor(self._row, self._col, value, self._sizes, is_sorted=True)

    def sum(self, dim):
        assert dim == 1 and self._value is None
        return torch.bincount(self._row, minlength=self._sizes[0]).float()

    def __getitem__(self, idx):
        counts = torch.bincount(self._row, minlength=self._sizes[0])
        rowptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
        cnt = counts[idx]
        new_row = torch.repeat_interleave(torch.arange(idx.shape[0]), cnt)
        start = torch.repeat_interleave(rowptr[idx], cnt)
        within = torch.arange(int(cnt.sum())) - torch.repeat_interleave(cnt.cumsum(0) - cnt, cnt)
        pos = start + within
        return SparseTensor(new_row, self._col[pos], None if self._value is None else self._value[pos], (idx.shape[0], self._sizes[1]),
                            is_sorted=True)


def register_stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    acts = mod('torch_geometric.nn.acts', swish=swish)
    inits = mod('torch_geometric.nn.inits', glorot_orthogonal=glorot_orthogonal)
    tg_nn = mod('torch_geometric.nn', radius_graph=radius_graph, acts=acts, inits=inits)
    mod('torch_geometric', nn=tg_nn)
    mod('torch_scatter', scatter=scatter)
    mod('torch_sparse', SparseTensor=SparseTensor)
    if not hasattr(np, 'math'):
        np.math = math


# ---- inputs and weights ----------------------------------------------------------------------------------------------------------------
def molecules(sizes, seed):
    """z [N, 9] int64, pos [N, 3] fp32, batch [N]"""
    rng = np.random.default_rng(seed)
    zs, ps = [], []
    for n in sizes:
        while True:
            p = rng.normal(0.0, 1.8, size=(n, 3)).astype(np.float32)
            d = np.linalg.norm(p[:, None] - p[None], axis=-1) + 10 * np.eye(n)
            if d.min() >= 0.8:
                break
        ps.append(p)
        zs.append(np.stack([rng.integers(0, dim, size=n) for dim in ATOM_DIMS], 1).astype(np.int64))
    return np.concatenate(zs), np.concatenate(ps), np.repeat(np.arange(len(sizes)), sizes)


def conditions(pos, sizes, cutoff):
    """(closest candidate to the wrap, closest angle to 0 / pi, largest neighbour count before the cap, smallest neighbour count,
    triplets whose k is the only candidate) in fp64"""
    src, dst, in_ptr = R.radius_graph(pos, sizes, cutoff)
    _, _, trip_ptr = R.triplets(src, dst, in_ptr)
    _, angle, _, margin, single = R.angles(pos, src, dst, in_ptr, trip_ptr, np.float64)
    return (float(margin.min()), float(np.minimum(angle, math.pi - angle).min()), int(max(sizes)) - 1, int(np.diff(in_ptr).min()),
            int(single.sum()))


def _unit_noise(rng, shape):
    """float64 noise of mean 0 and variance 1, the same bits on every machine: the sum of four 16-bit integers of numpy's PCG64
    stream, centred and scaled - integer draws and exact float64 steps only.  torch.randn is NOT used for the weights: its vectorised
    CPU kernels and its plain ones (which the generator run selects) give values that differ in the last bit, the rebuilt weights
    would then be a rounding off the ones the reference ran with, and that alone costs the device tests most of their tolerance."""
    draws = rng.integers(0, 2 ** 16, size=tuple(shape) + (4,), dtype=np.int64).sum(-1)
    return (draws - 2 * (2 ** 16 - 1)).astype(np.float64) / (2 ** 16 / math.sqrt(3.0))


def fill_state(shapes, seed, zero_output):
    """{name: tensor} for the state_dict entries `shapes`, a pure function of names, shapes and seed, bit for bit (trained-like:
    matrices noise / sqrt(fan_in), embedding tables noise x 0.5, biases noise x 0.2, freq pi (1 .. k) + noise x 0.05, node_embedding
    noise; computed in float64, rounded to float32 once); with zero_output the output matrices `*_v*.lin.weight` stay zero"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape in shapes.items():
        shape = tuple(int(d) for d in shape)
        parts = name.split('.')
        if zero_output and parts[-2:] == ['lin', 'weight'] and parts[0] in ('init_v', 'update_vs'):
            out[name] = torch.zeros(shape)
            continue
        noise = _unit_noise(rng, shape)
        if name == 'emb.dist_emb.freq':
            value = math.pi * np.arange(1, shape[0] + 1, dtype=np.float64) + noise * 0.05
        elif 'embedding_list' in name:
            value = noise * 0.5
        elif len(shape) == 2:
            value = noise / math.sqrt(shape[1])
        elif parts[-1] == 'bias':
            value = noise * 0.2
        else:
            value = noise
        out[name] = torch.from_numpy(value.astype(np.float32))
    return out


def state_from_npz(z, cfg):
    """the state_dict the reference ran with, rebuilt; checked against the stored per-tensor sums, which have to match exactly"""
    names = [str(n) for n in z[f'{cfg}/sd_names']]
    shapes = {n: [d for d in row if d >= 0] for n, row in zip(names, z[f'{cfg}/sd_shapes'].tolist())}
    sd = fill_state(shapes, int(z[f'{cfg}/seed']), CONFIGS[cfg].get('output_init') == 'zeros')
    for n, want in zip(names, z[f'{cfg}/sd_sums'].tolist()):
        got = float(sd[n].numpy().astype(np.float64).sum()) + float(np.abs(sd[n].numpy().astype(np.float64)).sum())
        assert got == want, (cfg, n, got, want)
    return sd


def grad_view(t):
    """what the fixture keeps of a gradient: at most GRAD_KEEP elements, evenly strided over the flattened tensor"""
    flat = t.reshape(-1)
    return flat[::max(1, -(-flat.numel() // GRAD_KEEP))]


def run(model, module, z, pos, batch, target, dtype):
    """one forward + backward of the reference; -> everything the fixture keeps of it"""
    rec = {}
    orig = module.xyztodat

    def recording(*a, **k):
        out = orig(*a, **k)
        rec['dist'], rec['angle'], rec['torsion'], rec['i'], rec['j'], rec['idx_kj'], rec['idx_ji'] = (o.detach().clone() for o in out)
        return out

    hook = model.emb.register_forward_hook(lambda m, args, out: rec.update(sbf=out[1].detach().clone(), t=out[2].detach().clone()))
    module.xyztodat = recording
    try:
        data = types.SimpleNamespace(z=torch.from_numpy(z), pos=torch.from_numpy(pos).to(dtype), batch=torch.from_numpy(batch))
        u = model(data)
    finally:
        module.xyztodat = orig
        hook.remove()
    loss = torch.nn.L1Loss()(u, target.to(dtype))
    model.zero_grad()
    loss.backward()
    rec['u'] = u.detach().clone()
    rec['grad'] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return rec


def main():
    G.import_reference()
    register_stand_ins()
    from models import spherical_message_passing as M
    out = {}
    for cfg, kw in CONFIGS.items():
        seed = 100 + ord(cfg)
        while True:
            z, pos, batch = molecules(SIZES[cfg], seed)
            wrap, ang, nbr, low, singles = conditions(pos, SIZES[cfg], kw['cutoff'])
            if wrap > WRAP_MARGIN and ang > ANGLE_MARGIN and nbr <= 32 and low >= 1 and singles >= 1:
                break
            print(cfg, 'seed', seed, 'rejected: wrap margin', wrap, 'angle margin', ang, 'fewest neighbours', low, 'singles', singles)
            seed += 1000
        assert wrap > WRAP_MARGIN and ang > ANGLE_MARGIN and nbr <= 32
        with torch.no_grad():          # dist_emb.reset_parameters writes its Parameter through arange(out=...): refused in grad mode
            model = M.SMP(**kw)
        for q in model.parameters():     # arange(out=freq) under no_grad leaves freq with requires_grad False; in grad mode, where the
            q.requires_grad_(True)       # reference was written to be built, every parameter is trained
        sd = fill_state({k: v.shape for k, v in model.state_dict().items()}, seed, kw.get('output_init') == 'zeros')
        model.load_state_dict(sd, strict=True)
        target = torch.randn(len(SIZES[cfg]), kw['target_dim'], generator=torch.Generator().manual_seed(5))
        model64 = copy.deepcopy(model).double()
        r32 = run(model, M, z, pos, batch, target, torch.float32)
        r64 = run(model64, M, z, pos, batch, target, torch.float64)
        for k in ('i', 'j', 'idx_kj', 'idx_ji'):
            assert torch.equal(r32[k], r64[k]), (cfg, k)
        assert set(r32['grad']) == set(r64['grad'])
        m64 = R.geometry(pos, SIZES[cfg], kw['cutoff'], 1, 1, np.float64)
        assert float(np.abs(r64['torsion'].numpy() - m64['torsion']).max()) < 1e-9 and m64['single'].sum() == singles
        for r, two_pi in ((r32, np.float32(2 * math.pi)), (r64, 2 * math.pi)):
            assert np.all(r['torsion'].numpy()[m64['single']] == two_pi)
        p = f'{cfg}/'
        out[p + 'z'], out[p + 'pos'], out[p + 'sizes'], out[p + 'seed'] = z, pos, np.array(SIZES[cfg]), np.array(seed)
        out[p + 'sd_names'] = np.array(list(sd))
        out[p + 'sd_shapes'] = np.array([(list(v.shape) + [-1, -1])[:2] for v in sd.values()], dtype=np.int64)
        out[p + 'sd_sums'] = np.array([float(v.numpy().astype(np.float64).sum()) + float(np.abs(v.numpy().astype(np.float64)).sum())
                                      for v in sd.values()])
        out[p + 'target'] = target.numpy()
        for k in ('i', 'j', 'idx_kj', 'idx_ji'):
            out[p + k] = r32[k].numpy().astype(np.int32)
        step = BASIS_STEP[cfg]
        for tag, r in (('32', r32), ('64', r64)):
            for k in ('u', 'dist', 'angle', 'torsion'):
                out[f'{p}{k}{tag}'] = r[k].numpy()
            out[f'{p}sbf{tag}'], out[f'{p}t{tag}'] = r['sbf'][::step].numpy(), r['t'][::step].numpy()
            out.update({f'{p}grad{tag}/{k}': grad_view(v).numpy().copy() for k, v in r['grad'].items()})
        out[p + 'grad_names'] = np.array(list(r32['grad']))
        gerr = max(float((r32['grad'][k].double() - v).abs().max() / max(float(v.abs().max()), 1e-30)) for k, v in r64['grad'].items()
                   if float(v.abs().max()) > 0)
        print(cfg, 'seed', seed, 'E', r32['i'].shape[0], 'T', r32['idx_kj'].shape[0], 'wrap margin', wrap, 'angle margin', ang,
              'u', r64['u'].flatten()[:3].tolist(), '|u32 - u64|', float((r32['u'].double() - r64['u']).abs().max()),
              'worst grad rel err of the fp32 run', gerr)
    path = os.path.join(HERE, 'smp.npz')
    np.savez_compressed(path, **out)
    zf = np.load(path)
    for cfg in CONFIGS:
        state_from_npz(zf, cfg)
    size = os.path.getsize(path)
    print('wrote smp.npz', size, 'bytes')
    assert size < 2 ** 20


if __name__ == '__main__':
    main()
