"""Fixture of GeoMol's message-passing network on OGB features (reference models/geomol_mpnn_ogb_feat.py, models/geomol_mpnn.py): the
unmodified reference GeomolGNNWrapperOGBFeat on seeded synthetic molecules, forward + loss + backward -> tests/golden/geomol.npz
(molecules, state_dict, output, final node and edge representations, loss, every parameter's gradient, the buffers after the step,
and the fp32 reference's own error against an fp64 run of itself).

    python tests/golden/gen_golden_geomol.py          (imports the reference checkout, as gen_golden.py does)

Four configurations on the molecules of gen_golden_gin.molecules() (five QM9-like molecules, one QMugs-like molecule above 64 atoms,
one single atom without edges): 'a' hidden_dim 16, depth 3, n_layers 2, target_dim 3 (loss: mean of the outputs squared); 'b'
hidden_dim 50 (the width of configs/geomolgnn_wrapper_ogb_feat.yml), target_dim 1, L1 loss; 'c' hidden_dim 13, depth 1, n_layers 1,
no readout BatchNorm, L1 loss; 'd' as 'a' in eval mode after one training step (SGD, lr 1e-3).

Weights are trained-like: Linear weights randn / sqrt(fan_in), biases 0.2 randn, random BatchNorm affine, edge_eps 0.15 and node_eps
-0.25 (the reference's zeros would hide both residual paths).

ref_err of a gradient = max |fp32 - fp64| / max(max |fp64|, 1e-4 x the largest gradient of the set), the convention of
gen_golden_gin.py.

The reference imports two functions of libraries that are absent here; their stand-ins are registered below, written from the
libraries' documented semantics:
  torch_geometric.nn.global_mean_pool(x, batch)              per-graph mean of the node rows: index_add over `batch`, divided by the
                                                             node counts
  torch_scatter.scatter_sum(src, index, dim=0, dim_size=n)   out[index[i]] += src[i] along dim 0: index_add into zeros [n, ...]
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_gin as GG  # noqa: E402

CONFIGS = {
    'a': dict(hidden_dim=16, target_dim=3, depth=3, n_layers=2, readout_layers=2, readout_batchnorm=True),
    'b': dict(hidden_dim=50, target_dim=1, depth=3, n_layers=2, readout_layers=2, readout_batchnorm=True),
    'c': dict(hidden_dim=13, target_dim=3, depth=1, n_layers=1, readout_layers=2, readout_batchnorm=False),
    'd': dict(hidden_dim=16, target_dim=3, depth=3, n_layers=2, readout_layers=2, readout_batchnorm=True),
}
SEEDS = {'a': 71, 'b': 72, 'c': 73, 'd': 71}
EDGE_EPS, NODE_EPS = 0.15, -0.25


def register_stand_ins():
    def global_mean_pool(x, batch, size=None):
        n = int(batch.max()) + 1 if size is None else size
        sums = torch.zeros(n, x.shape[1], dtype=x.dtype).index_add(0, batch, x)
        counts = torch.zeros(n, dtype=x.dtype).index_add(0, batch, torch.ones(batch.shape[0], dtype=x.dtype))
        return sums / counts.clamp(min=1)[:, None]

    def scatter_sum(src, index, dim=0, out=None, dim_size=None):
        assert dim == 0 and out is None
        n = int(index.max()) + 1 if dim_size is None else dim_size
        return torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add(0, index, src)

    tg = types.ModuleType('torch_geometric')
    tg_nn = types.ModuleType('torch_geometric.nn')
    tg_nn.global_mean_pool = global_mean_pool
    tg.nn = tg_nn
    sys.modules['torch_geometric'], sys.modules['torch_geometric.nn'] = tg, tg_nn
    ts = types.ModuleType('torch_scatter')
    ts.scatter_sum = scatter_sum
    sys.modules['torch_scatter'] = ts


def make_trained_like(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / np.sqrt(m.weight.shape[1]))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            elif isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1 + torch.randn(m.weight.shape, generator=g) * 0.2)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
        model.node_gnn.update.edge_eps.fill_(EDGE_EPS)
        model.node_gnn.update.node_eps.fill_(NODE_EPS)


def data_of(mols):
    """the PyG-style batch the reference's forward reads: z, edge_index, edge_attr, batch"""
    off, src, dst, batch = 0, [], [], []
    for b, m in enumerate(mols):
        src.append(m.src + off)
        dst.append(m.dst + off)
        batch.append(np.full(m.n_atoms, b, np.int64))
        off += m.n_atoms
    return types.SimpleNamespace(z=torch.from_numpy(np.concatenate([m.atom_feat for m in mols])),
                                 edge_index=torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)])),
                                 edge_attr=torch.from_numpy(np.concatenate([m.bond_feat for m in mols])),
                                 batch=torch.from_numpy(np.concatenate(batch)))


def loss_of(cfg, y, target):
    return (y ** 2).mean() if cfg in ('a', 'd') else torch.nn.L1Loss()(y, target.to(y.dtype))


def run(model, data, cfg, target):
    """-> output, node representation, edge representation, loss (after backward)"""
    feat = []
    hook = model.node_gnn.register_forward_hook(lambda mod, args, out: feat.append([t.detach().clone() for t in out]))
    y = model(data)
    hook.remove()
    loss = loss_of(cfg, y, target)
    model.zero_grad()
    loss.backward()
    return y.detach(), feat[0][0], feat[0][1], loss.detach()


def main():
    G.import_reference()
    register_stand_ins()
    from models.geomol_mpnn_ogb_feat import GeomolGNNWrapperOGBFeat
    out = {}
    for cfg, kw in CONFIGS.items():
        mols = GG.molecules(SEEDS[cfg])
        data = data_of(mols)
        torch.manual_seed(7)
        model = GeomolGNNWrapperOGBFeat(**kw)
        make_trained_like(model, 23 + ord(cfg if cfg != 'd' else 'a'))
        target = torch.randn(len(mols), kw['target_dim'], generator=torch.Generator().manual_seed(5))
        model.train()
        if cfg == 'd':      # one training step, then everything in eval mode
            opt = torch.optim.SGD(model.parameters(), lr=1e-3)
            run(model, data, cfg, target)
            opt.step()
            model.eval()
        p = f'{cfg}/'
        out.update(G.mols_to_npz(mols, prefix=p + 'mol'))
        out.update(G.sd_np(model, p + 'sd'))
        out[p + 'target'] = target.numpy()
        ref64 = copy.deepcopy(model).double()
        y, feat, efeat, loss = run(model, data, cfg, target)
        out[p + 'out'], out[p + 'feat'], out[p + 'efeat'], out[p + 'loss'] = y.numpy(), feat.numpy(), efeat.numpy(), np.array(loss.item())
        missing = [k for k, q in model.named_parameters() if q.grad is None]
        assert not missing, missing
        out.update({f'{p}grad/{k}': q.grad.numpy().copy() for k, q in model.named_parameters()})
        out.update({f'{p}buf_after/{k}': v.numpy().copy() for k, v in model.named_buffers()})
        y64, feat64, efeat64, _ = run(ref64, data, cfg, target)
        out[p + 'ref_err/out'] = np.array(GG.rel_err(y, y64))
        out[p + 'ref_err/feat'] = np.array(GG.rel_err(feat, feat64))
        out[p + 'ref_err/efeat'] = np.array(GG.rel_err(efeat, efeat64))
        g64 = dict(ref64.named_parameters())
        scale = max(float(q.grad.abs().max()) for q in g64.values())
        worst = 0.0
        for k, q in model.named_parameters():
            e = float((q.grad.double() - g64[k].grad).abs().max() / max(float(g64[k].grad.abs().max()), 1e-4 * scale))
            out[f'{p}ref_err/grad/{k}'] = np.array(e)
            worst = max(worst, e)
        print(cfg, 'atoms', [m.n_atoms for m in mols], 'loss', loss.item(), 'ref_err out', float(out[p + 'ref_err/out']), 'feat',
              float(out[p + 'ref_err/feat']), 'efeat', float(out[p + 'ref_err/efeat']), 'worst grad ref_err', worst)
    path = os.path.join(HERE, 'geomol.npz')
    np.savez_compressed(path, **out)
    print('wrote geomol.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
