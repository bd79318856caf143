"""Fixture of the EGNN 3D encoder (reference models/egnn.py): the unmodified reference EGNN on seeded synthetic molecules, forward +
loss + backward -> tests/golden/egnn.npz (molecules with their coordinates, input features, state_dict, output, final node features,
loss, every parameter's gradient, the buffers after the step, and the fp32 reference's own error against an fp64 run of itself).

    python tests/golden/gen_golden_egnn.py          (imports the reference checkout, as gen_golden.py does)

Four configurations at hidden_dim 16, propagation_depth 3, dropout 0, on five QM9-like molecules plus one QMugs-like molecule above 64
atoms and one single-atom molecule (no edges), each as a complete graph with ndata['x']: 'a' random float features of width 5,
batch_norm, sum reduce, readout min / max / mean (configs/0.yml), readout_hidden_dim 10, target_dim 8; 'b' batch_norm=False, mean
reduce, readout sum / mean; 'ones' node_dim 1 with constant-ones features (the input of configs/0.yml) and batch_norm; 'd' as 'a' in
eval mode after one training step (SGD, lr 1e-4).  The loss is the mean of the squared outputs.

'ones' feeds the first BatchNorm a constant column: mean = value, variance 0, output = the BatchNorm bias - if the mean is exact.
torch's fp32 sum of 164 equal floats is not (a few ulp off), and 1 / sqrt(eps) = 316 makes that an error of 9e-5 of the layer's
output in the reference's own fp32 run (against 3e-15 in its fp64 run), 4e-5 at the model output: a fixture that far from its own
fp64 run would say nothing at the 1e-5 the running statistics are compared at.  So the weight and bias of `input`'s Linear are
rounded to multiples of 1/64 for 'ones': x W^T + b and every partial sum of the column are then exact in fp32 in any order, torch's
mean is the value and its variance 0, as the kernels' row-shifted statistics give them (csrc/bn.hip).  models/egnn.py is not touched.

ref_err of a gradient = max |fp32 - fp64| / max(max |fp64|, 1e-4 x the largest gradient of the set): analytically-zero gradients (a
bias in front of a BatchNorm) are rounding noise on both sides and would otherwise give a meaningless ratio.

The DGL stand-in of tests/golden/_stubs covers everything models/egnn.py touches (apply_nodes, update_all with fn.sum / fn.mean and
an apply function, edges.src / edges.dst, readout_nodes): nothing is registered here.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_gin as GG  # noqa: E402

BASE = dict(edge_dim=1, hidden_dim=16, propagation_depth=3, dropout=0.0, target_dim=8, readout_hidden_dim=10)
CONFIGS = {
    'a': dict(BASE, node_dim=5, batch_norm=True, reduce_func='sum', readout_aggregators=['min', 'max', 'mean']),
    'b': dict(BASE, node_dim=5, batch_norm=False, reduce_func='mean', readout_aggregators=['sum', 'mean']),
    'ones': dict(BASE, node_dim=1, batch_norm=True, reduce_func='sum', readout_aggregators=['min', 'max', 'mean']),
    'd': dict(BASE, node_dim=5, batch_norm=True, reduce_func='sum', readout_aggregators=['min', 'max', 'mean']),
}
SEEDS = {'a': 71, 'b': 72, 'ones': 73, 'd': 71}


def features(cfg, n_atoms):
    if cfg == 'ones':
        return torch.ones(n_atoms, 1)
    return torch.randn(n_atoms, CONFIGS[cfg]['node_dim'], generator=torch.Generator().manual_seed(SEEDS[cfg] + 1000))


def graph_of(dgl, mols, feat, dtype=torch.float32):
    gs, a0 = [], 0
    for m in mols:
        s, d = G.synth.complete_graph_edges(m.n_atoms)
        g = dgl.graph((torch.from_numpy(s), torch.from_numpy(d)), num_nodes=m.n_atoms)
        g.ndata['feat'] = feat[a0:a0 + m.n_atoms].to(dtype)
        g.ndata['x'] = torch.from_numpy(np.ascontiguousarray(m.coords, dtype=np.float32)).to(dtype)
        a0 += m.n_atoms
        gs.append(g)
    return dgl.batch(gs)


def make_trained_like(model, seed):
    """gen_golden.make_trained_like (O(1) pre-BatchNorm scale, BatchNorm affine away from 1 / 0, non-zero biases) and a soft-edge gate
    that is neither saturated nor flat"""
    G.make_trained_like(model, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for layer in model.mp_layers:
            lin = layer.soft_edge_network
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / np.sqrt(lin.weight.shape[1]))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.2)


def exact_constant_column(model):
    """'ones': the parameters of `input`'s Linear as multiples of 1/64 (see the module docstring)"""
    lin = model.input.fully_connected[0].linear
    with torch.no_grad():
        lin.weight.copy_(torch.round(lin.weight * 64) / 64)
        lin.bias.copy_(torch.round(lin.bias * 64) / 64)


def run(model, bg):
    """-> output, final node features, loss (after backward)"""
    y = model(bg)
    loss = (y ** 2).mean()
    model.zero_grad()
    loss.backward()
    return y.detach(), bg.ndata['feat'].detach(), loss.detach()


def main():
    dgl = G.import_reference()[0]
    from models.egnn import EGNN
    out = {}
    for cfg, kw in CONFIGS.items():
        mols = GG.molecules(SEEDS[cfg])
        feat = features(cfg, sum(m.n_atoms for m in mols))
        torch.manual_seed(7)
        model = EGNN(**kw)
        make_trained_like(model, 23 + ord(cfg[0]) if cfg != 'd' else 23 + ord('a'))
        if cfg == 'ones':
            exact_constant_column(model)
        model.train()
        if cfg == 'd':      # one training step, then everything in eval mode
            opt = torch.optim.SGD(model.parameters(), lr=1e-4)
            run(model, graph_of(dgl, mols, feat))
            opt.step()
            model.eval()
        p = f'{cfg}/'
        out.update(G.mols_to_npz(mols, prefix=p + 'mol'))
        out[p + 'feat_in'] = feat.numpy()
        out.update(G.sd_np(model, p + 'sd'))
        ref64 = copy.deepcopy(model).double()
        y, nodes, loss = run(model, graph_of(dgl, mols, feat))
        out[p + 'out'], out[p + 'feat'], out[p + 'loss'] = y.numpy(), nodes.numpy(), np.array(loss.item())
        out.update({f'{p}grad/{k}': q.grad.numpy().copy() for k, q in model.named_parameters()})
        out.update({f'{p}buf_after/{k}': v.numpy().copy() for k, v in model.named_buffers()})
        y64, nodes64, _ = run(ref64, graph_of(dgl, mols, feat, torch.float64))
        out[p + 'ref_err/out'] = np.array(GG.rel_err(y, y64))
        out[p + 'ref_err/feat'] = np.array(GG.rel_err(nodes, nodes64))
        g64 = dict(ref64.named_parameters())
        scale = max(float(q.grad.abs().max()) for q in g64.values())
        worst = 0.0
        for k, q in model.named_parameters():
            e = float((q.grad.double() - g64[k].grad).abs().max() / max(float(g64[k].grad.abs().max()), 1e-4 * scale))
            out[f'{p}ref_err/grad/{k}'] = np.array(e)
            worst = max(worst, e)
        print(cfg, 'atoms', [m.n_atoms for m in mols], 'loss', loss.item(), 'ref_err out', float(out[p + 'ref_err/out']),
              'feat', float(out[p + 'ref_err/feat']), 'worst grad ref_err', worst)
    path = os.path.join(HERE, 'egnn.npz')
    np.savez_compressed(path, **out)
    print('wrote egnn.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(4)
    main()
