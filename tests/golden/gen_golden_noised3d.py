"""Fixture of the noised-3D negatives (reference configs/old_configs/contrastive_training_noised_3d.yml): the unmodified reference
NoisedDistancesCollate (datasets/custom_collate.py:131-152) and NoisedCoordinatesCollate (:160-185) on four small molecules whose
3D graphs carry edata['w'] (the key both classes noise), ndata['x'] and ndata['feat'], with targets, U = 2 copies, std = 0.2, under
a fixed torch seed -> tests/golden/noised3d.npz (the molecules, the targets and, per collate, the batched 2D and 3D graphs the
reference returned: edges, batch_num_nodes, 'w', 'x', 'feat').

    python tests/golden/gen_golden_noised3d.py          (imports the reference checkout, as gen_golden.py does)

The DGL stand-in (tests/golden/_stubs/dgl) has no all_edges, which NoisedCoordinatesCollate calls: it is DGL's name for edges()
with the default arguments (edge-id order) and is aliased to it from this file.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

STD, NUM_NOISED, SEED = 0.2, 2, 20


def molecules():
    """three seeded synthetic molecules and a two-atom one (a complete graph of two edges)"""
    mols = G.synth.make_dataset(3, seed=57)
    rng = np.random.default_rng(4)
    atom = np.stack([rng.integers(0, d, 2) for d in G.synth.ATOM_FEATURE_DIMS], 1).astype(np.int64)
    bond = np.stack([rng.integers(0, d, 2) for d in G.synth.BOND_FEATURE_DIMS], 1).astype(np.int64)
    mols.insert(2, G.synth.Molecule(2, np.array([0, 1]), np.array([1, 0]), atom, bond,
                                    rng.standard_normal((2, 3)).astype(np.float32)))
    return mols


def items(dgl, mols, targets):
    out = []
    for m, t in zip(mols, targets):
        g = dgl.graph((torch.from_numpy(m.src), torch.from_numpy(m.dst)), num_nodes=m.n_atoms)
        g.ndata['feat'] = torch.from_numpy(m.atom_feat)
        g.edata['feat'] = torch.from_numpy(m.bond_feat)
        s, d = G.synth.complete_graph_edges(m.n_atoms)
        c = dgl.graph((torch.from_numpy(s), torch.from_numpy(d)), num_nodes=m.n_atoms)
        c.ndata['feat'] = torch.from_numpy(m.atom_feat)
        c.ndata['x'] = torch.from_numpy(m.coords.astype(np.float32))
        c.edata['w'] = torch.from_numpy(G.synth.pairwise_distances(m.coords, s, d))
        out.append((g, c, t))
    return out


def main():
    dgl = G.import_reference()[0]
    dgl.DGLGraph.all_edges = dgl.DGLGraph.edges
    sys.modules.setdefault('torch_geometric', types.ModuleType('torch_geometric'))    # custom_collate.py:6 (unused here)
    pkg = types.ModuleType('datasets')                                                 # bypass datasets/__init__.py
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    from datasets.custom_collate import NoisedCoordinatesCollate, NoisedDistancesCollate
    mols = molecules()
    targets = torch.from_numpy(np.random.default_rng(8).standard_normal((len(mols), 3)).astype(np.float32))
    out = G.mols_to_npz(mols)
    out['seed'], out['std'], out['num_noised'], out['targets'] = np.array(SEED), np.array(STD), np.array(NUM_NOISED), targets.numpy()
    for tag, cls in (('distances', NoisedDistancesCollate), ('coordinates', NoisedCoordinatesCollate)):
        its = items(dgl, mols, targets)
        before = [c.edata['w'].clone() for _, c, _ in its]
        torch.manual_seed(SEED)
        (g2,), (g3,), t = cls(STD, NUM_NOISED)(its)
        assert all(torch.equal(b, c.edata['w']) for b, (_, c, _) in zip(before, its))
        out[f'{tag}/targets'] = t.numpy()
        for name, g in (('g2', g2), ('g3', g3)):
            out[f'{tag}/{name}/src'], out[f'{tag}/{name}/dst'] = g._src.numpy(), g._dst.numpy()
            out[f'{tag}/{name}/batch_num_nodes'] = g.batch_num_nodes().numpy()
            out[f'{tag}/{name}/feat'] = g.ndata['feat'].numpy()
        out[f'{tag}/g3/w'], out[f'{tag}/g3/x'] = g3.edata['w'].numpy(), g3.ndata['x'].numpy()
        print(tag, 'nodes', g3.number_of_nodes(), 'edges', g3.number_of_edges(), 'min w', float(g3.edata['w'].min()))
    np.savez_compressed(os.path.join(HERE, 'noised3d.npz'), **out)
    print('wrote noised3d.npz', os.path.getsize(os.path.join(HERE, 'noised3d.npz')), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(4)
    main()
