"""CPU tests of the GraphCL baseline's node drop: NodeDropCollate against the reference's own views
(tests/golden/node_drop.npz, tests/golden/gen_golden_nodedrop.py), BatchedMolGraph.remove_nodes, the host half of the device
fast path (FlatMolDataset.assemble_nodedrop_host) and the launcher binding."""
import copy
import importlib
import os
import sys

import numpy as np
import torch

from helpers import load, mols_from_npz, synth

amd = importlib.import_module('3dinfomax_amd')
graph = importlib.import_module('3dinfomax_amd.graph')
dataset = importlib.import_module('3dinfomax_amd.dataset')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_removed(z, v):
    """the removal sets the reference's collate drew for view v (1 or 2), one tensor per molecule"""
    counts = z[f'removed{v}_count']
    return [torch.from_numpy(r) for r in np.split(z[f'removed{v}'], np.cumsum(counts)[:-1])]


def host_view(mols, removed):
    """the host path: every molecule's bond graph, remove_nodes, batch, build_index"""
    g = amd.batch([amd.bond_graph(m).remove_nodes(r) for m, r in zip(mols, removed)])
    return g, graph.build_index(*(t.numpy() for t in g.edges()), g.number_of_nodes(), g.batch_num_nodes().numpy())


def test_collate_reproduces_reference_views_and_leaves_items_unmodified():
    z = load('node_drop.npz')
    mols = mols_from_npz(z)
    # tuple items with an extra field, as a dataset with more required_data yields them
    items = [(amd.bond_graph(m), torch.tensor(float(i))) for i, m in enumerate(mols)]
    before = copy.deepcopy([(g.edges(), dict(g.ndata), dict(g.edata), g.batch_num_nodes(), g.number_of_nodes()) for g, _ in items])
    torch.manual_seed(int(z['seed']))
    (v1,), (v2,) = amd.NodeDropCollate(float(z['drop_ratio']))(items)
    for tag, g in (('view1', v1), ('view2', v2)):
        s, d = g.edges()
        assert np.array_equal(s.numpy(), z[f'{tag}/src']) and np.array_equal(d.numpy(), z[f'{tag}/dst']), tag
        assert np.array_equal(g.ndata['feat'].numpy(), z[f'{tag}/atom_feat']), tag
        assert np.array_equal(g.edata['feat'].numpy(), z[f'{tag}/bond_feat']), tag
        assert np.array_equal(g.batch_num_nodes().numpy(), z[f'{tag}/batch_num_nodes']), tag
        assert g.number_of_nodes() == int(z[f'{tag}/batch_num_nodes'].sum())
    for (g, _), (edges, nd, ed, bnn, n) in zip(items, before):
        assert g.number_of_nodes() == n and torch.equal(g.batch_num_nodes(), bnn)
        assert torch.equal(g.edges()[0], edges[0]) and torch.equal(g.edges()[1], edges[1])
        assert all(torch.equal(g.ndata[k], v) for k, v in nd.items()) and all(torch.equal(g.edata[k], v) for k, v in ed.items())


def test_drop_count_is_the_truncated_float64_product():
    rng = np.random.default_rng(0)
    n = 100
    src = rng.integers(0, n, 300)
    g = amd.BatchedMolGraph(torch.from_numpy(src), torch.from_numpy(rng.integers(0, n, 300)), n,
                            ndata={'feat': torch.zeros(n, 9, dtype=torch.long)}, edata={'feat': torch.zeros(300, 3, dtype=torch.long)})
    (v1,), (v2,) = amd.NodeDropCollate(0.29)([(g,)])
    assert v1.number_of_nodes() == v2.number_of_nodes() == 100 - 28
    (v1,), _ = amd.NodeDropCollate(0.2)([(amd.BatchedMolGraph(torch.tensor([0, 1]), torch.tensor([1, 0]), 4),)])
    assert v1.number_of_nodes() == 4                                    # int(0.2 * 4) == 0
    ds = dataset.FlatMolDataset([synth.Molecule(n, src, src, np.zeros((n, 9), np.int64), np.zeros((300, 3), np.int64),
                                                np.zeros((n, 3), np.float32))])
    hb = ds.assemble_nodedrop_host([0], 0.29, rng=np.random.default_rng(1))
    assert [int(v['dims'][0]) for v in hb['node_drop']] == [72, 72]


def test_remove_nodes_commutes_with_batching():
    rng = np.random.default_rng(3)
    mols = synth.make_dataset(9, seed=5) + synth.make_dataset(3, seed=6, kind='qmugs')
    gs = [amd.bond_graph(m) for m in mols]
    removed = [rng.choice(m.n_atoms, size=rng.integers(0, m.n_atoms), replace=False) for m in mols]
    removed[2] = np.arange(mols[2].n_atoms)                              # every node of a molecule
    offs = np.cumsum([0] + [m.n_atoms for m in mols])[:-1]
    a = amd.batch([g.remove_nodes(r) for g, r in zip(gs, removed)])
    b = amd.batch(gs).remove_nodes(np.concatenate([r + o for r, o in zip(removed, offs)]))
    for x, y in zip(a.edges() + (a.ndata['feat'], a.edata['feat'], a.batch_num_nodes()),
                    b.edges() + (b.ndata['feat'], b.edata['feat'], b.batch_num_nodes())):
        assert torch.equal(x, y)
    assert a.number_of_nodes() == b.number_of_nodes()
    assert b.batch_num_nodes().tolist() == [m.n_atoms - len(r) for m, r in zip(mols, removed)]
    # DGL's semantics directly: kept nodes renumbered ascending, kept edges in their order
    g = gs[0]
    r = np.array([1, 4])
    h = g.remove_nodes(r)
    keep = np.setdiff1d(np.arange(g.number_of_nodes()), r)
    s, d = g.edges()
    ek = np.isin(s.numpy(), keep) & np.isin(d.numpy(), keep)
    assert np.array_equal(h.edges()[0].numpy(), np.searchsorted(keep, s.numpy()[ek]))
    assert np.array_equal(h.edges()[1].numpy(), np.searchsorted(keep, d.numpy()[ek]))
    assert np.array_equal(h.edata['feat'].numpy(), g.edata['feat'].numpy()[ek])
    assert np.array_equal(h.ndata['feat'].numpy(), g.ndata['feat'].numpy()[keep])
    assert g.number_of_nodes() == mols[0].n_atoms                        # the input is untouched


def _check_host_half(mols, hb, removed):
    B = len(mols)
    for v, view in enumerate(hb['node_drop']):
        g, idx = host_view(mols, removed[v])
        N2, E2 = (int(x) for x in view['dims'])
        assert (N2, E2) == (g.number_of_nodes(), g.number_of_edges())
        assert np.array_equal(view['n'].numpy(), g.batch_num_nodes().numpy())
        assert tuple(view['groups']) == idx.deg_groups
        assert int(view['max_indeg']) == idx.max_in_degree
        assert int(view['rows']) == idx.deg_rows.shape[0]
        lay = {name: (o, c) for name, o, c in hb['layout']}
        o, c = lay['v32']
        v32 = hb['buf'].numpy()[o:o + 4 * c].view(np.int32)
        gp2, ep2, deg_base, pad_range, tiles = (v32[a:b] for a, b in view['cuts'])
        assert np.array_equal(gp2, idx.graph_ptr.numpy())
        s = g.edges()[0].numpy()
        mol_of_edge = np.searchsorted(gp2, s, side='right') - 1
        assert np.array_equal(ep2, np.concatenate([[0], np.cumsum(np.bincount(mol_of_edge, minlength=B))]))
        assert np.array_equal(tiles, idx.deg_tile_group.numpy())
        # deg_base: where each molecule's first node of every in-degree lands in deg_rows
        rows = idx.deg_rows.numpy()
        indeg = np.diff(idx.in_ptr.numpy())
        stride = int(hb['deg_stride'])
        for D, start, count in idx.deg_groups:
            ids = rows[start:start + count]
            mol = np.searchsorted(gp2, ids, side='right') - 1
            first = {int(m): start + int(np.nonzero(mol == m)[0][0]) for m in np.unique(mol)}
            for m, slot in first.items():
                assert deg_base.reshape(B, stride)[m, D] == slot, (v, m, D)
            assert (indeg[ids] == D).all()
        assert sorted(map(tuple, pad_range.reshape(-1, 2).tolist())) == sorted(
            (s_ + c_, s_ + (c_ + 63) // 64 * 64) for _, s_, c_ in idx.deg_groups)


def test_host_half_matches_build_index_on_host_dropped_graphs():
    z = load('node_drop.npz')
    mols = mols_from_npz(z)
    removed = [fixture_removed(z, 1), fixture_removed(z, 2)]
    ds = dataset.FlatMolDataset(mols)
    hb = ds.assemble_nodedrop_host(np.arange(len(mols)), removed=removed)
    _check_host_half(mols, hb, removed)
    for v in range(2):
        assert all(np.array_equal(np.sort(a), np.sort(b.numpy())) for a, b in zip(dataset.node_drop_removed(hb)[v], removed[v]))
    # drawn removal sets, a shuffled batch of drug-sized molecules
    mols = synth.make_dataset(40, seed=2, kind='qmugs')
    ds = dataset.FlatMolDataset(mols)
    ids = np.random.default_rng(0).permutation(40)[:25]
    hb = ds.assemble_nodedrop_host(ids, 0.2, rng=np.random.default_rng(7))
    _check_host_half([mols[i] for i in ids], hb, dataset.node_drop_removed(hb))


def test_drawn_removal_sets_have_exactly_the_truncated_count():
    mols = synth.make_dataset(60, seed=4) + synth.make_dataset(10, seed=4, kind='qmugs')
    ds = dataset.FlatMolDataset(mols)
    n = np.array([m.n_atoms for m in mols])
    stream = dataset.BatchStream(ds, 30, steps=40, seed=3, node_drop=0.3)
    seen = set()
    for i in range(len(stream)):
        hb = stream[i]
        epoch, k = divmod(i, stream.per_epoch)
        ids = np.random.default_rng(3 + epoch).permutation(len(ds))[k * 30:(k + 1) * 30]
        for v, sets in enumerate(dataset.node_drop_removed(hb)):
            assert [len(r) for r in sets] == [int(0.3 * x) for x in n[ids]]
            assert all(len(np.unique(r)) == len(r) and (r < x).all() for r, x in zip(sets, n[ids]))
            seen.add(tuple(np.concatenate(sets).tolist()))
    assert len(seen) == 2 * len(stream)                                  # every batch and view draws afresh


def test_launcher_binds_node_drop_collate():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import launch_reference
    names = launch_reference.plugin_names()
    assert names['NodeDropCollate'] is amd.NodeDropCollate
