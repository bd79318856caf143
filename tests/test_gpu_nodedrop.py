"""-m gpu: the node-dropped views of the GraphCL baseline built on the device (csrc/nodedrop.hip through
dataset.nodedrop_to_device) - exactly the reference's views (tests/golden/node_drop.npz) and exactly the host path
(BatchedMolGraph.remove_nodes + graph.build_index) on edge cases - and the GraphCL training step on them against the reference's
(PNA on view 1 then view 2 in train mode, NTXent, one backward)."""
import importlib

import numpy as np
import pytest
import torch

from helpers import PNA_SMALL, close, grads_close, load, mols_from_npz, rel_err, sd_from_npz, synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def amd():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return importlib.import_module('3dinfomax_amd')


def _mods():
    return importlib.import_module('3dinfomax_amd.dataset'), importlib.import_module('3dinfomax_amd.graph')


def fixture_removed(z, v):
    counts = z[f'removed{v}_count']
    return [np.asarray(r) for r in np.split(z[f'removed{v}'], np.cumsum(counts)[:-1])]


def device_views(mols, removed=None, drop_ratio=0.2, rng=None):
    dataset, _ = _mods()
    ds = dataset.FlatMolDataset(mols)
    hb = ds.assemble_nodedrop_host(np.arange(len(mols)), drop_ratio, rng=rng, removed=removed)
    (g1,), (g2,) = dataset.nodedrop_to_device(hb, DEV)
    return (g1, g2), hb


def host_view(amd, mols, removed):
    _, graph = _mods()
    g = amd.batch([amd.bond_graph(m).remove_nodes(r) for m, r in zip(mols, removed)])
    return g, graph.build_index(*(t.numpy() for t in g.edges()), g.number_of_nodes(), g.batch_num_nodes().numpy())


INDEX_FIELDS = ('in_ptr', 'perm', 'src_s', 'dst_s', 'out_ptr', 'out_epos', 'graph_ptr', 'inv_perm', 'deg_rows', 'deg_tile_group')


def assert_index_equal(got, ref, what):
    assert (got.num_nodes, got.num_edges, got.num_graphs) == (ref.num_nodes, ref.num_edges, ref.num_graphs), what
    for f in INDEX_FIELDS:
        a, b = getattr(got, f).cpu().numpy(), getattr(ref, f).numpy()
        assert a.shape == b.shape and np.array_equal(a, b), f'{what}: {f}'
    assert got.max_in_degree == ref.max_in_degree, what
    assert tuple(got.deg_groups) == tuple(ref.deg_groups), what


def assert_view_equal(gd, gh, idx, what):
    assert gd.number_of_nodes() == gh.number_of_nodes() and gd.number_of_edges() == gh.number_of_edges(), what
    for a, b, name in ((gd.edges()[0], gh.edges()[0], 'src'), (gd.edges()[1], gh.edges()[1], 'dst'),
                       (gd.ndata['feat'], gh.ndata['feat'], 'atom_feat'), (gd.edata['feat'], gh.edata['feat'], 'bond_feat'),
                       (gd.batch_num_nodes(), gh.batch_num_nodes(), 'batch_num_nodes')):
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), f'{what}: {name}'
    assert_index_equal(gd.index(), idx, what)


def test_device_views_equal_the_reference_views_exactly(amd):
    _, graph = _mods()
    z = load('node_drop.npz')
    mols = mols_from_npz(z)
    removed = [fixture_removed(z, 1), fixture_removed(z, 2)]
    (g1, g2), _ = device_views(mols, removed)
    torch.cuda.synchronize()
    for tag, g in (('view1', g1), ('view2', g2)):
        assert g.device.type == 'cuda'
        s, d = g.edges()
        assert np.array_equal(s.cpu().numpy(), z[f'{tag}/src']) and np.array_equal(d.cpu().numpy(), z[f'{tag}/dst']), tag
        assert np.array_equal(g.ndata['feat'].cpu().numpy(), z[f'{tag}/atom_feat']), tag
        assert np.array_equal(g.edata['feat'].cpu().numpy(), z[f'{tag}/bond_feat']), tag
        assert np.array_equal(g.batch_num_nodes().numpy(), z[f'{tag}/batch_num_nodes']), tag
        bnn = z[f'{tag}/batch_num_nodes']
        assert_index_equal(g.index(), graph.build_index(z[f'{tag}/src'], z[f'{tag}/dst'], int(bnn.sum()), bnn), tag)


def _star(n_leaves=4):
    src = [x for k in range(1, n_leaves + 1) for x in (0, k)]
    dst = [x for k in range(1, n_leaves + 1) for x in (k, 0)]
    return _mol(n_leaves + 1, src, dst, 1)


def _mol(n, src, dst, seed):
    rng = np.random.default_rng(seed)
    src, dst = np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
    atom = np.stack([rng.integers(0, d, n) for d in synth.ATOM_FEATURE_DIMS], 1).astype(np.int64)
    bond = np.stack([rng.integers(0, d, src.shape[0]) for d in synth.BOND_FEATURE_DIMS], 1).astype(np.int64)
    return synth.Molecule(n, src, dst, atom, bond, np.zeros((n, 3), np.float32))


def _edge_case(name):
    """(molecules, removal sets of both views, or None for drawn ones)"""
    rng = np.random.default_rng(11)
    if name == 'no_edges':             # view 1 keeps one atom per molecule: E' = 0
        mols = synth.make_dataset(6, seed=1)
        return mols, ([np.arange(1, m.n_atoms) for m in mols], [rng.choice(m.n_atoms, m.n_atoms // 3, replace=False) for m in mols])
    if name == 'one_atom':             # one-atom molecules, some of them removed whole in view 2
        mols = [_mol(1, [], [], k) for k in range(5)] + synth.make_dataset(3, seed=2) + [_mol(1, [], [], 9)]
        none = [np.zeros(0, np.int64)] * len(mols)
        v2 = [np.array([0]) if m.n_atoms == 1 and k % 2 == 0 else np.zeros(0, np.int64) for k, m in enumerate(mols)]
        return mols, (none, v2)
    if name == 'vanishing_group':      # the star's centre is the only node of in-degree 4: its group disappears in view 1
        mols = [_mol(3, [0, 1, 1, 2], [1, 0, 2, 1], 3), _star(), _mol(2, [0, 1], [1, 0], 4)]
        return mols, ([np.zeros(0, np.int64), np.array([0]), np.zeros(0, np.int64)], [np.zeros(0, np.int64), np.array([2]), np.array([1])])
    if name == 'large':                # molecules above one wave's chunk of nodes and of edges (64)
        big = [m for m in (synth.qmugs_like(rng) for _ in range(400)) if m.n_atoms > 90][:4]
        assert len(big) == 4 and all(m.src.shape[0] > 128 for m in big)
        mols = synth.make_dataset(3, seed=5) + big[:2] + synth.make_dataset(2, seed=6) + big[2:]
        return mols, None
    if name == 'b4096':
        return synth.make_dataset(4096, seed=8), None
    raise KeyError(name)


@pytest.mark.parametrize('case', ['no_edges', 'one_atom', 'vanishing_group', 'large', 'b4096'])
def test_device_views_equal_the_host_path(amd, case):
    dataset, _ = _mods()
    mols, removed = _edge_case(case)
    views, hb = device_views(mols, removed, rng=np.random.default_rng(5))
    removed = dataset.node_drop_removed(hb)
    torch.cuda.synchronize()
    if case == 'no_edges':
        assert views[0].number_of_edges() == 0
    if case == 'vanishing_group':
        assert 4 in [D for D, _, _ in host_view(amd, mols, [np.zeros(0, np.int64)] * 3)[1].deg_groups]
        assert 4 not in [D for D, _, _ in views[0].index().deg_groups]
    for v in range(2):
        gh, idx = host_view(amd, mols, removed[v])
        assert_view_equal(views[v], gh, idx, f'{case} view {v + 1}')


def _all_arrays(views):
    out = []
    for g in views:
        idx = g.index()
        out += [*g.edges(), g.ndata['feat'], g.edata['feat']] + [getattr(idx, f) for f in INDEX_FIELDS]
    return [t.cpu() for t in out]


def test_build_is_bit_deterministic_and_does_not_synchronise(amd):
    dataset, _ = _mods()
    mols = synth.make_dataset(500, seed=12, kind='qmugs')
    ds = dataset.FlatMolDataset(mols)
    hb = ds.assemble_nodedrop_host(np.arange(500), 0.2, rng=np.random.default_rng(3))
    first = dataset.nodedrop_to_device(hb, DEV)
    torch.cuda.synchronize()
    a = _all_arrays([first[0][0], first[1][0]])
    torch.cuda.set_sync_debug_mode('error')
    try:
        second = dataset.nodedrop_to_device(hb, DEV)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    b = _all_arrays([second[0][0], second[1][0]])
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    removed = dataset.node_drop_removed(hb)
    for v, g in enumerate((second[0][0], second[1][0])):
        gh, idx = host_view(amd, mols, removed[v])
        assert_view_equal(g, gh, idx, f'qmugs b500 view {v + 1}')


def test_batch_stream_node_drop_end_to_end(amd):
    dataset, _ = _mods()
    mols = synth.make_dataset(300, seed=13)
    ds = dataset.FlatMolDataset(mols)
    stream = dataset.BatchStream(ds, 128, steps=3, seed=4, node_drop=0.2)
    loader = torch.utils.data.DataLoader(stream, batch_size=None, num_workers=0, pin_memory=True)
    for i, hb in enumerate(loader):
        (g1,), (g2,) = dataset.BatchStream.to_device(hb, DEV)
        epoch, k = divmod(i, stream.per_epoch)
        ids = np.random.default_rng(4 + epoch).permutation(len(ds))[k * 128:(k + 1) * 128]
        batch_mols = [mols[j] for j in ids]
        removed = dataset.node_drop_removed(hb)
        assert all(len(r) == int(0.2 * m.n_atoms) for v in range(2) for r, m in zip(removed[v], batch_mols))
        torch.cuda.synchronize()
        for v, g in enumerate((g1, g2)):
            gh, idx = host_view(amd, batch_mols, removed[v])
            assert_view_equal(g, gh, idx, f'batch {i} view {v + 1}')


def graphcl_step(amd, z, views):
    pna = amd.PNA(avg_d=1.0, device=DEV, **PNA_SMALL)
    pna.load_state_dict(sd_from_npz(z, 'sd'), strict=True)
    pna.cuda().train()
    g1, g2 = (g.local_copy() for g in views)
    pred = pna(g1)                     # GraphCLTrainer.forward_pass: model(*view1), model(*view2), loss(pred, target)
    targ = pna(g2)
    loss = amd.NTXent(tau=0.1)(pred, targ)
    loss.backward()
    return pna, pred, targ, loss, g1, g2


def test_graphcl_step_vs_reference_fixture(amd):
    z = load('node_drop.npz')
    mols = mols_from_npz(z)
    (g1, g2), _ = device_views(mols, [fixture_removed(z, 1), fixture_removed(z, 2)])
    pna, pred, targ, loss, a, b = graphcl_step(amd, z, (g1, g2))
    assert rel_err(pred.detach().cpu(), z['out1']) < TOL
    assert rel_err(targ.detach().cpu(), z['out2']) < TOL
    assert rel_err(a.ndata['feat'].detach().cpu(), z['feat1']) < TOL
    assert rel_err(b.ndata['feat'].detach().cpu(), z['feat2']) < TOL
    assert rel_err(torch.tensor([loss.item()]), torch.tensor([float(z['loss'])])) < TOL
    grads_close({k: p.grad for k, p in pna.named_parameters()}, sd_from_npz(z, 'grad'), 5e-4, 'graphcl ')
    sd = pna.state_dict()
    for k, v in sd_from_npz(z, 'buf_after').items():
        assert close(sd[k], v, TOL, 1e-6), k                         # running statistics after two train-mode forwards


def test_graphcl_steps_repeat_bit_identically(amd):
    z = load('node_drop.npz')
    mols = mols_from_npz(z)
    (g1, g2), _ = device_views(mols, [fixture_removed(z, 1), fixture_removed(z, 2)])
    runs = []
    for _ in range(2):
        pna, pred, targ, loss, _, _ = graphcl_step(amd, z, (g1, g2))
        runs.append([pred.detach(), targ.detach(), loss.detach()] + [p.grad for _, p in pna.named_parameters()]
                    + [v for _, v in pna.named_buffers()])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*runs))
