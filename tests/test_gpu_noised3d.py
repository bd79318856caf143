"""-m gpu: the (1 + U)-fold noised complete-graph batch built on the device (csrc/noised3d.hip through
dataset.noised_complete_graphs_on_device / FlatMolDataset.assemble_noised / BatchStream(noised_3d=...)).

Structure: exactly graph.build_index of graph.batch of 1 + U host copies.  U = 0: bitwise complete_graphs_on_device.  std = 0: every
copy's d bitwise the clean d.  Values: d (and x) against the fp64 host mirror of the noise stream (tests/noise_reference.py) fed the
same seed and step, per element |ours - fp64| <= max(4 err_ref, 2e-6 |fp64|) - the rule of tests/test_gpu_metrics_edges.py - with
err_ref the largest error, over the same array, of a plain fp32 numpy evaluation of the same formulas on the same inputs; every
check prints err, err_ref and the largest ratio err / allowed before it asserts ('Noised-3D negatives', keeps the largest).
Shapes: B = 3 molecules of 1, 2 and 5 atoms (a molecule without edges, one with two), B = 7 molecules of 9-12 atoms (several
workgroups per copy), B = 1 (six atoms, and a single atom: no edge at all), U in {0, 1, 3}, both modes."""
import copy
import importlib

import numpy as np
import pytest
import torch

import noise_reference as NR
from helpers import PNA_SMALL, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STD = 0.2
SIZES = {'b3': (1, 2, 5), 'b7': (9, 12, 10, 11, 9, 12, 10), 'b1': (6,), 'b1_atom': (1,)}
INDEX_FIELDS = ('in_ptr', 'perm', 'src_s', 'dst_s', 'out_ptr', 'out_epos', 'graph_ptr', 'inv_perm')
NET3D_KW = dict(target_dim=8, hidden_dim=10, node_wise_output_layers=0, message_net_layers=1, update_net_layers=1,
                reduce_func='mean', fourier_encodings=4, propagation_depth=1, batch_norm=True, readout_batchnorm=True,
                batch_norm_momentum=0.93, readout_hidden_dim=10, readout_layers=1, readout_aggregators=['min', 'max', 'mean'])


@pytest.fixture(scope='module')
def amd():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return importlib.import_module('3dinfomax_amd')


def _mods():
    return importlib.import_module('3dinfomax_amd.dataset'), importlib.import_module('3dinfomax_amd.graph')


def chain(n, seed):
    """n atoms bonded in a chain, random features, positions a few angstrom apart"""
    rng = np.random.default_rng(seed)
    a = np.arange(n - 1, dtype=np.int64)
    src, dst = np.stack([a, a + 1], 1).ravel(), np.stack([a + 1, a], 1).ravel()
    atom = np.stack([rng.integers(0, d, n) for d in synth.ATOM_FEATURE_DIMS], 1).astype(np.int64)
    bond = np.stack([rng.integers(0, d, src.shape[0]) for d in synth.BOND_FEATURE_DIMS], 1).astype(np.int64).reshape(-1, 3)
    return synth.Molecule(n, src, dst, atom, bond, (1.5 * rng.standard_normal((n, 3))).astype(np.float32))


_CACHE = {}


def molecules(case):
    if case not in _CACHE:
        _CACHE[case] = [chain(n, 100 + 7 * k) for k, n in enumerate(SIZES[case])]
    return _CACHE[case]


def build(mols, U, mode, std=STD, seed=5, step=0):
    dataset, _ = _mods()
    ds = dataset.FlatMolDataset(mols)
    (g2,), (g3,) = ds.assemble_noised(np.arange(len(mols)), DEV, std, U, mode, seed=seed, step=step)
    torch.cuda.synchronize()
    return g2, g3


def clean(mols):
    dataset, _ = _mods()
    (g2,), (g3,) = dataset.FlatMolDataset(mols).assemble(np.arange(len(mols)), DEV)
    torch.cuda.synchronize()
    return g2, g3


def coords_of(mols):
    return np.concatenate([m.coords for m in mols]).astype(np.float32)


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
@pytest.mark.parametrize('U', [0, 1, 3])
@pytest.mark.parametrize('case', list(SIZES))
def test_structure_equals_the_index_of_the_batched_host_copies(amd, case, U, mode):
    _, graph = _mods()
    mols = molecules(case)
    _, g3 = build(mols, U, mode)
    one = amd.batch([amd.complete_graph(m) for m in mols])
    host = amd.batch([one] * (1 + U))
    ref = graph.build_index(*(t.numpy() for t in host.edges()), host.number_of_nodes(), host.batch_num_nodes().numpy())
    assert g3.device.type == 'cuda' and g3.number_of_nodes() == host.number_of_nodes() and g3.number_of_edges() == host.number_of_edges()
    for a, b, name in zip(g3.edges(), host.edges(), ('src', 'dst')):
        assert a.dtype == torch.int64 and torch.equal(a.cpu(), b), name
    assert torch.equal(g3.batch_num_nodes().cpu(), host.batch_num_nodes())
    got = g3.index()
    assert (got.num_nodes, got.num_edges, got.num_graphs) == (ref.num_nodes, ref.num_edges, ref.num_graphs)
    for f in INDEX_FIELDS:
        a, b = getattr(got, f).cpu().numpy(), getattr(ref, f).numpy()
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), f
    assert got.max_in_degree == ref.max_in_degree
    rows, tiles, groups = got.degree_groups()
    assert np.array_equal(rows.cpu().numpy(), ref.deg_rows.numpy()) and tuple(groups) == tuple(ref.deg_groups)
    assert g3.edata['d'].shape == (host.number_of_edges(), 1) and g3.edata['d'].dtype == torch.float32
    assert ('x' in g3.ndata) == (mode == 'coordinates')
    if mode == 'coordinates':
        assert g3.ndata['x'].shape == (host.number_of_nodes(), 3)
    assert g3.ready_event is not None


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
@pytest.mark.parametrize('case', list(SIZES))
def test_no_copies_is_bitwise_the_clean_batch(amd, case, mode):
    mols = molecules(case)
    _, g3 = build(mols, 0, mode)
    _, ref = clean(mols)
    for a, b in zip(g3.edges(), ref.edges()):
        assert torch.equal(a, b)
    for f in INDEX_FIELDS:
        assert torch.equal(getattr(g3.index(), f), getattr(ref.index(), f)), f
    assert g3.index().max_in_degree == ref.index().max_in_degree
    assert torch.equal(g3.edata['d'].view(torch.int32), ref.edata['d'].view(torch.int32))
    assert torch.equal(g3.batch_num_nodes(), ref.batch_num_nodes())
    if mode == 'coordinates':
        assert np.array_equal(g3.ndata['x'].cpu().numpy().view(np.uint32), coords_of(mols).view(np.uint32))


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
@pytest.mark.parametrize('case', ['b3', 'b7', 'b1'])
def test_zero_std_leaves_every_copy_the_clean_distances(amd, case, mode):
    mols = molecules(case)
    U = 3
    _, g3 = build(mols, U, mode, std=0.0)
    _, ref = clean(mols)
    d = g3.edata['d'].view(torch.int32).view(1 + U, -1)
    assert all(torch.equal(d[c], ref.edata['d'].view(torch.int32).view(-1)) for c in range(1 + U))
    if mode == 'coordinates':
        assert np.array_equal(g3.ndata['x'].cpu().numpy(), np.tile(coords_of(mols), (1 + U, 1)))


def check_against_mirror(tag, got, ref64, ref32):
    """per element |got - fp64| <= max(4 err_ref, 2e-6 |fp64|), err_ref = max |fp32 numpy - fp64| over the array"""
    got = np.asarray(got, dtype=np.float64).reshape(ref64.shape)
    err_ref = float(np.abs(ref32.astype(np.float64) - ref64).max()) if ref64.size else 0.0
    err = np.abs(got - ref64)
    allowed = np.maximum(4 * err_ref, 2e-6 * np.abs(ref64))
    ratio = float((err / np.maximum(allowed, 1e-300)).max()) if ref64.size else 0.0
    print(f'{tag}: err {float(err.max()) if err.size else 0.0:.3e} err_ref {err_ref:.3e} largest err / allowed {ratio:.3f}')
    assert np.isfinite(got).all() and (err <= allowed).all(), tag
    return ratio


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
@pytest.mark.parametrize('U', [1, 3])
@pytest.mark.parametrize('case', ['b3', 'b7', 'b1'])
def test_values_match_the_fp64_mirror(amd, case, U, mode):
    mols = molecules(case)
    seed, step = (9 << 32) | 1234, (1 << 33) | 17          # both words of seed and step in use
    _, g3 = build(mols, U, mode, seed=seed, step=step)
    n = [m.n_atoms for m in mols]
    d64, x64 = NR.noised_batch(coords_of(mols), n, STD, U, mode, seed, step)
    d32, x32 = NR.noised_batch(coords_of(mols), n, STD, U, mode, seed, step, dtype=np.float32)
    check_against_mirror(f'{case} U={U} {mode} d', g3.edata['d'].cpu().numpy().ravel(), d64, d32)
    if mode == 'coordinates':
        check_against_mirror(f'{case} U={U} {mode} x', g3.ndata['x'].cpu().numpy(), x64, x32)
        # both directions of a pair see the same positions: d is symmetric bit for bit, and it is the norm of the stored x
        s, t = (e.cpu().numpy() for e in g3.edges())
        d = g3.edata['d'].cpu().numpy().ravel()
        lookup = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(s, t))}
        back = np.array([lookup[(int(b), int(a))] for a, b in zip(s, t)], dtype=np.int64)
        assert np.array_equal(d.view(np.uint32), d[back].view(np.uint32))
        x = g3.ndata['x'].cpu().numpy()
        diff = x[s] - x[t]
        norm = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2])
        assert np.allclose(norm, d, rtol=3e-7, atol=1e-7)          # same fp32 formula, 1 ulp (the host's sqrt is another library's)


def at_origin(mols):
    return [synth.Molecule(m.n_atoms, m.src, m.dst, m.atom_feat, m.bond_feat, np.zeros_like(m.coords)) for m in mols]


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_noise_does_not_depend_on_the_batch_around_it(amd, mode):
    """The noise is a function of (seed, step, copy, element) alone, element = the batch's node id (coordinates mode) or the batch's
    EDGE id (distances mode).  (a) The first three molecules of B = 7 keep their node ids and their edge ids in the sub-batch of
    those three: their noised positions and distances are bitwise the same in both modes, whatever the launch looks like.
    (b) With every atom at the origin the clean distance is 0 and d (x) is the noise term itself: two batches of different
    molecules then agree bitwise on every edge id (node id) they share - the key is the id in the batch, not the molecule."""
    mols = molecules('b7')
    U = 3
    _, full = build(mols, U, mode, seed=21, step=4)
    _, sub = build(mols[:3], U, mode, seed=21, step=4)
    n_sub, e_sub = sub.number_of_nodes() // (1 + U), sub.number_of_edges() // (1 + U)
    d_full = full.edata['d'].view(torch.int32).view(1 + U, -1)[:, :e_sub]
    assert torch.equal(d_full, sub.edata['d'].view(torch.int32).view(1 + U, -1))
    if mode == 'coordinates':
        assert torch.equal(full.ndata['x'].view(torch.int32).view(1 + U, -1, 3)[:, :n_sub], sub.ndata['x'].view(torch.int32).view(1 + U, -1, 3))
    _, a = build(at_origin(mols), U, mode, seed=21, step=4)
    _, b = build(at_origin(mols[3:] + molecules('b3')), U, mode, seed=21, step=4)
    key = 'x' if mode == 'coordinates' else 'd'
    fa, fb = (g.ndata[key] if key == 'x' else g.edata[key] for g in (a, b))
    fa, fb = fa.view(torch.int32).reshape(1 + U, -1), fb.view(torch.int32).reshape(1 + U, -1)
    k = min(fa.shape[1], fb.shape[1])
    assert k >= 50 and torch.equal(fa[:, :k], fb[:, :k])
    assert (fa[0] == 0).all() and (fa[1:] != 0).float().mean().item() > 0.99


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_seed_and_step_change_every_copy_and_leave_the_clean_one(amd, mode):
    mols = molecules('b7')
    U = 3
    _, ref = clean(mols)
    runs = {k: build(mols, U, mode, seed=s, step=t)[1] for k, (s, t) in
            {'base': (3, 0), 'again': (3, 0), 'step': (3, 1), 'seed': (4, 0), 'step_hi': (3, 1 << 32), 'seed_hi': (3 | (1 << 32), 0)}.items()}
    d = {k: g.edata['d'].view(torch.int32).view(1 + U, -1) for k, g in runs.items()}
    assert torch.equal(d['base'], d['again'])
    for k in ('step', 'seed', 'step_hi', 'seed_hi'):
        assert torch.equal(d[k][0], ref.edata['d'].view(torch.int32).view(-1)), k
        for c in range(1, 1 + U):
            assert (d[k][c] != d['base'][c]).float().mean().item() > 0.99, (k, c)
    for c in range(1, 1 + U):                       # the copies differ from each other and from the clean batch
        assert (d['base'][c] != d['base'][0]).float().mean().item() > 0.99
        assert all((d['base'][c] != d['base'][o]).float().mean().item() > 0.99 for o in range(1, c))


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_net3d_and_the_extra_negatives_loss_on_the_device_built_batch(amd, mode):
    _, graph = _mods()
    mols = molecules('b7')
    B, U = len(mols), 3
    g2, g3 = build(mols, U, mode, seed=8, step=2)
    torch.manual_seed(0)
    net = amd.Net3D(node_dim=0, edge_dim=1, **NET3D_KW)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith('linear.weight'):
                p.mul_(p.shape[1] * 0.7)
    # the same batch rebuilt on the host from the device batch's own tensors
    src, dst = (t.cpu() for t in g3.edges())
    host = graph.BatchedMolGraph(src, dst, g3.number_of_nodes(), g3.batch_num_nodes().cpu(), edata={'d': g3.edata['d'].cpu()})
    assert host._index is None
    host = host.to(DEV)                                 # build_index on the host, then the upload
    cot = torch.randn((1 + U) * B, NET3D_KW['target_dim'], generator=torch.Generator().manual_seed(1)).to(DEV)
    outs = []
    for g in (g3, host):
        m = copy.deepcopy(net).to(DEV).train()
        z = m(g.local_copy())
        (z * cot).sum().backward()
        torch.cuda.synchronize()
        outs.append((z.detach(), {k: p.grad for k, p in m.named_parameters()}, dict(m.named_buffers())))
    (z_dev, grad_dev, buf_dev), (z_host, grad_host, buf_host) = outs
    assert z_dev.shape == ((1 + U) * B, NET3D_KW['target_dim']) and torch.isfinite(z_dev).all()
    assert torch.equal(z_dev, z_host)
    for k in grad_host:
        assert grad_dev[k] is not None and torch.equal(grad_dev[k], grad_host[k]), k
    for k in buf_host:
        assert torch.equal(buf_dev[k], buf_host[k]), k
    # the loss the batch is for: PNA embeddings of the B molecules against the (1 + U) B rows of z2
    torch.manual_seed(2)
    pna = amd.PNA(avg_d=1.0, device=DEV, **PNA_SMALL).to(DEV).train()
    m = copy.deepcopy(net).to(DEV).train()
    z1, z2 = pna(g2), m(g3.local_copy())
    assert z1.shape == (B, 8) and z2.shape == ((1 + U) * B, 8)
    loss = amd.NTXentExtraNegatives(tau=0.1, extra_negatives_weight=50)(z1, z2)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and torch.isfinite(loss).item()
    for model in (pna, m):
        for k, p in model.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), k


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_batch_stream_through_the_prefetcher_equals_assemble_noised(amd, mode):
    dataset, _ = _mods()
    mols = synth.make_dataset(40, seed=13)
    ds = dataset.FlatMolDataset(mols)
    opts = {'std': STD, 'num_noised': 2, 'mode': mode}
    stream = dataset.BatchStream(ds, 16, steps=3, seed=6, noised_3d=opts)
    loader = torch.utils.data.DataLoader(stream, batch_size=None, num_workers=0, pin_memory=True)
    with dataset.DevicePrefetcher(loader, DEV) as batches:
        got = list(batches)
    assert len(got) == 3
    for i, ((g2,), (g3,)) in enumerate(got):
        epoch, k = divmod(i, stream.per_epoch)
        ids = np.random.default_rng(6 + epoch).permutation(len(ds))[k * 16:(k + 1) * 16]
        (r2,), (r3,) = ds.assemble_noised(ids, DEV, STD, 2, mode, seed=6, step=i)
        torch.cuda.synchronize()
        assert g3.batch_size == 3 * 16 and torch.equal(g3.batch_num_nodes(), r3.batch_num_nodes())
        for a, b in zip((*g2.edges(), *g3.edges()), (*r2.edges(), *r3.edges())):
            assert torch.equal(a, b)
        for f in INDEX_FIELDS:
            assert torch.equal(getattr(g3.index(), f), getattr(r3.index(), f)), f
        assert torch.equal(g3.edata['d'].view(torch.int32), r3.edata['d'].view(torch.int32))
        assert set(g3.ndata) == set(r3.ndata) and all(torch.equal(g3.ndata[k], r3.ndata[k]) for k in r3.ndata)
