"""CPU tests of the noised-3D negatives: NoisedDistancesCollate / NoisedCoordinatesCollate against the reference's own batches
(tests/golden/noised3d.npz, tests/golden/gen_golden_noised3d.py), the host mirror of the device builder's noise stream
(tests/noise_reference.py: known-answer vector, moments) and the host-side refusals of the device path."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import noise_reference as NR
from helpers import load, mols_from_npz, synth

amd = importlib.import_module('3dinfomax_amd')
dataset = importlib.import_module('3dinfomax_amd.dataset')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLATES = {'distances': 'NoisedDistancesCollate', 'coordinates': 'NoisedCoordinatesCollate'}


def fixture_items(z, key='w', with_targets=True, with_x=True):
    items = []
    for m, t in zip(mols_from_npz(z), z['targets']):
        g3 = amd.complete_graph(m, coordinates=with_x)
        g3.edata = {key: g3.edata['d']}
        item = (amd.bond_graph(m), g3)
        items.append(item + (torch.from_numpy(t.copy()),) if with_targets else item)
    return items


def snapshot(items):
    return [[t.clone() for g in item[:2] for t in (*g.edges(), *g.ndata.values(), *g.edata.values())] for item in items]


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_collate_reproduces_the_reference_batch_bit_for_bit(mode):
    z = load('noised3d.npz')
    items = fixture_items(z)
    before = snapshot(items)
    torch.manual_seed(int(z['seed']))
    (g2,), (g3,), targets = getattr(amd, COLLATES[mode])(float(z['std']), int(z['num_noised']))(items)
    for name, g in (('g2', g2), ('g3', g3)):
        assert np.array_equal(g.edges()[0].numpy(), z[f'{mode}/{name}/src']), name
        assert np.array_equal(g.edges()[1].numpy(), z[f'{mode}/{name}/dst']), name
        assert np.array_equal(g.batch_num_nodes().numpy(), z[f'{mode}/{name}/batch_num_nodes']), name
        assert np.array_equal(g.ndata['feat'].numpy(), z[f'{mode}/{name}/feat']), name
    w, x = g3.edata['w'].numpy(), g3.ndata['x'].numpy()
    assert w.dtype == np.float32 and w.shape == z[f'{mode}/g3/w'].shape and np.array_equal(w.view(np.uint32), z[f'{mode}/g3/w'].view(np.uint32))
    assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), z[f'{mode}/g3/x'].view(np.uint32))
    assert targets.dtype == torch.float32 and np.array_equal(targets.numpy(), z[f'{mode}/targets'])
    # copy-major: graph c B + i is molecule i of copy c, copy 0 the clean batch
    B, U = len(items), int(z['num_noised'])
    assert g3.batch_size == (1 + U) * B and torch.equal(g3.batch_num_nodes(), g2.batch_num_nodes().repeat(1 + U))
    clean = amd.batch([it[1] for it in items])
    E, N = clean.number_of_edges(), clean.number_of_nodes()
    assert torch.equal(g3.edata['w'][:E], clean.edata['w']) and torch.equal(g3.ndata['x'][:N], clean.ndata['x'])
    assert not torch.equal(g3.edata['w'][E:2 * E], clean.edata['w'])
    # the items are left as they were
    assert all(torch.equal(a, b) for s0, s1 in zip(before, snapshot(items)) for a, b in zip(s0, s1))


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_collate_without_targets_returns_two_fields(mode):
    z = load('noised3d.npz')
    out = getattr(amd, COLLATES[mode])(0.2, 1)(fixture_items(z, with_targets=False))
    assert len(out) == 2 and out[1][0].batch_size == 2 * len(z['targets'])


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_collate_noises_w_when_present_else_d(mode):
    z = load('noised3d.npz')
    cls = getattr(amd, COLLATES[mode])
    runs = {}
    for key in ('w', 'd'):
        torch.manual_seed(3)
        (_,), (g3,), _ = cls(0.2, 2)(fixture_items(z, key=key))
        assert set(g3.edata) == {key}
        runs[key] = g3.edata[key]
    assert torch.equal(runs['w'], runs['d'])
    # both present: 'w' is the one that is noised, 'd' rides along unchanged
    items = fixture_items(z, key='w')
    for it in items:
        it[1].edata['d'] = it[1].edata['w'].clone()
    torch.manual_seed(3)
    (_,), (g3,), _ = cls(0.2, 2)(items)
    E = g3.number_of_edges() // 3
    assert torch.equal(g3.edata['w'], runs['w']) and torch.equal(g3.edata['d'], g3.edata['d'][:E].repeat(3, 1))
    # neither: refused by name
    for it in items:
        it[1].edata = {'feat': it[1].edata['w']}
    with pytest.raises(KeyError, match=COLLATES[mode]):
        cls(0.2, 2)(items)


def test_coordinates_collate_refuses_graphs_without_positions():
    z = load('noised3d.npz')
    for U in (0, 2):
        with pytest.raises(ValueError, match=r"ndata\['x'\].*complete_graph\(mol, coordinates=True\)"):
            amd.NoisedCoordinatesCollate(0.2, U)(fixture_items(z, with_x=False))
    amd.NoisedDistancesCollate(0.2, 2)(fixture_items(z, with_x=False))        # the distances collate does not need them


@pytest.mark.parametrize('mode', ['distances', 'coordinates'])
def test_no_copies_equals_contrastive_collate(mode):
    z = load('noised3d.npz')
    items = fixture_items(z, key='d')
    got = getattr(amd, COLLATES[mode])(0.2, 0)(items)
    ref = amd.contrastive_collate(items)
    assert len(got) == len(ref) == 3 and torch.equal(got[2], ref[2])
    for (a,), (b,) in zip(got[:2], ref[:2]):
        assert torch.equal(a.edges()[0], b.edges()[0]) and torch.equal(a.edges()[1], b.edges()[1])
        assert torch.equal(a.batch_num_nodes(), b.batch_num_nodes())
        assert set(a.ndata) == set(b.ndata) and all(torch.equal(a.ndata[k], b.ndata[k]) for k in b.ndata)
        assert set(a.edata) == set(b.edata) and all(torch.equal(a.edata[k], b.edata[k]) for k in b.edata)


def test_launcher_binds_the_noising_collates():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import launch_reference
    names = launch_reference.plugin_names()
    assert names['NoisedDistancesCollate'] is amd.NoisedDistancesCollate
    assert names['NoisedCoordinatesCollate'] is amd.NoisedCoordinatesCollate


# ---- the host mirror of the device builder's noise -------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's published vectors for philox4x32-10: counter and key all zero, all ones, and the digits of pi"""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for counter, key, want in kat:
        assert tuple(int(x) for x in NR.philox4x32_10(counter, key)) == want
    # vectorised evaluation = element by element; (seed, step) words land where the rule says
    el = np.array([0, 1, 77, 2 ** 32 - 1])
    w = NR.words(el, 3, seed=(5 << 32) | 9, step=(7 << 32) | 11)
    for i, e in enumerate(el):
        assert np.array_equal(w[i], NR.philox4x32_10((int(e), 3, 11, 7), (9, 5)))


def test_mirror_is_stable_and_uniforms_are_fp32_values_in_the_half_open_unit_interval():
    a, wa = NR.normals(np.arange(5000), 2, seed=12, step=34)
    b, wb = NR.normals(np.arange(5000), 2, seed=12, step=34)
    assert a.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(wa, wb)
    u = NR.uniform(np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xfffffeff, 0xffffffff], dtype=np.uint32))
    assert u.dtype == np.float32 and u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert (u > 0).all() and (u <= 1).all() and u[-1] == 1.0          # 2^24 - 0.5 rounds to 2^24 in fp32
    assert np.isfinite(NR.normals(np.arange(4), 1, 0, 0)[0]).all()


def test_mirror_normals_have_the_moments_of_a_standard_normal():
    """2 10^5 normals, seed fixed: mean, variance, third and fourth moment within 5 standard errors of 0, 1, 0, 3 (standard errors of
    the sample moments of a standard normal about the known mean 0: sqrt(1 / n), sqrt(2 / n), sqrt(15 / n), sqrt(96 / n)); the
    (z0, z1), copy-to-copy and step-to-step sample correlations within 5 standard errors (sqrt(1 / pairs)) of 0."""
    n = 200000
    z, _ = NR.normals(np.arange(n // 3 + 1), 1, seed=2026, step=0)
    z = z.ravel()[:n]
    for name, got, want, se in (('mean', z.mean(), 0.0, np.sqrt(1 / n)), ('variance', (z * z).mean(), 1.0, np.sqrt(2 / n)),
                                ('third', (z ** 3).mean(), 0.0, np.sqrt(15 / n)), ('fourth', (z ** 4).mean(), 3.0, np.sqrt(96 / n))):
        print(f'{name}: {got:.5f} want {want} se {se:.5f} -> {(got - want) / se:+.2f} se')
        assert abs(got - want) <= 5 * se, name
    pairs = n // 2
    el = np.arange(pairs)
    base, _ = NR.normals(el, 1, seed=2026, step=0)
    other_copy, _ = NR.normals(el, 2, seed=2026, step=0)
    other_step, _ = NR.normals(el, 1, seed=2026, step=1)
    other_seed, _ = NR.normals(el, 1, seed=2027, step=0)
    for name, a, b in (('z0 z1', base[:, 0], base[:, 1]), ('z0 z2', base[:, 0], base[:, 2]), ('copy', base[:, 0], other_copy[:, 0]),
                       ('step', base[:, 0], other_step[:, 0]), ('seed', base[:, 0], other_seed[:, 0]),
                       ('neighbour', base[:-1, 0], base[1:, 0])):
        r = float(np.corrcoef(a, b)[0, 1])
        print(f'correlation {name}: {r:+.5f} ({r * np.sqrt(a.shape[0]):+.2f} se)')
        assert abs(r) <= 5 / np.sqrt(a.shape[0]), name


# ---- the device path's host side ---------------------------------------------------------------------------------------------
def test_batch_stream_refuses_noised_3d_with_node_drop_and_bad_options():
    ds = dataset.FlatMolDataset(synth.make_dataset(8, seed=1))
    with pytest.raises(ValueError, match='noised_3d and node_drop are mutually exclusive'):
        dataset.BatchStream(ds, 4, steps=2, node_drop=0.2, noised_3d={'std': 0.2, 'num_noised': 2})
    with pytest.raises(ValueError, match='mode'):
        dataset.BatchStream(ds, 4, steps=2, noised_3d={'std': 0.2, 'num_noised': 2, 'mode': 'angles'})
    with pytest.raises(ValueError, match='unknown keys'):
        dataset.BatchStream(ds, 4, steps=2, noised_3d={'std': 0.2, 'num_noised': 2, 'sigma': 1})


def test_batch_stream_host_half_is_the_plain_one_plus_the_options():
    ds = dataset.FlatMolDataset(synth.make_dataset(20, seed=2))
    plain = dataset.BatchStream(ds, 6, steps=5, seed=7)
    noised = dataset.BatchStream(ds, 6, steps=5, seed=7, noised_3d={'std': 0.2, 'num_noised': 10})
    for i in range(5):
        a, b = plain[i], noised[i]
        assert b['noised_3d'] == {'std': 0.2, 'num_noised': 10, 'mode': 'distances', 'seed': 7, 'step': i}
        assert set(b) == set(a) | {'noised_3d'} and torch.equal(a['buf'], b['buf']) and a['layout'] == b['layout']


def test_builder_refuses_a_total_beyond_int32_by_name():
    """argument validation happens on the host before any launch: no GPU needed"""
    L = importlib.import_module('3dinfomax_amd._lib')
    lib = L.load()
    args = [None] * 12
    assert lib.i3d_noised_graph_build(None, None, None, 500, 20000, 300_000_000, 10, 0, 0.2, 0, 0, *args) == -1
    assert b'does not fit the int32 index arrays' in lib.i3d_last_error()
    assert lib.i3d_noised_graph_build(None, None, None, 500, 1 << 30, 0, 1, 0, 0.2, 0, 0, *args) == -1
    assert b'does not fit the int32 index arrays' in lib.i3d_last_error()
    assert lib.i3d_noised_graph_build(None, None, None, 4, 40, 300, 2, 2, 0.2, 0, 0, *args) == -1
    assert b'mode' in lib.i3d_last_error()
    assert lib.i3d_noised_graph_build(None, None, None, 4, 40, 300, 2, 1, 0.2, 0, 0, *args) == -1
    assert b'x_out' in lib.i3d_last_error()
    with pytest.raises(ValueError, match='does not fit the int32 index arrays'):
        n = np.full(500, 700, dtype=np.int64)
        dataset.noised_complete_graphs_on_device(torch.zeros(int(n.sum()), 3), None, n, torch.from_numpy(n), 0.2, 10, 'distances', 0, 0)
