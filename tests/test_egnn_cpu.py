"""EGNN on the host: the reference's parameter layout, the refused options, the plugin surface, the coordinates on the complete graph
and the C ABI of the gate-and-reduce kernels (fixture: tests/golden/gen_golden_egnn.py)."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load, mols_from_npz, sd_from_npz, synth

import gen_golden_egnn as GE

egnn = importlib.import_module('3dinfomax_amd.egnn')
L = importlib.import_module('3dinfomax_amd._lib')
alias = importlib.import_module('infomax3d_amd')
launcher = importlib.import_module('launch_reference')

SMALL = dict(node_dim=3, edge_dim=1, hidden_dim=8, target_dim=2, readout_aggregators=['sum'], propagation_depth=1)


@pytest.mark.parametrize('cfg', sorted(GE.CONFIGS))
def test_state_dict_matches_reference_and_loads_strict(cfg):
    z = load('egnn.npz')
    ref = sd_from_npz(z, f'{cfg}/sd')
    torch.manual_seed(0)
    model = amd.EGNN(avg_d=1.0, device='cpu', **GE.CONFIGS[cfg])          # unknown kwargs are swallowed (train.py passes both)
    sd = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k
    top = {k.split('.')[0] for k in sd}
    assert top == {'input', 'mp_layers', 'node_wise_output_network', 'output'}
    for l in range(3):
        for part in ('message_network', 'update_network', 'soft_edge_network'):
            assert any(k.startswith(f'mp_layers.{l}.{part}.') for k in sd), (l, part)


@pytest.mark.parametrize('kw, exc, word', [
    (dict(fourier_encodings=4), NotImplementedError, 'fourier_encodings'),
    (dict(reduce_func='max'), ValueError, 'reduce'),
    (dict(readout_aggregators=['sum', 'std']), ValueError, 'readout_aggregators'),
    (dict(readout_aggregators=[]), ValueError, 'readout_aggregators'),
    (dict(node_dim=0), ValueError, 'node_dim'),
])
def test_refusals_name_their_argument(kw, exc, word):
    with pytest.raises(exc, match=word):
        amd.EGNN(**dict(SMALL, **kw))


def test_node_dim_refusal_says_what_the_reference_does():
    with pytest.raises(ValueError, match=r"train\.py.*ndata\['feat'\]|ndata\['feat'\].*train\.py"):
        amd.EGNN(**dict(SMALL, node_dim=0))


def test_missing_coordinates_are_refused_by_name():
    mol = synth.make_dataset(1, seed=1)[0]
    model = amd.EGNN(**SMALL)
    for g in (amd.complete_graph(mol), ):
        g.ndata['feat'] = torch.zeros(mol.n_atoms, 3)
        with pytest.raises(ValueError, match=r"ndata\['x'\]"):
            egnn._coordinates(g)
        with pytest.raises(ValueError, match=r"ndata\['x'\]"):
            with torch.no_grad():
                model(g)
    g = amd.complete_graph(mol, coordinates=True)
    g.ndata['x'] = g.ndata['x'][:, :2]
    with pytest.raises(ValueError, match=r"ndata\['x'\].*\[N, 3\]"):
        egnn._coordinates(g)


def test_complete_graph_carries_coordinates_on_request_only():
    mol = synth.make_dataset(3, seed=5)[2]
    plain, with_x = amd.complete_graph(mol), amd.complete_graph(mol, coordinates=True)
    assert sorted(plain.ndata) == ['feat'] and sorted(plain.edata) == ['d']
    assert sorted(with_x.ndata) == ['feat', 'x'] and sorted(with_x.edata) == ['d']
    x = with_x.ndata['x']
    assert x.dtype == torch.float32 and tuple(x.shape) == (mol.n_atoms, 3)
    np.testing.assert_array_equal(x.numpy(), mol.coords.astype(np.float32))
    for k in ('feat',):
        assert torch.equal(plain.ndata[k], with_x.ndata[k])
    assert torch.equal(plain.edata['d'], with_x.edata['d'])
    assert torch.equal(plain.edges()[0], with_x.edges()[0]) and torch.equal(plain.edges()[1], with_x.edges()[1])
    other = mol.coords[::-1].copy()
    moved = amd.complete_graph(mol, coords=other, coordinates=True)
    np.testing.assert_array_equal(moved.ndata['x'].numpy(), other.astype(np.float32))
    batched = amd.batch([with_x, moved])
    assert tuple(batched.ndata['x'].shape) == (2 * mol.n_atoms, 3)


def test_exported_by_the_package_the_alias_and_the_launcher():
    names = launcher.plugin_names()
    for name in ('EGNN', 'EGCLayer'):
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(amd, name) is getattr(egnn, name)
        assert getattr(alias, name) is getattr(egnn, name)
        assert names[name] is getattr(egnn, name)
    assert amd.egnn is egnn
    assert egnn.EGCLayer.fused_gate_reduce is True


def test_gate_reduce_entry_points_are_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_gate_reduce_fwd', 'i3d_gate_reduce_bwd', 'i3d_gate_reduce_max_feat'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_abi_version() == 2
    assert lib.i3d_gate_reduce_max_feat() == 512


def test_invalid_sizes_are_refused_and_uncovered_widths_are_not_taken_before_any_launch():
    lib = L.load()
    for n, e, h in ((0, 0, 16), (4, -1, 16), (4, 0, 0)):
        assert lib.i3d_gate_reduce_fwd(None, None, None, None, None, n, e, h, 0, None, None, None) == -1
        assert b'invalid argument' in lib.i3d_last_error()
        assert lib.i3d_gate_reduce_bwd(None, None, None, None, None, n, e, h, 0, None, None, None, None) == -1
    for h in (6, 2, 513, 516, 1024):      # valid, but not the kernels': the caller composes the step
        assert lib.i3d_gate_reduce_fwd(None, None, None, None, None, 4, 3, h, 0, None, None, None) == L.NOT_TAKEN == 1
        assert lib.i3d_gate_reduce_bwd(None, None, None, None, None, 4, 3, h, 1, None, None, None, None) == L.NOT_TAKEN
    for h in (4, 20, 128, 512):           # a covered width goes on to the pointer checks
        assert lib.i3d_gate_reduce_fwd(None, None, None, None, None, 4, 3, h, 0, None, None, None) == -1
        assert b'null' in lib.i3d_last_error()
        assert lib.i3d_gate_reduce_bwd(None, None, None, None, None, 4, 3, h, 0, None, None, None, None) == -1


def test_fixture_holds_what_the_gpu_tests_read():
    z = load('egnn.npz')
    for cfg, kw in GE.CONFIGS.items():
        mols = mols_from_npz(z, f'{cfg}/mol')
        assert len(mols) == 7 and any(m.n_atoms > 64 for m in mols) and any(m.n_atoms == 1 for m in mols)
        n = sum(m.n_atoms for m in mols)
        assert z[f'{cfg}/feat_in'].shape == (n, kw['node_dim']) and z[f'{cfg}/feat'].shape == (n, 16)
        assert z[f'{cfg}/out'].shape == (7, 8)
        grads = [k for k in z.files if k.startswith(f'{cfg}/grad/')]
        assert len(grads) == len([k for k in z.files if k.startswith(f'{cfg}/sd/') and 'running' not in k and 'tracked' not in k])
        assert all(f'{cfg}/ref_err/grad/' + k.split('/grad/')[1] in z.files for k in grads)
        if kw['batch_norm']:      # BatchNorm affine parameters away from 1 / 0
            g = z[f'{cfg}/sd/mp_layers.0.message_network.fully_connected.0.batch_norm.weight']
            assert np.abs(g - 1).max() > 0.05
    assert np.all(z['ones/feat_in'] == 1.0)
    assert int(z['d/buf_after/input.fully_connected.0.batch_norm.num_batches_tracked']) == 1      # eval mode: the one training step
    assert int(z['a/buf_after/input.fully_connected.0.batch_norm.num_batches_tracked']) == 1
