"""DistancePredictor / pairwise_distance_collate on the host: the reference's parameter layout, collate semantics, plugin surface and
the options the fused path refuses (fixture: tests/golden/gen_golden_distance.py)."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load, mols_from_npz, sd_from_npz, synth

import gen_golden_distance as GD

dp = importlib.import_module('3dinfomax_amd.distance_predictor')
launcher = importlib.import_module('launch_reference')


@pytest.mark.parametrize('cfg', sorted(GD.CONFIGS))
def test_state_dict_matches_reference_and_loads_strict(cfg):
    z = load('distance_predictor.npz')
    ref = sd_from_npz(z, f'{cfg}/sd')
    torch.manual_seed(0)
    model = amd.DistancePredictor(pna_args=dict(GD.PNA_ARGS), **GD.CONFIGS[cfg])
    sd = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_transformer_parameters_follow_torch_init_and_seed_order():
    kw = dict(GD.CONFIGS['a'])
    torch.manual_seed(3)
    a = amd.DistancePredictor(pna_args=dict(GD.PNA_ARGS), **kw)
    torch.manual_seed(3)
    b = amd.DistancePredictor(pna_args=dict(GD.PNA_ARGS), **kw)
    assert isinstance(a.transformer_layer, torch.nn.TransformerEncoderLayer)
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k


@pytest.mark.parametrize('cfg', sorted(GD.CONFIGS))
def test_pairwise_distance_collate_matches_reference(cfg):
    z = load('distance_predictor.npz')
    mols = mols_from_npz(z, f'{cfg}/mol')
    items = []
    for m in mols:
        s, d = synth.complete_graph_edges(m.n_atoms)
        items.append((amd.bond_graph(m), torch.stack([torch.from_numpy(s), torch.from_numpy(d)]),
                      torch.from_numpy(synth.pairwise_distances(m.coords, s, d))))
    before = [it[1].clone() for it in items]
    (g, pidx, mask), dist = amd.pairwise_distance_collate(items)
    assert pidx.dtype == torch.int64 and mask.dtype == torch.bool
    np.testing.assert_array_equal(pidx.numpy(), z[f'{cfg}/pidx'])
    np.testing.assert_array_equal(mask.numpy(), z[f'{cfg}/mask'])
    np.testing.assert_array_equal(dist.numpy(), z[f'{cfg}/dist'])
    assert g.number_of_nodes() == sum(m.n_atoms for m in mols)
    for it, b in zip(items, before):          # the items are not shifted in place
        assert torch.equal(it[1], b)


def test_pair_index_is_the_complete_graph_index():
    mols = synth.make_dataset(3, seed=2)
    items = []
    for m in mols:
        s, d = synth.complete_graph_edges(m.n_atoms)
        items.append((amd.bond_graph(m), torch.stack([torch.from_numpy(s), torch.from_numpy(d)]),
                      torch.from_numpy(synth.pairwise_distances(m.coords, s, d))))
    (g, pidx, _), _ = amd.pairwise_distance_collate(items)
    idx = dp.pair_index(pidx, g)
    ref = amd.batch([amd.complete_graph(m) for m in mols]).index()
    for name in ('in_ptr', 'perm', 'src_s', 'dst_s', 'out_ptr', 'out_epos', 'graph_ptr', 'inv_perm'):
        assert torch.equal(getattr(idx, name), getattr(ref, name)), name
    assert dp.pair_index(pidx, g) is idx


def test_plugin_names_bind_distance_predictor_and_collate():
    names = launcher.plugin_names()
    assert names['DistancePredictor'] is amd.DistancePredictor
    assert names['pairwise_distance_collate'] is amd.pairwise_distance_collate


@pytest.mark.parametrize('kw, exc, word', [
    (dict(transformer_layer=True, distance_net=True, projection_dim=0, pna_dropout=0.1), NotImplementedError, 'dropout'),
    (dict(transformer_layer=True, distance_net=True, projection_dim=0, activation='gelu'), NotImplementedError, 'activation'),
    (dict(transformer_layer=True, distance_net=False, projection_dim=3), ValueError, 'projection_dim'),
    (dict(transformer_layer=True, distance_net=True, projection_dim=0, nhead=1), NotImplementedError, 'nhead'),
    (dict(transformer_layer=True, distance_net=True, projection_dim=0, nhead=3), ValueError, 'nhead'),
    (dict(transformer_layer=False, distance_net=True, projection_dim=0, projection_layers=2), ValueError, 'projection_layers'),
])
def test_refusals_name_their_option(kw, exc, word):
    kw = dict(kw)
    pna_args = dict(GD.PNA_ARGS, hidden_dim=200 if kw.get('nhead') == 1 else 16, dropout=kw.pop('pna_dropout', 0.0))
    with pytest.raises(exc, match=word):
        amd.DistancePredictor(target_dim=1, pna_args=pna_args, **kw)


def test_transformer_dropout_zero_and_relu_are_accepted():
    m = amd.DistancePredictor(target_dim=1, pna_args=dict(GD.PNA_ARGS), distance_net=True, projection_dim=0, nhead=2,
                              activation=torch.nn.functional.relu)
    assert m.transformer_layer.dropout.p == 0.0
