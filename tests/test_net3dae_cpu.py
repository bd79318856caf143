"""Net3DAE / NTXentAE / contrastive_vae_collate on the host: the reference's parameter layout and collate semantics (fixture:
tests/golden/gen_golden_net3dae.py), the reference's node_wise_* quirk, the options refused by name, the plugin surface and the C ABI
of the fused pair head."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load, mols_from_npz, sd_from_npz, synth

import gen_golden_net3dae as GA

L = importlib.import_module('3dinfomax_amd._lib')
net3d_ae = importlib.import_module('3dinfomax_amd.net3d_ae')
launcher = importlib.import_module('launch_reference')


def _items(mols, as_dgl=False):
    items = []
    for m in mols:
        s, d = synth.complete_graph_edges(m.n_atoms)
        dist = torch.from_numpy(synth.pairwise_distances(m.coords, s, d))
        g2, g3 = amd.bond_graph(m), amd.complete_graph(m)
        if as_dgl:
            g2, g3 = _StubDGL(g2), _StubDGL(g3)
        items.append((g2, g3, torch.stack([torch.from_numpy(s), torch.from_numpy(d)]), dist))
    return items


class _StubDGL:
    """the slice of dgl.DGLGraph the collates touch (graph.as_batched_graph)"""

    def __init__(self, g):
        self._g = g
        self.ndata, self.edata = dict(g.ndata), dict(g.edata)

    def edges(self):
        return self._g.edges()

    def number_of_nodes(self):
        return self._g.number_of_nodes()

    def batch_num_nodes(self):
        return self._g.batch_num_nodes()


@pytest.mark.parametrize('cfg', sorted(GA.CONFIGS))
def test_collate_matches_reference_and_leaves_the_items_alone(cfg):
    z = load('net3dae.npz')
    mols = mols_from_npz(z, f'{cfg}/mol')
    items = _items(mols)
    before = [(it[2].clone(), it[3].clone()) for it in items]
    out = amd.contrastive_vae_collate(items)
    assert len(out) == 3 and len(out[0]) == 1 and len(out[1]) == 2
    (g2,), (g3, pidx), dist = out
    assert pidx.dtype == torch.int64
    np.testing.assert_array_equal(pidx.numpy(), z[f'{cfg}/pidx'])
    np.testing.assert_array_equal(dist.numpy(), z[f'{cfg}/dist'])
    assert g2.number_of_nodes() == g3.number_of_nodes() == sum(m.n_atoms for m in mols)
    assert g3.number_of_edges() == pidx.shape[1]
    s3, d3 = g3.edges()
    assert torch.equal(torch.stack([s3, d3]), pidx)          # the pairs are the complete graph's edges, in its order
    for it, (p, d) in zip(items, before):
        assert torch.equal(it[2], p) and torch.equal(it[3], d)


def test_collate_takes_dgl_like_items():
    z = load('net3dae.npz')
    mols = mols_from_npz(z, 'a/mol')
    (a2,), (a3, ap), ad = amd.contrastive_vae_collate(_items(mols))
    (b2,), (b3, bp), bd = amd.contrastive_vae_collate(_items(mols, as_dgl=True))
    assert torch.equal(ap, bp) and torch.equal(ad, bd)
    for ga, gb in ((a2, b2), (a3, b3)):
        assert all(torch.equal(x, y) for x, y in zip(ga.edges(), gb.edges()))
        assert torch.equal(ga.batch_num_nodes(), gb.batch_num_nodes())
        for frame_a, frame_b in ((ga.ndata, gb.ndata), (ga.edata, gb.edata)):
            assert set(frame_a) == set(frame_b)
            for k in frame_a:
                assert torch.equal(frame_a[k], frame_b[k]), k


@pytest.mark.parametrize('cfg', sorted(GA.CONFIGS))
def test_state_dict_matches_reference_and_loads_strict(cfg):
    z = load('net3dae.npz')
    ref = sd_from_npz(z, f'{cfg}/sd')
    torch.manual_seed(0)
    model = amd.Net3DAE(**GA.CONFIGS[cfg])
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in z[f'{cfg}/sd_keys']]
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_node_wise_options_share_one_attribute_and_the_later_wins():
    kw = dict(GA.CONFIGS['a'])
    enc_only = amd.Net3DAE(**dict(kw, node_wise_encoder_layers=2, node_wise_output_layers=0))
    both = amd.Net3DAE(**dict(kw, node_wise_encoder_layers=2, node_wise_output_layers=1))
    out_only = amd.Net3DAE(**dict(kw, node_wise_encoder_layers=0, node_wise_output_layers=3))
    neither = amd.Net3DAE(**kw)
    assert len(enc_only.node_wise_output_network.fully_connected) == 2
    assert len(both.node_wise_output_network.fully_connected) == 1          # node_wise_output_layers assigned last
    assert len(out_only.node_wise_output_network.fully_connected) == 3      # built, but applied only when node_wise_encoder_layers > 0
    assert out_only.node_wise_encoder_layers == 0
    assert not hasattr(neither, 'node_wise_output_network')
    assert not any(k.startswith('node_wise_encoder') for k in both.state_dict())


def test_submodule_names_and_unknown_kwargs():
    m = amd.Net3DAE(**dict(GA.CONFIGS['b'], some_future_option=1, target_dim=5))
    names = {n for n, _ in m.named_children()}
    assert {'edge_input', 'encoder_layers', 'decoder_layers', 'distance_net'} <= names
    assert m.node_projection_net is None and 'node_embedding' in dict(m.named_parameters())
    c = amd.Net3DAE(**GA.CONFIGS['c'])
    assert c.distance_net is None and c.node_projection_net is not None
    f = amd.Net3DAE(**dict(GA.CONFIGS['a'], use_node_features=True))
    assert hasattr(f, 'atom_encoder') and 'node_embedding' not in dict(f.named_parameters())


@pytest.mark.parametrize('kw, exc, word', [
    (dict(distance_net=True, projection_layers=2, projection_dim=0), ValueError, 'projection_dim'),
    (dict(readout_aggregators=['min', 'std']), NotImplementedError, 'readout_aggregators'),
    (dict(activation='gelu'), NotImplementedError, 'activation'),
    (dict(reduce_func='max'), ValueError, 'reduce function'),
    (dict(encoder_depth=-1), ValueError, 'encoder_depth'),
])
def test_constructor_refusals_name_their_option(kw, exc, word):
    with pytest.raises(exc, match=word):
        amd.Net3DAE(**dict(GA.CONFIGS['a'], **kw))


def test_fused_head_is_chosen_only_where_it_applies():
    kw = dict(GA.CONFIGS['a'])
    m = amd.Net3DAE(**kw).train()
    assert m.fused_head_refusal() is None
    assert 'projection_layers' in amd.Net3DAE(**dict(kw, projection_layers=3)).train().fused_head_refusal()
    assert 'projection_dim' in amd.Net3DAE(**dict(kw, projection_dim=129)).train().fused_head_refusal()
    d = amd.Net3DAE(**kw).train()
    for fc in d.distance_net.fully_connected:
        fc.dropout = torch.nn.Dropout(0.1)
    assert 'dropout' in d.fused_head_refusal()
    assert d.eval().fused_head_refusal() is None          # dropout is the identity in eval mode
    old = net3d_ae.FUSED_PAIR_HEAD
    net3d_ae.FUSED_PAIR_HEAD = False
    try:
        assert 'FUSED_PAIR_HEAD' in m.fused_head_refusal()
    finally:
        net3d_ae.FUSED_PAIR_HEAD = old


def test_plugin_names_bind_the_autoencoder():
    for name in ('Net3DAE', 'NTXentAE', 'contrastive_vae_collate'):
        assert name in amd.__all__
    names = launcher.plugin_names()
    assert names['Net3DAE'] is amd.Net3DAE is net3d_ae.Net3DAE
    assert names['NTXentAE'] is amd.NTXentAE
    assert names['contrastive_vae_collate'] is amd.contrastive_vae_collate


def test_ntxentae_constructor_and_world_size_refusal(monkeypatch):
    loss = amd.NTXentAE(norm=True, tau=0.1, uniformity_reg=0, variance_reg=0, covariance_reg=0, reconstruction_reg=0.5)
    assert loss.reconstruction_reg == 0.5 and loss.tau == 0.1
    assert amd.NTXentAE().reconstruction_reg == 1
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss.attach_group(group)
    z = torch.zeros(4, 8)
    with pytest.raises(NotImplementedError, match='NTXentAE'):
        loss(z, z, torch.zeros(5, 1), torch.zeros(5, 1))


def test_header_declares_the_pair_head_and_the_library_exports_it():
    import __graft_entry__ as ge
    ge.build()
    lib = L.load()
    new = ['i3d_pair_mlp_supported', 'i3d_pair_mlp_workspace_floats', 'i3d_pair_mlp_fwd', 'i3d_pair_mlp_bwd',
           'i3d_mse_partial_floats', 'i3d_mse_fwd', 'i3d_mse_bwd']
    declared = L.declared_symbols()
    for name in new:
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_abi_version() == 2
    assert lib.i3d_pair_mlp_supported(70) == 1 and lib.i3d_pair_mlp_supported(3) == 1 and lib.i3d_pair_mlp_supported(128) == 1
    assert lib.i3d_pair_mlp_supported(129) == 0 and lib.i3d_pair_mlp_supported(0) == 0
    assert lib.i3d_pair_mlp_workspace_floats(1_000_000, 70) > 0
    # argument validation happens on the host before any launch: no GPU needed
    rc = lib.i3d_pair_mlp_fwd(*([None] * 9), 10, 200, 1, 1e-5, 0.1, *([None] * 8))
    assert rc == -1 and b'width' in lib.i3d_last_error()
    rc = lib.i3d_pair_mlp_fwd(*([None] * 9), 0, 70, 1, 1e-5, 0.1, *([None] * 8))
    assert rc == 0          # no pairs: nothing to launch
