"""GeoMol's message-passing network (GeomolGNNWrapperOGBFeat) on the host: the reference's parameter layout, the kept quirks, the
plugin surface, the C ABI of the step kernels and the accepted inputs (fixture: tests/golden/gen_golden_geomol.py)."""
import importlib
import types

import numpy as np
import pytest
import torch

from helpers import amd, load, mols_from_npz, sd_from_npz

import gen_golden_geomol as GM

geomol = importlib.import_module('3dinfomax_amd.geomol')
L = importlib.import_module('3dinfomax_amd._lib')
alias = importlib.import_module('infomax3d_amd')
launcher = importlib.import_module('launch_reference')

CLASSES = ('GeomolGNNWrapperOGBFeat', 'GeomolGNNOGBFeat', 'GeomolMetaLayer', 'EdgeModel', 'GeomolNodeModel', 'GeomolMLP')
SYMBOLS = ('i3d_geomol_edge_fwd', 'i3d_geomol_edge_bwd', 'i3d_geomol_residual_fwd', 'i3d_geomol_residual_bwd')


@pytest.mark.parametrize('cfg', sorted(GM.CONFIGS))
def test_state_dict_matches_reference_and_loads_strict(cfg):
    z = load('geomol.npz')
    ref = sd_from_npz(z, f'{cfg}/sd')
    torch.manual_seed(0)
    model = amd.GeomolGNNWrapperOGBFeat(**GM.CONFIGS[cfg])
    sd = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_key_list_of_the_default_depth():
    keys = list(amd.GeomolGNNWrapperOGBFeat(hidden_dim=16, target_dim=1, n_layers=2, readout_layers=2).state_dict())
    assert len(keys) == 57
    assert keys[0] == 'node_gnn.bond_encoder.bond_embedding_list.0.weight' and keys[-1] == 'output.fully_connected.1.linear.bias'
    for name in ('node_init', 'edge_init', 'update.edge_model.mlp', 'update.node_model.node_mlp_1', 'update.node_model.node_mlp_2'):
        assert [k for k in keys if k.startswith(f'node_gnn.{name}.')] == [f'node_gnn.{name}.layers.{i}.{p}' for i in (0, 2, 4)
                                                                          for p in ('weight', 'bias')]
    assert 'node_gnn.update.edge_model.node_in.bias' not in keys and 'node_gnn.update.edge_model.node_out.bias' not in keys
    assert 'node_gnn.update.edge_model.edge.bias' in keys


def test_mlp_width_rule_in_both_directions():
    narrow = amd.GeomolMLP(24, 3, 2)                 # out_dim < 10: the hidden width is in_dim
    assert [tuple(m.weight.shape) for m in narrow.layers if isinstance(m, torch.nn.Linear)] == [(24, 24), (24, 24), (3, 24)]
    wide = amd.GeomolMLP(7, 12, 2)                   # else out_dim
    assert [tuple(m.weight.shape) for m in wide.layers if isinstance(m, torch.nn.Linear)] == [(12, 7), (12, 12), (12, 12)]
    edge = amd.GeomolMLP(7, 10, 1)
    assert [tuple(m.weight.shape) for m in edge.layers if isinstance(m, torch.nn.Linear)] == [(10, 7), (10, 10)]
    assert list(edge.state_dict()) == ['layers.0.weight', 'layers.0.bias', 'layers.2.weight', 'layers.2.bias']
    assert not any(isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)) for m in wide.modules())


@pytest.mark.parametrize('depth', [1, 3, 6])
def test_update_exists_once_whatever_the_depth(depth):
    model = amd.GeomolGNNWrapperOGBFeat(hidden_dim=12, target_dim=2, depth=depth, n_layers=2)
    metas = [m for m in model.modules() if isinstance(m, amd.GeomolMetaLayer)]
    assert len(metas) == 1 and metas[0] is model.node_gnn.update and model.node_gnn.depth == depth
    assert len(model.state_dict()) == 57
    for eps in (metas[0].edge_eps, metas[0].node_eps):
        assert isinstance(eps, torch.nn.Parameter) and eps.shape == (1,) and float(eps.detach()) == 0.0
    # init MLPs have num_layers 2 whatever n_layers says
    one = amd.GeomolGNNWrapperOGBFeat(hidden_dim=12, target_dim=2, depth=depth, n_layers=1)
    assert len(one.node_gnn.node_init.layers) == 5 and len(one.node_gnn.update.edge_model.mlp.layers) == 3


def test_unknown_kwargs_are_swallowed_and_momentum_is_unused():
    model = amd.GeomolGNNWrapperOGBFeat(hidden_dim=12, target_dim=2, batch_norm_momentum=0.93, dropout=0.3, random_vec_dim=10,
                                        something_else='x')
    assert not any(isinstance(m, torch.nn.BatchNorm1d) for m in model.node_gnn.modules())
    bns = [m for m in model.output.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(bns) == 1 and bns[0].momentum == 0.1              # the readout keeps momentum 0.1
    gnn = amd.GeomolGNNOGBFeat(hidden_dim=12, anything=1)
    assert gnn.depth == 3 and gnn.hidden_dim == 12
    with pytest.raises(NotImplementedError, match='batch_norm'):
        amd.GeomolMLP(8, 8, 2, batch_norm=True)


def test_exported_by_the_package_the_alias_and_the_launcher():
    names = launcher.plugin_names()
    for name in CLASSES:
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(alias, name) is getattr(geomol, name)
        assert names[name] is getattr(geomol, name)
    assert geomol.FUSED_STEP is True


def test_geomol_entry_points_are_declared_and_validate_on_the_host():
    declared = set(L.declared_symbols())
    assert set(SYMBOLS) <= declared
    lib = L.load()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert lib.i3d_abi_version() == 2
    for n, e, h in ((0, 0, 16), (4, -1, 16), (4, 0, 0)):
        assert lib.i3d_geomol_edge_fwd(None, None, None, None, n, e, h, None, None) == -1
        assert lib.i3d_geomol_edge_bwd(None, None, None, None, None, n, e, h, None, None, None) == -1
    for r, h in ((-1, 16), (4, 0)):
        assert lib.i3d_geomol_residual_fwd(None, None, None, r, h, None, None) == -1
        assert lib.i3d_geomol_residual_bwd(None, None, None, r, h, None, None, None, None) == -1
    assert lib.i3d_geomol_edge_fwd(None, None, None, None, 4, 3, 16, None, None) == -1        # null pointers with valid sizes
    assert lib.i3d_geomol_residual_bwd(None, None, None, 4, 16, None, None, None, None) == -1
    assert b'invalid argument' in lib.i3d_last_error()


def _pyg(mols):
    d = GM.data_of(mols)
    return types.SimpleNamespace(z=d.z, edge_index=d.edge_index, edge_attr=d.edge_attr, batch=d.batch)


def test_pyg_style_object_gives_the_same_index_as_the_batched_graph():
    z = load('geomol.npz')
    mols = mols_from_npz(z, 'a/mol')
    data = _pyg(mols)
    bg = geomol.as_geomol_graph(data)
    assert geomol.as_geomol_graph(data) is bg                     # converted once, cached on the object
    ref = amd.batch([amd.bond_graph(m) for m in mols])
    assert geomol.as_geomol_graph(ref) is ref
    a, b = bg.index(), ref.index()
    assert (a.num_nodes, a.num_edges, a.num_graphs, a.max_in_degree) == (b.num_nodes, b.num_edges, b.num_graphs, b.max_in_degree)
    for f in ('in_ptr', 'perm', 'src_s', 'dst_s', 'out_ptr', 'out_epos', 'graph_ptr', 'inv_perm'):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(bg.ndata['feat'], ref.ndata['feat']) and torch.equal(bg.edata['feat'], ref.edata['feat'])
    assert torch.equal(bg.batch_num_nodes(), ref.batch_num_nodes())


def test_decreasing_batch_vector_is_refused_by_name():
    z = load('geomol.npz')
    data = _pyg(mols_from_npz(z, 'c/mol'))
    data.batch = data.batch.flip(0)
    with pytest.raises(ValueError, match='batch is not non-decreasing'):
        geomol.as_geomol_graph(data)
    short = _pyg(mols_from_npz(z, 'c/mol'))
    short.batch = short.batch[:-1]
    with pytest.raises(ValueError, match='batch'):
        geomol.as_geomol_graph(short)


def test_fixture_holds_what_the_gpu_tests_read():
    z = load('geomol.npz')
    for cfg, kw in sorted(GM.CONFIGS.items()):
        mols = mols_from_npz(z, f'{cfg}/mol')
        assert any(m.n_atoms > 64 for m in mols) and any(m.n_atoms == 1 and m.src.shape[0] == 0 for m in mols)
        n, e = sum(m.n_atoms for m in mols), sum(m.src.shape[0] for m in mols)
        assert z[f'{cfg}/feat'].shape == (n, kw['hidden_dim']) and z[f'{cfg}/efeat'].shape == (e, kw['hidden_dim'])
        assert z[f'{cfg}/out'].shape == (len(mols), kw['target_dim'])
        grads = {k.split('/grad/')[1] for k in z.files if k.startswith(f'{cfg}/grad/')}
        assert grads == set(sd_from_npz(z, f'{cfg}/sd')) - {k for k in sd_from_npz(z, f'{cfg}/sd') if 'running' in k or 'tracked' in k}
        assert all(f'{cfg}/ref_err/grad/{k}' in z.files for k in grads)
        assert float(z[f'{cfg}/ref_err/out']) < 1e-5
        e_eps, n_eps = float(z[f'{cfg}/sd/node_gnn.update.edge_eps'][0]), float(z[f'{cfg}/sd/node_gnn.update.node_eps'][0])
        assert e_eps != 0.0 and n_eps != 0.0 and e_eps != n_eps                 # zero would hide both residual paths
        if cfg != 'd':                                                         # 'd' has taken one SGD step
            assert e_eps == np.float32(GM.EDGE_EPS) and n_eps == np.float32(GM.NODE_EPS)
