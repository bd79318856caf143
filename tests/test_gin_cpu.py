"""OGBGNN (GIN + virtual node) on the host: the reference's parameter layout, the refused options, the plugin surface, the C ABI of
the message kernels and the per-batch code-sorted edge index (fixture: tests/golden/gen_golden_gin.py)."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load, mols_from_npz, sd_from_npz

import gen_golden_gin as GG

gin = importlib.import_module('3dinfomax_amd.gin')
ops = importlib.import_module('3dinfomax_amd.ops')
L = importlib.import_module('3dinfomax_amd._lib')
alias = importlib.import_module('infomax3d_amd')
launcher = importlib.import_module('launch_reference')

CLASSES = ('OGBGNN', 'GNN_node', 'GNN_node_Virtualnode', 'GINConv')


@pytest.mark.parametrize('cfg', sorted(GG.CONFIGS))
def test_state_dict_matches_reference_and_loads_strict(cfg):
    z = load('ogbgnn.npz')
    ref = sd_from_npz(z, f'{cfg}/sd')
    torch.manual_seed(0)
    model = amd.OGBGNN(emb_dim=3, **GG.CONFIGS[cfg])          # unknown kwargs are swallowed (configs/26.yml: emb_dim)
    sd = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_kept_quirks_of_the_reference():
    vn = amd.OGBGNN(hidden_dim=8, num_layers=2, virtual_node=True, batch_norm_momentum=0.93)
    assert all(conv.mlp[1].momentum == 0.1 for conv in vn.node_gnn.convs)          # GINConv(hidden_dim): the default momentum
    assert all(bn.momentum == 0.93 for bn in vn.node_gnn.batch_norms)
    assert all(mlp[1].momentum == 0.93 and mlp[4].momentum == 0.93 for mlp in vn.node_gnn.mlp_virtualnode_list)
    assert len(vn.node_gnn.mlp_virtualnode_list) == 1
    assert torch.count_nonzero(vn.node_gnn.virtualnode_embedding.weight) == 0
    assert all(float(conv.eps.detach()) == 0.0 and conv.eps.shape == (1,) for conv in vn.node_gnn.convs)
    plain = amd.OGBGNN(hidden_dim=8, num_layers=2, virtual_node=False, batch_norm_momentum=0.93)
    assert all(conv.mlp[1].momentum == 0.93 for conv in plain.node_gnn.convs)
    assert isinstance(plain.node_gnn, amd.GNN_node) and isinstance(vn.node_gnn, amd.GNN_node_Virtualnode)


@pytest.mark.parametrize('kw, exc, word', [
    (dict(gnn_type='gcn'), NotImplementedError, 'gnn_type'),
    (dict(graph_pooling='max'), NotImplementedError, 'graph_pooling'),
    (dict(graph_pooling='attention'), NotImplementedError, 'graph_pooling'),
    (dict(graph_pooling='set2set'), NotImplementedError, 'graph_pooling'),
    (dict(graph_pooling='median'), ValueError, 'pooling'),
    (dict(num_layers=1), ValueError, 'layers'),
    (dict(JK='concat'), ValueError, 'JK'),
])
def test_refusals_name_their_argument(kw, exc, word):
    with pytest.raises(exc, match=word):
        amd.OGBGNN(**dict(dict(hidden_dim=8, num_layers=2), **kw))


def test_max_pooling_refusal_says_what_the_reference_does():
    with pytest.raises(NotImplementedError, match='without instantiating'):
        amd.OGBGNN(hidden_dim=8, num_layers=2, graph_pooling='max')


def test_exported_by_the_package_the_alias_and_the_launcher():
    names = launcher.plugin_names()
    for name in CLASSES:
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(alias, name) is getattr(gin, name)
        assert names[name] is getattr(gin, name)
    assert gin.FUSED_CONV is True


def test_gin_entry_points_are_declared_and_exported():
    declared = [s for s in L.declared_symbols() if s.startswith('i3d_gin_')]
    assert {'i3d_gin_conv_fwd', 'i3d_gin_conv_bwd', 'i3d_gin_conv_bwd_partial_floats', 'i3d_gin_chunk_edges'} <= set(declared)
    lib = L.load()
    for s in declared:
        assert hasattr(lib, s), s
        assert s in L._SIGNATURES, s
    assert lib.i3d_abi_version() == 2


def test_impossible_sizes_are_refused_before_any_launch():
    lib = L.load()
    assert lib.i3d_gin_conv_bwd_partial_floats(0, 0, 16, 60) == 0
    assert lib.i3d_gin_conv_bwd_partial_floats(4, 0, 16, 257) == 0
    chunk = lib.i3d_gin_chunk_edges()
    assert lib.i3d_gin_conv_bwd_partial_floats(4, 0, 16, 60) == 2 * (60 * 16 + (1 << 16))
    assert lib.i3d_gin_conv_bwd_partial_floats(4, chunk + 1, 16, 60) == 2 * ((2 + 60) * 16 + (1 << 16))
    for n, e, h, v in ((0, 0, 16, 60), (4, -1, 16, 60), (4, 0, 0, 60), (4, 0, 16, 0), (4, 0, 16, 257)):
        assert lib.i3d_gin_conv_fwd(None, None, None, 0, None, v, None, None, None, None, n, e, h, None, None, None) == -1
        assert lib.i3d_gin_conv_bwd(None, None, None, v, *([None] * 8), n, e, h, None, None, None, None, None) == -1
    assert b'invalid argument' in lib.i3d_last_error()


@pytest.mark.parametrize('E, V', [(0, 60), (1, 60), (997, 60), (5000, 256)])
def test_code_sorted_index_against_numpy(E, V):
    rng = np.random.default_rng(E + V)
    p = rng.random(V) ** 6            # skewed: a few codes hold most edges, many hold none
    codes = rng.choice(V, size=E, p=p / p.sum()).astype(np.int32)
    order, ptr = ops.code_sorted_index(torch.from_numpy(codes), V)
    assert order.dtype == torch.int32 and ptr.dtype == torch.int32 and ptr.shape == (V + 1,)
    np.testing.assert_array_equal(order.numpy(), np.argsort(codes, kind='stable'))
    np.testing.assert_array_equal(ptr.numpy(), np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=V))]))


def test_edge_codes_enumeration_matches_the_table_rows():
    """row v of the table is the embedding of the combination with joint code v: first feature column fastest"""
    dims = [5, 6, 2]
    comb = gin._combinations(dims, 'cpu')
    assert comb.shape == (60, 3)
    strides = torch.tensor([1, 5, 30])
    assert torch.equal((comb * strides).sum(1), torch.arange(60))
    for k, d in enumerate(dims):
        assert int(comb[:, k].max()) == d - 1


def test_fixture_holds_what_the_gpu_tests_read():
    z = load('ogbgnn.npz')
    for cfg in sorted(GG.CONFIGS):
        mols = mols_from_npz(z, f'{cfg}/mol')
        assert any(m.n_atoms > 64 for m in mols) and any(m.n_atoms == 1 and m.src.shape[0] == 0 for m in mols)
        n = sum(m.n_atoms for m in mols)
        assert z[f'{cfg}/feat'].shape == (n, 16) and z[f'{cfg}/out'].shape == (len(mols), GG.CONFIGS[cfg]['target_dim'])
        grads = [k for k in z.files if k.startswith(f'{cfg}/grad/')]
        assert grads and all(f'{cfg}/ref_err/grad/' + k.split('/grad/')[1] in z.files for k in grads)
        assert float(z[f'{cfg}/ref_err/out']) < 1e-5
        for l in range(3):
            assert float(z[f'{cfg}/sd/node_gnn.convs.{l}.eps'][0]) != 0.0
        if GG.CONFIGS[cfg]['virtual_node']:
            assert np.count_nonzero(z[f'{cfg}/sd/node_gnn.virtualnode_embedding.weight']) > 0
