"""SAN on the host: the reference's parameter layout, the refusals, the data side (Laplacian encoding, san_graph), the C ABI's argument
checks, and the composed path in torch against the reference fixture (tests/golden/gen_golden_san.py)."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err

import gen_golden_san as GS
import san_reference as R

san = importlib.import_module('3dinfomax_amd.san')
graph = importlib.import_module('3dinfomax_amd.graph')
synth = importlib.import_module('3dinfomax_amd.synth')
L = importlib.import_module('3dinfomax_amd._lib')
alias = importlib.import_module('infomax3d_amd')
launcher = importlib.import_module('launch_reference')

CLASSES = ('SAN', 'SAN_NodeLPE', 'GraphTransformerLayer', 'MultiHeadAttentionLayer')
SAN_YML = dict(target_dim=1, in_feat_dropout=0.0, layer_norm=False, batch_norm=True, gamma=1e-6, full_graph=True, GT_hidden_dim=64,
               GT_n_heads=4, GT_out_dim=64, GT_layers=10, LPE_n_heads=4, LPE_layers=3, LPE_dim=16, dropout=0.01, batch_norm_momentum=0.1,
               readout_batchnorm=True, readout_hidden_dim=90, readout_layers=2, readout_aggregators=['min', 'max', 'mean', 'sum'],
               residual=True)


def batch_of(z, cfg, device='cpu'):
    """the fixture's batch of configuration `cfg` as the package's own data side builds it, the stored encoding put in"""
    mols = mols_from_npz(z, f'{cfg}/mol')
    parts = GS.san_graphs(mols, GS.CONFIGS[cfg]['full_graph'])
    g = amd.batch(parts)
    g.ndata['pos_enc'] = torch.from_numpy(z[f'{cfg}/pos_enc'].copy())
    return g.to(device) if device != 'cpu' else g


def model_of(z, cfg):
    torch.manual_seed(0)
    model = amd.SAN(**GS.CONFIGS[cfg])
    model.load_state_dict(GS.state_from_npz(z, cfg), strict=True)
    GS.zero_dropout(model)
    return model


def loss_of(cfg, y, z):
    return (y ** 2).mean() if cfg in ('a', 'd') else torch.nn.L1Loss()(y, torch.from_numpy(z[f'{cfg}/target']).to(y.device))


def check_against_fixture(model, g, z, cfg, what):
    """the rule of tests/test_gpu_gin.py: outputs to 1e-4, every gradient tensor at max(1e-3, 4 x the fp32 reference's own error of
    that tensor against fp64), the buffers after the step"""
    model.train(cfg != 'd')
    y = model(g)
    e_out, e_feat = rel_err(y.detach().cpu(), z[f'{cfg}/out']), rel_err(g.ndata['feat'].detach().cpu(), z[f'{cfg}/feat'])
    print(f'san model {what} {cfg}: output rel_err {e_out:.2e}, node state rel_err {e_feat:.2e} '
          f"(the reference's own fp32 error: {float(z[f'{cfg}/ref_err/out']):.2e}, {float(z[f'{cfg}/ref_err/feat']):.2e})")
    assert e_out < 1e-4 and e_feat < 1e-4, what
    loss = loss_of(cfg, y, z)
    assert abs(float(loss.detach()) - float(z[f'{cfg}/loss'])) <= 1e-4 * abs(float(z[f'{cfg}/loss']))
    # buffers after the step: running statistics and counters (d, eval mode: they must be what they were)
    sd = model.state_dict()
    stored = [k for k in z.files if k.startswith(f'{cfg}/buf_after/')]
    assert stored
    for key in stored:
        k, ref = key.split('/buf_after/')[1], z[key]
        if 'running' in k:
            assert rel_err(sd[k].detach().cpu(), ref) < 1e-5, k
        else:
            assert int(sd[k]) == int(ref), k
    if cfg == 'd':
        return
    model.zero_grad()
    loss.backward()
    names = [str(n) for n in z[f'{cfg}/grad_names']]
    ref_err = dict(zip(names, z[f'{cfg}/ref_err/grad'].tolist()))
    params = dict(model.named_parameters())
    got = {k: GS.grad_view(k, params[k].grad.detach().cpu()) for k in names}
    ref = {k: torch.from_numpy(z[f'{cfg}/grad/{k}']) for k in names}
    scale = max(float(v.abs().max()) for v in ref.values())
    worst = max(rel_err(got[k], ref[k]) for k in names if float(ref[k].abs().max()) > 1e-4 * scale)
    print(f'san model {what} {cfg}: worst gradient tensor {worst:.2e} of its largest entry (tensors above 1e-4 of the largest gradient)')
    for k in names:
        # one tensor per call, its own rtol (tests/test_gpu_gin.py); the '_scale' entry keeps grads_close's absolute floor tied to the
        # largest gradient of the whole set
        rtol = max(1e-3, 4 * ref_err[k])
        grads_close({k: got[k], '_scale': torch.tensor([scale])}, {k: ref[k], '_scale': torch.tensor([scale])}, rtol,
                    what=f'{what} {cfg} ')


@pytest.mark.parametrize('cfg', sorted(GS.CONFIGS))
def test_state_dict_matches_reference_and_loads_strict(cfg):
    z = load('san.npz')
    src = 'a' if cfg == 'd' else cfg
    names = [str(n) for n in z[f'{src}/sd_names']]
    shapes = [tuple(d for d in row if d >= 0) for row in z[f'{src}/sd_shapes'].tolist()]
    torch.manual_seed(0)
    model = amd.SAN(some_unknown_kwarg=3, **GS.CONFIGS[cfg])          # unknown kwargs are swallowed
    sd = model.state_dict()
    assert list(sd) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert any(k.startswith('gnn.embedding_e_fake.') for k in names)
    ref = GS.state_from_npz(z, cfg)
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_yml_parameters_construct():
    model = amd.SAN(**SAN_YML)
    assert len(model.gnn.layers) == 10 and len(model.gnn.PE_Transformer.layers) == 3
    assert all(layer.attention.Q.bias is None and layer.O_h.bias is not None for layer in model.gnn.layers)
    assert all(layer.batch_norm1_h.momentum == 0.1 for layer in model.gnn.layers)
    assert model.output.fully_connected[0].linear.in_features == 4 * 64


@pytest.mark.parametrize('kw, word', [
    (dict(GT_out_dim=32, residual=True), 'GT_out_dim'),
    (dict(GT_n_heads=5), 'GT_n_heads'),
    (dict(GT_hidden_dim=60, GT_out_dim=60, GT_n_heads=8), 'GT_n_heads'),
])
def test_refusals_name_their_argument(kw, word):
    with pytest.raises(ValueError, match=word):
        amd.SAN(**dict(SAN_YML, GT_layers=2, **kw))


def test_exported_by_the_package_the_alias_and_the_launcher():
    names = launcher.plugin_names()
    for name in CLASSES:
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(alias, name) is getattr(san, name)
        assert names[name] is getattr(san, name)
    assert amd.san_graph is graph.san_graph and amd.laplacian_pos_enc is graph.laplacian_pos_enc
    assert san.FUSED_ATTENTION is True


# ---- data side -----------------------------------------------------------------------------------------------------------------
def _mols():
    return GS.GG.molecules(71)


@pytest.mark.parametrize('self_loops', [True, False])
def test_laplacian_pos_enc_is_an_eigen_decomposition(self_loops):
    for mol in _mols():
        n = mol.n_atoms
        pe = graph.laplacian_pos_enc(mol, 10, self_loops)
        raw = graph.laplacian_pos_enc(mol, 10, self_loops, normalize=False)
        assert pe.shape == (n, 10, 2) and pe.dtype == torch.float32
        m = min(n, 10)
        assert torch.isnan(pe[:, m:]).all() and not torch.isnan(pe[:, :m]).any()          # NaN padding for n < num_freq
        lam = pe[0, :m, 0]
        assert torch.equal(pe[:, :m, 0], lam.expand(n, m)) and bool((lam[1:] >= lam[:-1]).all())
        M = graph.san_laplacian(mol, self_loops)
        assert torch.equal(M, M.T)
        V = raw[:, :m, 1]
        assert float((M @ V - V * lam).abs().max()) < 1e-5                                # L v = lambda v, un-normalised vectors
        rows = torch.nn.functional.normalize(V, p=2, dim=1, eps=1e-12)
        assert torch.allclose(pe[:, :m, 1], rows, atol=1e-7)


def test_laplacian_of_a_single_atom_and_of_a_hand_case():
    single = next(m for m in _mols() if m.n_atoms == 1)
    for loops in (True, False):
        pe = graph.laplacian_pos_enc(single, 10, loops)
        assert pe.shape == (1, 10, 2) and float(pe[0, 0, 0]) == 1.0 and abs(float(pe[0, 0, 1])) == 1.0
        assert torch.isnan(pe[0, 1:]).all()
    # two bonded atoms with self loops: A + I = ones, D = 2, L = [[1, -1], [-1, 1]], eye - L / D_j = [[.5, .5], [.5, .5]]: eigenvalues 0, 1
    pair = synth.Molecule(2, np.array([0, 1]), np.array([1, 0]), single.atom_feat.repeat(2, 0), np.zeros((2, 3), np.int64),
                          single.coords.repeat(2, 0))
    assert torch.allclose(graph.san_laplacian(pair), torch.full((2, 2), 0.5))
    assert torch.allclose(graph.laplacian_pos_enc(pair, 10)[0, :2, 0], torch.tensor([0.0, 1.0]), atol=1e-6)


def test_laplacian_scales_the_columns_as_the_reference_lines_do():
    """a chain of three atoms, degrees 2, 3, 2 with the self loops (1, 2, 1 without): `eye - N * L * N` with N a vector divides column
    j by D_j, and eigh reads the lower triangle - entries (1, 0) and (2, 1) are 1/D_0 = 1/2 and 1/D_1 = 1/3 (1 and 1/2 without loops);
    a symmetric scaling would make both 1/sqrt(6) (1/sqrt(2)).  Worked by hand."""
    single = next(m for m in _mols() if m.n_atoms == 1)
    chain = synth.Molecule(3, np.array([0, 1, 1, 2]), np.array([1, 0, 2, 1]), single.atom_feat.repeat(3, 0), np.zeros((4, 3), np.int64),
                           single.coords.repeat(3, 0))
    third = 1.0 / 3.0
    assert torch.allclose(graph.san_laplacian(chain, True), torch.tensor([[.5, .5, 0.], [.5, third, third], [0., third, .5]]), atol=1e-7)
    assert torch.allclose(graph.san_laplacian(chain, False), torch.tensor([[0., 1., 0.], [1., 0., .5], [0., .5, 0.]]), atol=1e-7)
    # with loops: det = (1/2 - x) [(1/3 - x)(1/2 - x) - 1/9 - 1/4]: x = 1/2 and x^2 - 5/6 x - 7/36 = 0, x = (5 +- sqrt(53)) / 12
    lam = graph.laplacian_pos_enc(chain, 10, True)[0, :3, 0]
    want = torch.tensor([(5 - np.sqrt(53.0)) / 12, 0.5, (5 + np.sqrt(53.0)) / 12], dtype=torch.float32)
    assert torch.allclose(lam, want, atol=1e-6)
    # without: zero diagonal, off-diagonals 1 and 1/2: x = 0, +-sqrt(1 + 1/4)
    lam = graph.laplacian_pos_enc(chain, 10, False)[0, :3, 0]
    assert torch.allclose(lam, torch.tensor([-np.sqrt(1.25), 0.0, np.sqrt(1.25)], dtype=torch.float32), atol=1e-6)
    # eigenvalue 1/2: row 0 gives v1 = 0, row 1 gives v2 = -3/2 v0: (2, 0, -3) / sqrt(13), either sign
    vec = graph.laplacian_pos_enc(chain, 10, True, normalize=False)[:, 1, 1]
    assert torch.allclose(vec.abs(), torch.tensor([2.0, 0.0, 3.0]) / 13 ** 0.5, atol=1e-6) and float(vec[0] * vec[2]) < 0


def test_edge_context_is_cached_on_the_index_and_builds_the_composed_tensors_on_demand():
    g = amd.batch([graph.san_graph(m) for m in _mols()[:2]])
    dims = list(synth.BOND_FEATURE_DIMS)
    ec = san.edge_context(g, dims, True)
    assert san.edge_context(g.local_copy(), dims, True) is ec          # a stepped-on resident batch is forwarded through copies
    assert san.edge_context(g, dims, False) is not ec
    assert ec._lazy == {}
    assert ec.src.dtype == torch.int64 and ec.real_b.dtype == torch.bool and set(ec._lazy) == {'src', 'perm', 'real_b'}
    assert int(ec.real_b.sum()) == int(g.edata['real'].sum())


def test_san_graph_layout_and_sign_flips():
    for mol in _mols():
        n = mol.n_atoms
        g = graph.san_graph(mol)
        src, dst = synth.complete_graph_edges(n)
        assert np.array_equal(g.edges()[0].numpy(), src) and np.array_equal(g.edges()[1].numpy(), dst)
        feat, real = g.edata['feat'], g.edata['real']
        assert feat.dtype == torch.int64 and feat.shape == (n * (n - 1), 3) and real.dtype == torch.int64
        bonds = {(int(s), int(d)): f for s, d, f in zip(mol.src, mol.dst, mol.bond_feat)}
        assert int(real.sum()) == len(bonds)
        for e, (s, d) in enumerate(zip(src.tolist(), dst.tolist())):
            if (s, d) in bonds:
                assert int(real[e]) == 1 and np.array_equal(feat[e].numpy(), bonds[(s, d)])
            else:
                assert int(real[e]) == 0 and int(feat[e].abs().sum()) == 0
        plain = graph.laplacian_pos_enc(mol)
        assert torch.equal(torch.nan_to_num(g.ndata['pos_enc'], nan=7.0), torch.nan_to_num(plain, nan=7.0))
    mol = _mols()[0]
    torch.manual_seed(3)
    a = graph.san_graph(mol, sign_flip=True).ndata['pos_enc']
    torch.manual_seed(3)
    b = graph.san_graph(mol, sign_flip=True).ndata['pos_enc']
    torch.manual_seed(3)
    signs = torch.where(torch.rand(10) >= 0.5, 1.0, -1.0)
    assert torch.equal(a, b) and (signs < 0).any() and (signs > 0).any()
    plain = graph.laplacian_pos_enc(mol)
    assert torch.equal(a[:, :, 0], plain[:, :, 0]) and torch.equal(a[:, :, 1], plain[:, :, 1] * signs)
    batched = amd.graph_collate([(graph.san_graph(m), torch.zeros(1)) for m in _mols()])[0][0]
    assert batched.ndata['pos_enc'].shape[0] == batched.number_of_nodes() == sum(m.n_atoms for m in _mols())
    assert batched.edata['real'].shape[0] == batched.number_of_edges()


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    declared = {s for s in L.declared_symbols() if s.startswith('i3d_san_')}
    assert declared == {'i3d_san_attn_fwd', 'i3d_san_attn_bwd', 'i3d_san_attn_bwd_partial_floats', 'i3d_san_attn_chunk_edges',
                        'i3d_san_attn_takes', 'i3d_san_edge_codes'}
    lib = L.load()
    for s in declared:
        assert hasattr(lib, s), s


def _fwd(lib, n, e, h, nh, v, ptrs=8, full=1):
    p = [ptrs or None] * 13          # a non-null value stands for a pointer: every refusal below comes before any use
    q, k, vv, q2, k2, te, te2, codes, real, in_ptr, src_s, out, z = p
    return lib.i3d_san_attn_fwd(q, k, vv, q2, k2, 5 * h, te, te2, v, codes, real, in_ptr, src_s, n, e, h, nh, full, 0.5, out, ptrs or None,
                                z, None)


def _bwd(lib, n, e, h, nh, v, ptrs=8, full=1):
    a = ptrs or None
    return lib.i3d_san_attn_bwd(a, a, a, a, a, a, a, a, a, 5 * h, a, a, v, a, a, a, a, a, a, a, a, a, n, e, h, nh, full, 0.5, a, a, a, a, a, a,
                                a, a, 5 * h, a, a, None)


def test_impossible_arguments_are_refused_before_any_launch():
    lib = L.load()
    for call in (_fwd, _bwd):
        for n, e, h, nh, v in ((-1, 0, 64, 4, 60), (4, -1, 64, 4, 60), (4, 2, 0, 4, 60), (4, 2, 64, 0, 60), (4, 2, 64, 4, 0),
                               (4, 2, 64, 5, 60), (4, 2, 24, 16, 60)):
            assert call(lib, n, e, h, nh, v) == -1, (call.__name__, n, e, h, nh, v)          # sizes, H % nh
            assert b'invalid argument' in lib.i3d_last_error()
        assert call(lib, 4, 2, 64, 4, 60, ptrs=0) == -1                                       # null pointers
        assert b'null pointer' in lib.i3d_last_error()
        # valid but outside the lane map / the code table: not taken, nothing launched
        assert call(lib, 4, 2, 130, 2, 60) == L.NOT_TAKEN                                     # dh = 65
        assert call(lib, 4, 2, 1024, 16, 60) == L.NOT_TAKEN                                   # 16 heads x 64 lanes
        assert call(lib, 4, 2, 64, 4, 257) == L.NOT_TAKEN
        assert call(lib, 0, 0, 64, 4, 60) == 0                                                # N = 0: nothing to do
    strides = L.int_array([1, 5, 30])
    assert lib.i3d_san_edge_codes(8, 8, 8, -1, 3, strides, 8, 8, None) == -1 and lib.i3d_san_edge_codes(8, 8, 8, 4, 9, strides, 8, 8, None) == -1
    assert lib.i3d_san_edge_codes(8, 8, 8, 4, 3, strides, None, 8, None) == -1 and lib.i3d_san_edge_codes(8, None, 8, 4, 3, strides, 8, 8, None) == -1
    assert lib.i3d_san_edge_codes(None, None, None, 0, 3, strides, None, None, None) == 0
    assert lib.i3d_san_attn_takes(64, 4, 60) == 0 and lib.i3d_san_attn_takes(200, 10, 60) == 0
    assert lib.i3d_san_attn_takes(512, 8, 256) == 0 and lib.i3d_san_attn_takes(8, 1, 1) == 0
    assert lib.i3d_san_attn_takes(64, 5, 60) == -1
    chunk = lib.i3d_san_attn_chunk_edges()
    assert lib.i3d_san_attn_bwd_partial_floats(chunk + 1, 16, 60) == 4 * (2 + 60) * 16
    assert lib.i3d_san_attn_bwd_partial_floats(-1, 16, 60) == 0 and lib.i3d_san_attn_bwd_partial_floats(5, 16, 257) == 0


# ---- the kernel test's inputs (tests/test_gpu_san.py) ------------------------------------------------------------------------------
@pytest.mark.parametrize('H, nh', R.SHAPES)
@pytest.mark.parametrize('full_graph', [True, False])
def test_kernel_cases_saturate_as_stated(H, nh, full_graph):
    import test_gpu_san as T
    t, grad, idx, index, N = R.make_case(H, nh, full_graph, *T.CASE[(H, nh, full_graph)])
    ref = R.run(t, grad, idx, nh, 0.5, full_graph, torch.float64)
    s = ref['s'].abs()
    share = float((s > 5).double().mean())
    assert 0.10 <= share <= 0.40, share
    assert float((s - 5).abs().min()) > 1e-3
    deg = np.diff(index.in_ptr.numpy())
    if full_graph:
        assert sorted(set(deg.tolist())) == [0, 1, 2, 16, 32, 69]
        fake_codes = idx['code'][~idx['real']]
        assert float((fake_codes == 0).double().mean()) > 0.9
    else:
        assert 0 in deg and deg.max() <= 3
    assert int((idx['code'] == R.ABSENT_CODE).sum()) == 0


# ---- the composed path in torch against the fixture ---------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', sorted(GS.CONFIGS))
def test_composed_path_on_the_host_matches_the_fixture(cfg, monkeypatch):
    z = load('san.npz')
    monkeypatch.setattr(san, 'FUSED_ATTENTION', False)
    model = model_of(z, cfg)
    g = batch_of(z, cfg)
    before = g.ndata['pos_enc'].clone()
    check_against_fixture(model, g, z, cfg, 'host')
    assert all(layer.attention.path == 'composed' for layer in model.gnn.layers)
    assert torch.equal(torch.nan_to_num(g.ndata['pos_enc'], nan=7.0), torch.nan_to_num(before, nan=7.0))      # read through a copy


def test_fused_attention_on_the_host_is_an_error_not_a_fallback():
    z = load('san.npz')
    model = model_of(z, 'c')
    with pytest.raises(RuntimeError, match='FUSED_ATTENTION'):
        model(batch_of(z, 'c'))


def test_fixture_holds_what_the_tests_read():
    z = load('san.npz')
    for cfg in sorted(GS.CONFIGS):
        mols = mols_from_npz(z, f'{cfg}/mol')
        assert any(m.n_atoms > 64 for m in mols) and any(m.n_atoms == 1 for m in mols)
        n = sum(m.n_atoms for m in mols)
        kw = GS.CONFIGS[cfg]
        assert z[f'{cfg}/feat'].shape == (n, kw['GT_out_dim']) and z[f'{cfg}/out'].shape == (len(mols), kw['target_dim'])
        assert z[f'{cfg}/pos_enc'].shape == (n, 10, 2) and np.isnan(z[f'{cfg}/pos_enc']).any()
        assert float(z[f'{cfg}/ref_err/out']) < 1e-4
        if cfg != 'd':
            assert len(z[f'{cfg}/grad_names']) == len(z[f'{cfg}/ref_err/grad']) > 0
    assert 0.05 < float(z['b/saturated']) < 0.5
