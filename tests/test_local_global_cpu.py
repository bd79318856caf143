"""Local-global pre-training without a GPU: the fp64 oracle of the loss that tests/test_gpu_local_global.py compares the kernels with
is pinned to the reference fixture (tests/golden/gen_golden_local_global.py), PNALocal's state_dict layout, the refusals of the loss
classes and of the C entry points, and the exported names."""
import importlib

import pytest
import torch

from helpers import amd, load, sd_from_npz

import gen_golden_local_global as GL

L = importlib.import_module('3dinfomax_amd._lib')
ops = importlib.import_module('3dinfomax_amd.ops')
losses = importlib.import_module('3dinfomax_amd.losses')
NEW_NAMES = (amd.NTXentLocalGlobal, amd.NTXentGlobalLocal, amd.PNALocal)      # nothing in this file is meaningful without them


def lg_oracle(zn, zg, nodes_per_graph, tau, norm=True, eps=1e-10, dtype=torch.float64, upstream=1.0):
    """-> loss, dzn, dzg of  upstream * mean_i -log(e_{i,g(i)} / sum_{j != g(i)} e_ij),  e = exp(s' / tau),
    s'_ij = zn_i . zg_j / (|zn_i| |zg_j| + eps) (norm=False: the dot product) in `dtype` on the CPU.  g comes from a segment index
    (repeat_interleave), the negatives are summed with the positive's column set to zero: no mask loop, no rowsum - pos."""
    zn = torch.as_tensor(zn).detach().cpu().to(dtype).requires_grad_(True)
    zg = torch.as_tensor(zg).detach().cpu().to(dtype).requires_grad_(True)
    counts = torch.as_tensor(nodes_per_graph, dtype=torch.int64).cpu()
    seg = torch.repeat_interleave(torch.arange(zg.shape[0]), counts)[:, None]
    assert seg.shape[0] == zn.shape[0]
    sim = zn @ zg.T
    if norm:
        sim = sim / (zn.norm(dim=1)[:, None] * zg.norm(dim=1)[None, :] + eps)
    e = torch.exp(sim / tau)
    pos = e.gather(1, seg).squeeze(1)
    neg = e.scatter(1, seg, 0.0).sum(dim=1)
    loss = -torch.log(pos / neg).mean()
    (loss * upstream).backward()
    return loss.detach(), zn.grad, zg.grad


@pytest.mark.parametrize('case', sorted(GL.LOSS_CASES))
def test_oracle_reproduces_the_reference_fp64_run(case):
    """loss to 1e-12 relative; the gradients row by row (a zero node row carries 1e10 next to 1e-3) to 1e-9"""
    z = load('local_global.npz')
    p = f'loss/{case}/'
    c = GL.LOSS_CASES[case]
    assert z[p + 'nodes_per_graph'].tolist() == c['nodes_per_graph'] and z[p + 'zn'].shape == (sum(c['nodes_per_graph']), c['dim'])
    loss, dzn, dzg = lg_oracle(z[p + 'zn'], z[p + 'zg'], z[p + 'nodes_per_graph'], c['tau'])
    ref = float(z[p + 'loss64'])
    print(f'{case}: oracle {float(loss):.15f} reference fp64 {ref:.15f}')
    assert abs(float(loss) - ref) <= 1e-12 * abs(ref)
    assert GL.row_rel_err(dzn, z[p + 'dzn64']) < 1e-9
    assert GL.row_rel_err(dzg, z[p + 'dzg64']) < 1e-9
    # the fixture's own fp32 figures are what the docstring of the generator says they are
    assert 2.0 ** -24 <= float(z[p + 'ref_err/loss']) < 1e-6 and float(z[p + 'ref_err/loss_raw']) <= float(z[p + 'ref_err/loss'])
    assert 0 < float(z[p + 'ref_err/dzn']) < 2e-6 and 0 < float(z[p + 'ref_err/dzg']) < 2e-6


def test_fixture_cases_hold_what_they_are_for():
    z = load('local_global.npz')
    zero_rows = {c: (torch.from_numpy(z[f'loss/{c}/zn']).abs().sum(1) == 0).nonzero().flatten().tolist() for c in GL.LOSS_CASES}
    assert len(zero_rows['b2']) == 1 and zero_rows['zero'] == [3] and zero_rows['long'] == []
    assert abs(z['loss/b2/dzn64']).max() > 1e9 and abs(z['loss/zero/dzn64']).max() > 1e8       # finite, of order 1 / eps
    assert all(torch.isfinite(torch.from_numpy(z[f'loss/{c}/{q}'])).all() for c in GL.LOSS_CASES for q in ('dzn64', 'dzg64', 'dzg'))
    assert 1 in z['model/mol_n_atoms'].tolist() and max(z['model/mol_n_atoms']) > 64


def test_oracle_is_finite_where_rowsum_minus_pos_is_not():
    """case 7 of the GPU tests: aligned positives e^10, negatives e^-10; log(2) - 20 in fp64 and in fp32, while the fp32 rowsum - pos
    is exactly zero"""
    zg = torch.tensor([[1.0, 2.0, -1.0, 0.5]]).repeat(3, 1)
    zg[1:] = -zg[0]
    zn = zg[0:1].repeat(2, 1)                      # two nodes of graph 0; graphs 1 and 2 hold the negated embedding
    for dtype in (torch.float64, torch.float32):
        sim = (zn[:2].to(dtype) @ zg.to(dtype).T) / (zn[:2].to(dtype).norm(dim=1)[:, None] * zg.to(dtype).norm(dim=1)[None, :] + 1e-10)
        e = torch.exp(sim / 0.1)
        rows = -torch.log(e[:, 0] / (e[:, 1] + e[:, 2]))
        assert torch.allclose(rows, torch.full((2,), torch.log(torch.tensor(2.0)).item() - 20, dtype=dtype), rtol=1e-5)
    e32 = torch.exp(torch.tensor([10.0, -10.0, -10.0]))
    assert float(e32.sum() - e32[0]) == 0.0           # what the kernels must not compute
    loss, _, _ = lg_oracle(zn[:2], zg, [2, 0, 0], 0.1)
    assert abs(float(loss) - (torch.log(torch.tensor(2.0, dtype=torch.float64)).item() - 20)) < 1e-8


def test_pna_local_state_dict_matches_the_reference_layout():
    z = load('local_global.npz')
    ref = sd_from_npz(z, 'model/sd')
    model = amd.PNALocal(**GL.MODEL)
    sd = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype, k
    model.load_state_dict(ref, strict=True)
    assert torch.equal(model.state_dict()['projection_head.fully_connected.1.linear.weight'],
                       ref['projection_head.fully_connected.1.linear.weight'])
    assert set(dict(model.named_children())) == {'node_gnn', 'projection_head'}
    # the reference's positional order and swallowed kwargs
    other = amd.PNALocal(0, 0, 16, 8, ['mean'], ['identity'], propagation_depth=1, avg_d=1.0, device='cpu', readout_aggregators=['min'])
    assert other.projection_head.fully_connected[0].linear.out_features == 16        # readout_hidden_dim=None: hidden_dim
    assert other.projection_head.fully_connected[0].batch_norm is not None and other.projection_head.fully_connected[1].batch_norm is None


def _no_library(monkeypatch):
    def boom():
        raise AssertionError('the library was loaded before the refusal')
    monkeypatch.setattr(L, 'load', boom)


@pytest.mark.parametrize('cls', ['NTXentLocalGlobal', 'NTXentGlobalLocal'])
def test_refusals_name_the_problem_before_any_device_work(cls, monkeypatch):
    _no_library(monkeypatch)
    loss = getattr(amd, cls)(tau=0.1)
    swap = cls == 'NTXentGlobalLocal'

    def call(zn, zg, npg):
        return loss(zg, zn, npg) if swap else loss(zn, zg, npg)

    zn, zg = torch.zeros(6, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match='nodes_per_graph is None'):
        call(zn, zg, None)
    with pytest.raises(ValueError, match='zg has 3 graph rows'):
        call(zn, zg, [3, 3])
    with pytest.raises(ValueError, match='zg has 3 graph rows'):
        call(zn, zg, torch.tensor([1, 2, 2, 1]))
    with pytest.raises(ValueError, match='sums to 7'):
        call(zn, zg, [3, 3, 1])
    with pytest.raises(ValueError, match='sums to 7'):
        call(zn, zg, torch.tensor([3, 3, 1]))
    with pytest.raises(ValueError, match='smallest entry -1'):
        call(zn, zg, [4, 3, -1])
    with pytest.raises(ValueError, match='no negatives'):
        call(zn, torch.zeros(1, 4), [6])
    with pytest.raises(ValueError, match='integers'):
        call(zn, zg, torch.tensor([2.0, 2.0, 2.0]))
    with pytest.raises(NotImplementedError, match='fp32'):
        call(zn.double(), zg.double(), [2, 2, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        call(zn, zg, [2, 2, 2])
    with pytest.raises(ValueError, match='one width'):
        call(zn, torch.zeros(3, 5), [2, 2, 2])
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss.attach_group(group)
    with pytest.raises(NotImplementedError, match='more than one rank'):
        call(zn, zg, [2, 2, 2])


def test_constructor_signatures_are_the_reference_ones():
    a = amd.NTXentLocalGlobal()
    assert a.norm is True and a.tau == 0.5 and a._eps == 1e-10
    b = amd.NTXentGlobalLocal(norm=False, tau=0.2)
    assert b.ntxent_local_global.norm is False and b.ntxent_local_global.tau == 0.2
    with pytest.raises(TypeError):
        amd.NTXentLocalGlobal(uniformity_reg=0.1)          # the reference class takes norm and tau only


def test_entry_points_are_declared_exported_and_validate_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_lg_ntxent_scratch_floats', 'i3d_lg_ntxent_work_floats', 'i3d_lg_ntxent_fwd', 'i3d_lg_ntxent_bwd', 'i3d_lg_row_chunk'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_abi_version() == 2
    assert lib.i3d_lg_row_chunk() == ops.LG_ROW_CHUNK
    n, b, d = 9000, 500, 256
    assert lib.i3d_lg_ntxent_scratch_floats(n, b) >= n * b + 3 * n + b
    chunks = -(-n // ops.LG_ROW_CHUNK)
    assert lib.i3d_lg_ntxent_work_floats(n, b, d) >= n * b + chunks * b + (n // 512) * b * d
    # argument validation happens on the host before any launch: no GPU needed.  Non-null dummies: the sizes are what is refused
    one = 1
    fwd = lambda n, b, d, tau=0.1, p=one: lib.i3d_lg_ntxent_fwd(p, p, p, n, b, d, tau, 1e-10, 1, p, p, None)       # noqa: E731
    bwd = lambda n, b, d, tau=0.1, p=one: lib.i3d_lg_ntxent_bwd(p, p, p, n, b, d, tau, 1e-10, 1, p, None, p, p, p, None)   # noqa: E731
    for fn in (fwd, bwd):
        assert fn(8, 1, 4) == -1 and b'no negative' in lib.i3d_last_error()
        assert fn(8, 0, 4) == -1 and b'no negative' in lib.i3d_last_error()
        assert fn(0, 2, 4) == -1 and b'node rows' in lib.i3d_last_error()
        assert fn(-3, 2, 4) == -1 and b'node rows' in lib.i3d_last_error()
        assert fn(8, -2, 4) == -1 and fn(8, 2, 0) == -1 and b'feature width' in lib.i3d_last_error()
        assert fn(8, 2, -4) == -1
        assert fn(8, 2, 4, 0.0) == -1 and b'tau' in lib.i3d_last_error()
        assert fn(8, 2, 4, 0.1, None) == -1 and b'null' in lib.i3d_last_error()
        assert fn(1 << 20, 1 << 12, 4) == -1 and b'31 bits' in lib.i3d_last_error()
    assert lib.i3d_lg_ntxent_scratch_floats(0, 4) == 0 and lib.i3d_lg_ntxent_work_floats(4, 4, 0) == 0


def test_names_import_from_the_package_and_the_alias():
    alias = importlib.import_module('infomax3d_amd')
    pna_local = importlib.import_module('3dinfomax_amd.pna_local')
    for name in ('NTXentLocalGlobal', 'NTXentGlobalLocal', 'PNALocal'):
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(alias, name) is getattr(amd, name)
    assert amd.NTXentLocalGlobal is losses.NTXentLocalGlobal and amd.NTXentGlobalLocal is losses.NTXentGlobalLocal
    assert amd.PNALocal is pna_local.PNALocal and amd.pna_local is pna_local
    launcher = importlib.import_module('launch_reference')
    rebound = launcher.plugin_names()                # what the launcher binds into the reference's train module
    assert rebound['PNALocal'] is amd.PNALocal and rebound['NTXentLocalGlobal'] is amd.NTXentLocalGlobal
