"""NTXentMinimumMatching / NTXentMaximumSimilarity / NTXentMultiplePositivesV2 / NTXentMultiplePositivesV3 on the host: fp64 restatements
of the four formulas against the reference's own fp64 results (fixture: tests/golden/gen_golden_confmatch.py) - which pins the positive
of the minimum-matching loss, taken over EVERY column molecule, and V2's negatives, conformer 0 only -, the selection gaps of the
fixture, the plugin surface, and the refusals that fire before any library call."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_confmatch as GC

launcher = importlib.import_module('launch_reference')
NAMES = dict(GC.LOSSES)
MATCHING, PER_CONFORMER = sorted(GC.MATCHING), sorted(GC.PER_CONFORMER)
CASES = list(GC.ALL_CASES)
CASE_IDS = [GC.case_tag(*c, n) for c, n in CASES]


def _block_similarity(z1, z2, norm):
    """s'[i, j, l, u] of z1 [B, C D] and z2 [B C, D]"""
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.reshape(B, -1, D), z2.reshape(B, -1, D)
    S = torch.einsum('ilk,juk->ijlu', a, b)
    if norm:
        S = S / (a.norm(dim=2)[:, None, :, None] * b.norm(dim=2)[None, :, None, :])
    return S


def _off_diagonal_sum(M):
    """sum_{j != i} M[i, j, ...] over the pairs themselves, not sum - diagonal"""
    B = M.shape[0]
    off = ~torch.eye(B, dtype=torch.bool)
    return (M * off.reshape(B, B, *([1] * (M.dim() - 2)))).sum(dim=1)


def min_restated(z1, z2, tau, norm=True, own_columns_only=False):
    """den_i = sum_{j != i} exp(min of block (i, j) / tau); pos_i = exp(max over ALL j and l of s'[(i, l), (j, l)] / tau) - with
    own_columns_only the max runs over j = i alone, which is NOT what the reference computes"""
    S = _block_similarity(z1, z2, norm)
    B = S.shape[0]
    matched = torch.diagonal(S, dim1=2, dim2=3)                       # [B, B, C]
    best = matched[torch.arange(B), torch.arange(B)].amax(dim=1) if own_columns_only else matched.amax(dim=(1, 2))
    den = _off_diagonal_sum(torch.exp(S.amin(dim=(2, 3)) / tau))
    return -torch.log(torch.exp(best / tau) / den).mean()


def max_restated(z1, z2, tau, norm=True):
    """den_i = sum_{j != i} exp(max of block (i, j) / tau), pos_i = exp(max of block (i, i) / tau)"""
    M = torch.exp(_block_similarity(z1, z2, norm).amax(dim=(2, 3)) / tau)
    return -torch.log(torch.diagonal(M) / _off_diagonal_sum(M)).mean()


def _row_similarity(z1, z2, norm):
    """s'[i, j, u] of z1 [B, D] and z2 [B C, D]"""
    B, D = z1.shape
    b = z2.reshape(B, -1, D)
    S = torch.einsum('ik,juk->iju', z1, b)
    if norm:
        S = S / (z1.norm(dim=1)[:, None, None] * b.norm(dim=2)[None, :, :])
    return S


def v2_restated(z1, z2, tau, norm=True):
    """pos_i = sum_u P[i, (i, u)], den_i = sum_{j != i} P[i, (j, 0)]: conformer 0 only"""
    P = torch.exp(_row_similarity(z1, z2, norm) / tau)
    B = P.shape[0]
    pos = P[torch.arange(B), torch.arange(B)].sum(dim=1)
    return -torch.log(pos / _off_diagonal_sum(P[:, :, 0])).mean()


def v3_restated(z1, z2, tau, norm=True):
    """one term per (i, u): pos = P[i, (i, u)], den = sum_{j != i} P[i, (j, u)]; the mean over the B C terms"""
    P = torch.exp(_row_similarity(z1, z2, norm) / tau)
    B = P.shape[0]
    return -torch.log(P[torch.arange(B), torch.arange(B)] / _off_diagonal_sum(P)).mean()


RESTATED = {'min': min_restated, 'max': max_restated, 'v2': v2_restated, 'v3': v3_restated}


def restated(key, z1, z2, tau, dtype=torch.float64, **kw):
    """-> (loss, dz1, dz2) of the restatement in `dtype`"""
    a = torch.as_tensor(z1).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(dtype).clone().requires_grad_(True)
    loss = RESTATED[key](a, b, tau, **kw)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def gapped_inputs(B, C, D, scale=1.0, norm=True):
    """inputs of the matching losses at a shape outside the fixture, found by the fixture's own rule: the first seed of 1000 B + 10 C + D,
    + 100000, ... whose selections are more than 1e-4 apart in fp64 -> (z1, z2, seed, gap)"""
    return GC.gapped_matching_inputs(B, C, D, False, scale, norm)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('key', sorted(NAMES))
def test_fp64_restatement_reproduces_the_reference(key, case):
    (B, C, D), near = case
    z = load('confmatch.npz')
    p = f'{key}/{GC.case_tag(B, C, D, near)}/'
    assert z[p + 'z1'].shape == ((B, C * D) if key in GC.MATCHING else (B, D)) and z[p + 'z2'].shape == (B * C, D)
    loss, g1, g2 = restated(key, z[p + 'z1'], z[p + 'z2'], GC.TAU)
    for name, got, ref in (('loss', loss, z[p + 'loss64']), ('dz1', g1, z[p + 'dz1_64']), ('dz2', g2, z[p + 'dz2_64'])):
        ref = torch.as_tensor(ref)
        assert ref.dtype == torch.float64
        err = (got - ref).abs().max().item()
        assert err <= 1e-10 * max(1.0, ref.abs().max().item()), (name, err)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_fixture_inputs_meet_the_selection_condition(case):
    """every selection of the matching losses is decided by more than 1e-4 in fp64: the selected entries, and with them the gradients,
    are the same in every precision"""
    (B, C, D), near = case
    z = load('confmatch.npz')
    for key in MATCHING:
        p = f'{key}/{GC.case_tag(B, C, D, near)}/'
        gap = GC.selection_gap(z[p + 'z1'], z[p + 'z2'])
        assert gap > GC.GAP and abs(gap - float(z[p + 'gap'])) <= 1e-12
        z1, z2 = GC.matching_inputs(B, C, D, near, int(z[p + 'seed']))
        assert np.array_equal(z1.numpy(), z[p + 'z1']) and np.array_equal(z2.numpy(), z[p + 'z2'])
    z = load('confmatch.npz')
    assert float(z['e2e/min/gap']) > GC.GAP and GC.selection_gap(z['e2e/min/z1'], z['e2e/min/z2']) > GC.GAP


def test_the_positive_of_minimum_matching_runs_over_every_column_molecule():
    """the reference's amax over the matched entries takes dim=(1, 2): restricted to the molecule's own columns the loss is another number"""
    z = load('confmatch.npz')
    p = f'min/{GC.case_tag(5, 3, 24)}/'
    z1, z2 = torch.from_numpy(z[p + 'z1']).double(), torch.from_numpy(z[p + 'z2']).double()
    assert abs(min_restated(z1, z2, GC.TAU).item() - float(z[p + 'loss64'])) < 1e-10
    assert abs(min_restated(z1, z2, GC.TAU, own_columns_only=True).item() - float(z[p + 'loss64'])) > 1e-3


def test_v2_takes_its_negatives_from_conformer_zero_only():
    z = load('confmatch.npz')
    p = f'v2/{GC.case_tag(5, 3, 24)}/'
    g2 = z[p + 'dz2_64'].reshape(5, 3, 24)
    z1, z2 = torch.from_numpy(z[p + 'z1']).double(), torch.from_numpy(z[p + 'z2']).double().requires_grad_(True)
    P = torch.exp(_row_similarity(z1, z2, True) / GC.TAU)
    own = -torch.log(P[torch.arange(5), torch.arange(5)].sum(dim=1)).mean()          # the positives' part alone
    g_own, = torch.autograd.grad(own, z2)
    assert np.abs(g2[:, 1:] - g_own.reshape(5, 3, 24)[:, 1:].numpy()).max() < 1e-12
    assert np.abs(g2[:, 0] - g_own.reshape(5, 3, 24)[:, 0].numpy()).max() > 1e-6


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    names = launcher.plugin_names()
    for name in NAMES.values():
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(amd, name) is getattr(alias, name) is getattr(losses, name) is names[name]
        assert issubclass(getattr(amd, name), losses._Separate2DBase)


@pytest.mark.parametrize('name', sorted(NAMES.values()))
def test_constructor_defaults_are_the_reference_s(name):
    d = getattr(amd, name)()
    assert (d.norm, d.tau, d.uniformity_reg, d.variance_reg, d.covariance_reg) == (True, 0.5, 0, 0, 0)
    c = getattr(amd, name)(False, 0.1, 0, 0.5, 0)
    assert (c.norm, c.tau, c.variance_reg) == (False, 0.1, 0.5)
    k = getattr(amd, name)(norm=False, tau=0.3, uniformity_reg=0, variance_reg=0, covariance_reg=0)
    assert k.tau == 0.3 and k.norm is False


def _no_library(monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)


def _refuses_group_and_regularisers(name, monkeypatch, z1, z2):
    with pytest.raises(NotImplementedError, match='covariance_reg'):
        getattr(amd, name)(tau=0.1, covariance_reg=0.1)(z1, z2)
    with pytest.raises(NotImplementedError, match='uniformity_reg'):
        getattr(amd, name)(tau=0.1, uniformity_reg=0.1)(z1, z2)
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss = getattr(amd, name)(tau=0.1).attach_group(group)
    with pytest.raises(NotImplementedError, match=name):
        loss(z1, z2)


@pytest.mark.parametrize('key', MATCHING)
def test_matching_refusals_fire_on_cpu_tensors_before_any_library_call(key, monkeypatch):
    _no_library(monkeypatch)
    name = NAMES[key]
    loss = getattr(amd, name)(tau=0.1)
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 3 * 8 + 1), torch.zeros(12, 8))          # z1 is not C D wide
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 24), torch.zeros(13, 8))                # z2 rows not divisible by the batch
    with pytest.raises(NotImplementedError, match='1..8'):
        loss(torch.zeros(2, 9 * 4), torch.zeros(18, 4))             # nine conformers
    with pytest.raises(ValueError, match='no negatives'):
        loss(torch.zeros(1, 8), torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    _refuses_group_and_regularisers(name, monkeypatch, torch.zeros(4, 24), torch.zeros(12, 8))


@pytest.mark.parametrize('key', PER_CONFORMER)
def test_per_conformer_refusals_fire_on_cpu_tensors_before_any_library_call(key, monkeypatch):
    _no_library(monkeypatch)
    ops = importlib.import_module('3dinfomax_amd.ops')
    name = NAMES[key]
    loss = getattr(amd, name)(tau=0.1)
    with pytest.raises(ValueError, match='expected'):
        loss(torch.zeros(4, 3, 8), torch.zeros(12, 8))
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 3 * 8), torch.zeros(12, 8))             # the layout of the matching losses
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 8), torch.zeros(13, 8))
    cap = ops.PER_CONF_MAX_CONFORMERS
    assert cap >= 16
    with pytest.raises(NotImplementedError, match=f'1..{cap}'):
        loss(torch.zeros(2, 4), torch.zeros(2 * (cap + 1), 4))
    with pytest.raises(ValueError, match='no negatives'):
        loss(torch.zeros(1, 4), torch.zeros(3, 4))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    _refuses_group_and_regularisers(name, monkeypatch, torch.zeros(4, 8), torch.zeros(12, 8))


def test_variance_regulariser_follows_the_reference_on_the_views():
    """std_loss works on the 3-D views the reference hands it; for V2 / V3 z1 stays 2-D"""
    g = torch.Generator().manual_seed(0)
    v, w = torch.randn(4, 3, 8, generator=g), torch.randn(4, 8, generator=g)
    std = lambda x: torch.relu(1 - torch.sqrt(x.var(dim=0) + 1e-4)).mean()
    for key, name in NAMES.items():
        first = v if key in GC.MATCHING else w
        got = getattr(amd, name)(variance_reg=0.5, tau=0.1)._regularisers(torch.zeros(()), first, v)
        assert abs(got.item() - 0.5 * (std(first) + std(v)).item()) < 1e-6


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_conf_match_max_conformers', 'i3d_per_conf_max_conformers', 'i3d_conf_match_work_floats', 'i3d_conf_match_fwd',
                 'i3d_conf_match_bwd', 'i3d_per_conf_fwd', 'i3d_per_conf_bwd'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    ops = importlib.import_module('3dinfomax_amd.ops')
    assert lib.i3d_conf_match_max_conformers() == ops.SEP2D_MAX_CONFORMERS == 8
    assert lib.i3d_per_conf_max_conformers() == ops.PER_CONF_MAX_CONFORMERS == 64
    assert lib.i3d_conf_match_work_floats(256) == 4 * 65536 + 3 * 256 + 65536 // 4
    # argument validation happens on the host before any launch: no GPU needed
    nothing = [None] * 8
    assert lib.i3d_conf_match_fwd(None, None, None, 4, 9, 0, 0.1, *nothing) == -1 and b'1..8' in lib.i3d_last_error()
    assert lib.i3d_conf_match_fwd(None, None, None, 1, 2, 1, 0.1, *nothing) == -1 and b'two molecules' in lib.i3d_last_error()
    assert lib.i3d_conf_match_fwd(None, None, None, 4, 2, 2, 0.1, *nothing) == -1 and b'mode' in lib.i3d_last_error()
    assert lib.i3d_conf_match_bwd(*[None] * 9, 4, 9, 8, 0, 1, 0.1, *[None] * 5) == -1 and b'1..8' in lib.i3d_last_error()
    assert lib.i3d_conf_match_bwd(*[None] * 9, 1, 2, 8, 0, 1, 0.1, *[None] * 5) == -1 and b'two molecules' in lib.i3d_last_error()
    assert lib.i3d_per_conf_fwd(None, None, None, 4, 65, 0, 0.1, None, None, None, None) == -1 and b'1..64' in lib.i3d_last_error()
    assert lib.i3d_per_conf_fwd(None, None, None, 1, 3, 1, 0.1, None, None, None, None) == -1
    assert b'two molecules' in lib.i3d_last_error()
    assert lib.i3d_per_conf_bwd(*[None] * 5, 4, 65, 1, 0.1, *[None] * 5) == -1 and b'1..64' in lib.i3d_last_error()
    assert lib.i3d_per_conf_bwd(*[None] * 5, 4, 3, 1, 0.0, *[None] * 5) == -1 and b'tau' in lib.i3d_last_error()
