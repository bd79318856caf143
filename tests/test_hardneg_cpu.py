"""InfoNCE / InfoNCEHard / NTXentHard / NTXentExtraNegatives / NTXentShuffled on the host: fp64 restatements of the five formulas against
the reference's own fp64 results (fixture: tests/golden/gen_golden_hardneg.py) - which pins that the gradient runs through the importance
weights of the hard pair -, the clamp conditions of the fixture, the plugin surface, and the refusals that fire before any library call."""
import importlib
import inspect

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_hardneg as GH

launcher = importlib.import_module('launch_reference')
NAMES = dict(GH.LOSSES)
CASES = GH.all_cases()
CASE_IDS = [GH.case_prefix(*c).strip('/').replace('/', '-') for c in CASES]
HARD_CASES = [c for c in CASES if c[0] in GH.HARD]
HARD_IDS = [GH.case_prefix(*c).strip('/').replace('/', '-') for c in HARD_CASES]


def case_setup(z, key, shape, tag):
    """(z1, z2 as the loss is called with them, constructor kwargs, U) of a fixture case"""
    kw, U = next((k, u) for t, k, u in GH.parameter_sets(key) if t == tag)
    B, D = shape
    z1, z2 = GH.case_inputs(z[f'in/{B}x{D}/z1'], z[f'in/{B}x{D}/z2'], z[f'in/{B}x{D}/x'], GH.DEFAULT_NORM[key], U)
    return z1, z2, kw, U


def _cosines(z1, z2, norm):
    s = z1 @ z2.T
    if norm:
        s = s / (z1.norm(dim=1)[:, None] * z2.norm(dim=1)[None, :])
    return s


def restated_loss(key, z1, z2, norm=True, tau=0.5, tau_plus=0.1, beta=0.5, extra_negatives_weight=1, perm=None, detach_weights=False):
    """the formulas of csrc/hardneg.hip as a torch expression in the dtype of z1: S, A and C are sums over the columns other than the
    positive's, never `row sum - positive`"""
    B, D = z1.shape
    if key == 'shuffled':
        z2 = z2[torch.as_tensor(perm)]
    other = z2[:B]
    P = torch.exp(_cosines(z1, other, norm) / tau)
    off = ~torch.eye(B, dtype=torch.bool)
    pos = torch.diagonal(P)
    S = (P * off).sum(dim=1)
    if key == 'infonce':
        l = torch.log(S + pos) - torch.log(pos)
    elif key == 'shuffled':
        l = torch.log(S) - torch.log(pos)
    elif key == 'extra':
        x = z2[B:].reshape(B, -1, D)
        sx = torch.einsum('ik,iuk->iu', z1, x)
        if norm:
            sx = sx / (z1.norm(dim=1)[:, None] * x.norm(dim=2))
        l = torch.log(S + extra_negatives_weight * torch.exp(sx / tau).sum(dim=1)) - torch.log(pos)
    else:
        Pb = torch.exp(beta * _cosines(z1, other, norm) / tau)
        if detach_weights:
            Pb = Pb.detach()
        n = B - 1
        A, C = (Pb * off).sum(dim=1), (P * Pb * off).sum(dim=1)
        ng = (n * C / A - tau_plus * n * pos) / (1 - tau_plus)
        ngc = torch.clamp(ng, min=n * float(np.exp(-1.0 / tau)))
        l = (torch.log(pos + ngc) if key == 'infonce_hard' else torch.log(ngc)) - torch.log(pos)
    return l.mean()


def restated(key, z1, z2, dtype=torch.float64, **kw):
    """-> (loss, dz1, dz2) of the restatement in `dtype`"""
    a = torch.as_tensor(z1).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(dtype).clone().requires_grad_(True)
    loss = restated_loss(key, a, b, **kw)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def restated_kwargs(key, kw, perm=None):
    """constructor kwargs of a case -> kwargs of `restated`, the class's defaults filled in"""
    out = dict(norm=GH.DEFAULT_NORM[key], tau=0.5)
    out.update(GH.DEFAULT_HARD.get(key, {}))
    out.update(kw)
    if key == 'shuffled':
        out['perm'] = perm
    return out


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_fp64_restatement_reproduces_the_reference(case):
    """loss at 1e-10; gradients at 1e-9 of their largest entry (the fixture stores them in steps of 4.7e-10 of it)"""
    key, shape, tag = case
    z = load('hardneg.npz')
    p = GH.case_prefix(key, shape, tag)
    z1, z2, kw, U = case_setup(z, key, shape, tag)
    assert z2.shape == (shape[0] * (1 + U), shape[1])
    perm = z[p + 'perm'] if key == 'shuffled' else None
    loss, g1, g2 = restated(key, z1, z2, **restated_kwargs(key, kw, perm))
    assert z[p + 'loss64'].dtype == np.float64
    assert abs(loss.item() - float(z[p + 'loss64'])) <= 1e-10 * max(1.0, abs(float(z[p + 'loss64'])))
    for name, got in (('dz1', g1), ('dz2', g2)):
        ref = torch.from_numpy(GH.decode(z, p, name))
        assert ref.shape == got.shape
        assert (got - ref).abs().max().item() <= 1e-9 * float(z[p + name + '_scale']), name
    assert z[p + 'err32'].shape == (3,) and (z[p + 'err32'] >= 0).all() and (z[p + 'err32'] < 1e-4).all()


@pytest.mark.parametrize('case', HARD_CASES, ids=HARD_IDS)
def test_fixture_inputs_meet_the_clamp_conditions(case):
    """between 20 % and 80 % of the rows clamped in every tau = 0.1 case with B >= 5; every row further than 1e-3 from the clamp, so every
    precision takes the same branch; nothing clamped at NTXentHard's defaults"""
    key, shape, tag = case
    z = load('hardneg.npz')
    p = GH.case_prefix(key, shape, tag)
    z1, z2, kw, _ = case_setup(z, key, shape, tag)
    share, margin = GH.clamp_figures(z1, z2, GH.DEFAULT_NORM[key], **dict(GH.DEFAULT_HARD[key], **kw))
    assert share == float(z[p + 'clamped']) and abs(margin - float(z[p + 'margin'])) <= 1e-12
    assert margin > GH.MARGIN
    if tag != 'default' and shape[0] >= 5:
        assert 0.2 <= share <= 0.8
    if tag == 'default' and key == 'ntxent_hard':
        assert share == 0.0


def test_the_gradient_runs_through_the_importance_weights():
    """with P^beta detached the fp64 gradient is another one: the reference differentiates through imp"""
    z = load('hardneg.npz')
    case = ('ntxent_hard', (5, 13), 'tau0.1_beta1')
    p = GH.case_prefix(*case)
    z1, z2, kw, _ = case_setup(z, *case)
    ref = GH.decode(z, p, 'dz1')
    _, through, _ = restated('ntxent_hard', z1, z2, **restated_kwargs('ntxent_hard', kw))
    _, detached, _ = restated('ntxent_hard', z1, z2, detach_weights=True, **restated_kwargs('ntxent_hard', kw))
    assert np.abs(through.numpy() - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(detached.numpy() - ref).max() > 1e-2 * np.abs(ref).max()


@pytest.mark.parametrize('shape', GH.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_fixture_inputs_and_permutations_regenerate(shape):
    B, D = shape
    z = load('hardneg.npz')
    for name, t in zip(('z1', 'z2', 'x'), GH.base_inputs(B, D)):
        assert np.array_equal(z[f'in/{B}x{D}/{name}'], t.numpy())
    for tag, _, _ in GH.parameter_sets('shuffled'):
        p = GH.case_prefix('shuffled', shape, tag)
        assert int(z[p + 'seed']) == GH.shuffle_seed(B, D, tag)
        torch.manual_seed(int(z[p + 'seed']))
        assert np.array_equal(torch.randperm(B).numpy(), z[p + 'perm'])


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    names = launcher.plugin_names()
    for name in NAMES.values():
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(amd, name) is getattr(alias, name) is getattr(losses, name) is names[name]
        assert issubclass(getattr(amd, name), losses._NTXentBase) and getattr(amd, name)._eps == 0.0


def test_the_launcher_binds_the_five_names():
    namespace = {name: object() for name in NAMES.values()}
    replaced = launcher.rebind(namespace, launcher.plugin_names())
    for name in NAMES.values():
        assert name in replaced and namespace[name] is getattr(amd, name)


REFERENCE_SIGNATURES = {
    'InfoNCE': dict(norm=True, tau=0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0),
    'InfoNCEHard': dict(norm=False, tau=0.5, tau_plus=0.1, beta=0.5),
    'NTXentHard': dict(norm=True, tau=0.5, tau_plus=0.1, beta=0.1),
    'NTXentExtraNegatives': dict(norm=True, tau=0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0, extra_negatives_weight=1),
    'NTXentShuffled': dict(norm=True, tau=0.5),
}


@pytest.mark.parametrize('name', sorted(REFERENCE_SIGNATURES))
def test_constructor_signatures_and_defaults_are_the_reference_s(name):
    """names, order and defaults of reference commons/losses.py:898, :976, :1007, :1047, :1087"""
    cls = getattr(amd, name)
    params = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != 'self']
    assert [(q.name, q.default) for q in params] == list(REFERENCE_SIGNATURES[name].items())
    d = cls()
    for k, v in REFERENCE_SIGNATURES[name].items():
        assert getattr(d, k) == v
    values = [False, 0.1] + [0.25 + i for i in range(len(params) - 2)]
    c = cls(*values)
    assert [getattr(c, q.name) for q in params] == values


def _no_library(monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)


def test_extra_negatives_refuse_a_bad_row_count_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    ops = importlib.import_module('3dinfomax_amd.ops')
    loss = amd.NTXentExtraNegatives(tau=0.1)
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 8), torch.zeros(13, 8))
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 8), torch.zeros(2, 8))                  # fewer rows than the batch
    with pytest.raises(ValueError, match='width'):
        loss(torch.zeros(4, 8), torch.zeros(8, 7))
    with pytest.raises(NotImplementedError, match=f'0..{ops.HARDNEG_MAX_EXTRA}'):
        loss(torch.zeros(1, 2), torch.zeros(ops.HARDNEG_MAX_EXTRA + 2, 2))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(4, 8, dtype=torch.float64), torch.zeros(8, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss(torch.zeros(4, 8), torch.zeros(4, 8))                  # U = 0 is a valid layout; CPU tensors are not


@pytest.mark.parametrize('name', ['InfoNCEHard', 'NTXentHard'])
def test_hard_losses_refuse_a_global_batch_of_one(name, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match='global batch of 1'):
        getattr(amd, name)()(torch.zeros(1, 8), torch.zeros(1, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        getattr(amd, name)()(torch.zeros(2, 8), torch.zeros(2, 8))  # two rows pass that check
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        amd.InfoNCE()(torch.zeros(1, 8), torch.zeros(1, 8))         # InfoNCE has no such condition


def test_shuffled_refuses_a_group_of_more_than_one_rank(monkeypatch):
    _no_library(monkeypatch)
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss = amd.NTXentShuffled(tau=0.1).attach_group(group)
    state = torch.random.get_rng_state()
    with pytest.raises(NotImplementedError, match='NTXentShuffled'):
        loss(torch.zeros(4, 8), torch.zeros(4, 8))
    assert torch.equal(torch.random.get_rng_state(), state)         # refused before the permutation is drawn


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    ops = importlib.import_module('3dinfomax_amd.ops')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_hardneg_max_extra', 'i3d_hardneg_norms', 'i3d_hardneg_fwd', 'i3d_hardneg_bwd', 'i3d_hardneg_loss_scratch_floats',
                 'i3d_hardneg_loss_fwd', 'i3d_hardneg_loss_bwd'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_hardneg_max_extra() == ops.HARDNEG_MAX_EXTRA == 256
    assert ops.HARDNEG_MODES == {'infonce': 0, 'ntxent_hard': 1, 'infonce_hard': 2, 'extra_negatives': 3}
    # n1 | n2 | coef | stats (fp64) | xdot | xn | sim, every part rounded up to four floats
    assert lib.i3d_hardneg_loss_scratch_floats(5, 7, 3) == 8 + 8 + 20 + 52 + 16 + 16 + 36
    assert lib.i3d_hardneg_loss_scratch_floats(64, 64, 0) == 64 + 64 + 256 + 640 + 64 * 64
    # argument validation happens on the host before any launch: no GPU needed
    fwd = lambda mode, b1, b2, n_extra, pos_offset, tau, tau_plus: lib.i3d_hardneg_loss_fwd(
        mode, None, None, None, b1, b2, n_extra, 8, pos_offset, 1, tau, tau_plus, 0.5, 1.0, 1.0, None, None, None)
    assert fwd(4, 4, 4, 0, 0, 0.5, 0.1) == -1 and b'mode' in lib.i3d_last_error()
    assert fwd(1, 1, 1, 0, 0, 0.5, 0.1) == -1 and b'no negatives' in lib.i3d_last_error()
    assert fwd(2, 4, 4, 0, 0, 0.5, 1.0) == -1 and b'tau_plus' in lib.i3d_last_error()
    assert fwd(0, 4, 4, 0, 0, 0.0, 0.1) == -1 and b'tau' in lib.i3d_last_error()
    assert fwd(0, 4, 6, 0, 3, 0.5, 0.1) == -1 and b'out of range' in lib.i3d_last_error()
    assert fwd(0, 4, 4, 1, 0, 0.5, 0.1) == -1 and b'extra' in lib.i3d_last_error()
    assert fwd(3, 4, 4, 257, 0, 0.5, 0.1) == -1 and b'0..256' in lib.i3d_last_error()
    assert fwd(3, 4, 4, 2, 0, 0.5, 0.1) == -1 and b'bad arguments' in lib.i3d_last_error()      # valid shape, null pointers
