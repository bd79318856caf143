"""NTXentLikelihoodLoss, JSDMultiplePositivesLoss, PositiveProb and NegativeProb on the host: fp64 restatements of the closed forms of
csrc/gausspair.hip against the reference's own fp64 results (fixtures: tests/golden/gen_golden_gauss.py) - which pins the row / column
roles, the per-dimension mean of densities, the unbiased variance, where the 1e-5 sits and the conformer-major layout of the metrics -,
the plugin surface, the refusals that fire before any library call, and the C ABI's argument checks."""
import functools
import importlib
import inspect
import math

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_gauss as GG

launcher = importlib.import_module('launch_reference')
LOSSES = ('NTXentLikelihoodLoss', 'JSDMultiplePositivesLoss')
METRICS = ('PositiveProb', 'NegativeProb')
LIK_SETTINGS = [(c, e, tau) for c, e in GG.LIK_CASES for tau in GG.TAUS]
JSD_SETTINGS = [(c, e, norm) for c, e in GG.JSD_CASES for norm in (False, True)]
LIK_IDS = [f'{GG.case_tag(c, e)}-t{tau}' for c, e, tau in LIK_SETTINGS]
JSD_IDS = [f'{GG.case_tag(c, e)}-n{int(norm)}' for c, e, norm in JSD_SETTINGS]


@functools.lru_cache(maxsize=None)
def fixture(key):
    return load(GG.FILES[key])


def lik_matrix(z1, z2, conformer_major=False, product=False):
    """L[i, j] = mean over conformers c and features d of N(x_jcd; m_id, exp(s_id)); rows: the 2D view.  conformer_major: row r of z2 is
    molecule r % B, conformer r // B (the metrics); product: the joint density of the D features instead of their mean"""
    B, D = z1.shape[0], z2.shape[1]
    m, sigma = z1[:, :D], torch.exp(z1[:, D:] / 2)
    x = z2.reshape(-1, B, D).permute(1, 0, 2) if conformer_major else z2.reshape(B, -1, D)
    t = (x[None, :, :, :] - m[:, None, None, :]) / sigma[:, None, None, :]
    p = torch.exp(-0.5 * t * t) / (sigma[:, None, None, :] * math.sqrt(2 * math.pi))
    return p.prod(dim=3).mean(dim=2) if product else p.mean(dim=(2, 3))


def lik_loss(z1, z2, tau=0.5, swap_roles=False, product=False):
    """mean_i (log sum_{j != i} exp(L_ij / tau) - L_ii / tau): the negatives summed directly, the row maximum out of the exponent"""
    L = lik_matrix(z1, z2, product=product)
    if swap_roles:
        L = L.T
    E = L / tau
    neg = E.masked_fill(torch.eye(E.shape[0], dtype=torch.bool), float('-inf'))
    mx = neg.max(dim=1).values.detach()
    return (mx + torch.log(torch.exp(neg - mx[:, None]).sum(dim=1)) - torch.diagonal(E)).mean()


def jsd_loss(z1, z2, norm=True, swap_roles=False, unbiased=True, eps_on_each_variance=False, weight_eps=1e-5):
    """-mean_a log(S_aa / sum_{b != a} S_ab), S[a, b] = 0.5 (log(prod v2_a + 1e-5) - sum s_b - D + sum (exp(s_b) + (m2_a - m1_b)^2) / (v2_a +
    1e-5)); rows a: the 3D view"""
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.reshape(B, 2, D), z2.reshape(B, -1, D)
    if norm:
        a, b = torch.nn.functional.normalize(a, dim=2), torch.nn.functional.normalize(b, dim=2)
    m1, s = a[:, 0], a[:, 1]
    m2, v2 = b.mean(dim=1), b.var(dim=1, unbiased=unbiased)
    logdet = torch.log((v2 + 1e-5).prod(dim=1)) if eps_on_each_variance else torch.log(v2.prod(dim=1) + 1e-5)
    quad = ((torch.exp(s)[None, :, :] + (m2[:, None, :] - m1[None, :, :]) ** 2) / (v2[:, None, :] + weight_eps)).sum(dim=2)
    S = 0.5 * (logdet[:, None] - s.sum(dim=1)[None, :] - D + quad)
    if swap_roles:
        S = S.T
    off = ~torch.eye(B, dtype=torch.bool)
    return -torch.log(torch.diagonal(S) / (S * off).sum(dim=1)).mean()


def prob_metrics(z1, z2, conformer_major=True):
    """(mean_i L_ii, mean_i sum_{j != i} L_ij)"""
    L = lik_matrix(z1, z2, conformer_major=conformer_major)
    off = ~torch.eye(L.shape[0], dtype=torch.bool)
    return torch.diagonal(L).mean(), (L * off).sum(dim=1).mean()


def restated(fn, z1, z2, dtype=torch.float64, **kw):
    """-> (loss, dz1, dz2) of a restatement in `dtype`"""
    a = torch.as_tensor(z1).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(dtype).clone().requires_grad_(True)
    loss = fn(a, b, **kw)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def _matches(got, z, p, tol=1e-10):
    for name, g in zip(('loss', 'dz1', 'dz2'), got):
        ref = torch.as_tensor(z[p + name + ('64' if name == 'loss' else '_64')])
        assert ref.dtype == torch.float64 and ref.shape == g.shape
        err = (g - ref).abs().max().item()
        assert err <= tol * max(1.0, ref.abs().max().item()), (name, err)


def reference_cancellation(z1, z2, tau):
    """the relative error the reference's own fp64 denominator `row sum - positive` can carry: B roundings of a sum as large as the
    positive, relative to what is left of it"""
    E = torch.exp(lik_matrix(torch.as_tensor(z1).double(), torch.as_tensor(z2).double()) / tau)
    den = (E * ~torch.eye(E.shape[0], dtype=torch.bool)).sum(dim=1)
    return float((E.shape[0] * 2.0 ** -53 * torch.diagonal(E) / den).max())


@pytest.mark.parametrize('setting', LIK_SETTINGS, ids=LIK_IDS)
def test_likelihood_restatement_reproduces_the_reference(setting):
    """to 1e-10.  One case cannot be held to that by any restatement: on aligned4 at tau = 0.1 the positive is e^25 times the negatives,
    so the reference's own fp64 `row sum - positive` keeps 25 of its 53 bits and its stored result is only that exact.  There the bound
    is what that cancellation can carry, B 2^-53 E_ii / den_i = 3.1e-4 (the restatement, which sums the negatives directly, sits 7e-6
    from the stored loss and 3.2e-5 from the stored dz2); in every other case that figure is below 1e-12 and the bound is 1e-10."""
    shape, edge, tau = setting
    z = fixture('lik')
    tag = GG.case_tag(shape, edge)
    z1, z2 = z[f'in/{tag}/z1'], z[f'in/{tag}/z2']
    B, C, D = shape
    assert z1.shape == (B, 2 * D) and z2.shape == (B * C, D)
    cancel = reference_cancellation(z1, z2, tau)
    assert cancel < 1e-10 or (edge, tau) == ('aligned4', 0.1)
    _matches(restated(lik_loss, z1, z2, tau=tau), z, f'lik/{tag}/t{tau}/', max(1e-10, cancel))


@pytest.mark.parametrize('setting', JSD_SETTINGS, ids=JSD_IDS)
def test_jsd_restatement_reproduces_the_reference(setting):
    shape, edge, norm = setting
    z = fixture('jsd')
    tag = GG.case_tag(shape, edge)
    z1, z2 = z[f'in/{tag}/z1'], z[f'in/{tag}/z2']
    B, C, D = shape
    assert z1.shape == (B, 2 * D) and z2.shape == (B * C, D)
    _matches(restated(jsd_loss, z1, z2, norm=norm), z, f'jsd/{tag}/n{int(norm)}/')


@pytest.mark.parametrize('case', GG.LIK_CASES, ids=[GG.case_tag(*c) for c in GG.LIK_CASES])
def test_metric_restatement_reproduces_the_reference(case):
    z = fixture('lik')
    tag = GG.case_tag(*case)
    z1, z2 = torch.from_numpy(z[f'in/{tag}/z1']).double(), torch.from_numpy(z[f'in/{tag}/z2']).double()
    pos, neg = prob_metrics(z1, z2)
    for got, name in ((pos, 'positive_prob'), (neg, 'negative_prob')):
        ref = float(z[f'metrics/{tag}/{name}'])
        assert z[f'metrics/{tag}/{name}'].dtype == np.float64
        assert abs(got.item() - ref) <= 1e-10 * max(1.0, abs(ref)), name


def test_fixture_inputs_regenerate_and_the_edge_cases_are_what_they_say():
    lik, jsd = fixture('lik'), fixture('jsd')
    for z, cases in ((lik, GG.LIK_CASES), (jsd, GG.JSD_CASES)):
        for shape, edge in cases:
            tag = GG.case_tag(shape, edge)
            for name, t in zip(('z1', 'z2'), GG.case_inputs(shape, edge)):
                assert np.array_equal(z[f'in/{tag}/{name}'], t.numpy()), (tag, name)
    D = GG.EDGE_SHAPE[2]
    tag = GG.case_tag(GG.EDGE_SHAPE, 'aligned4')
    assert -4.5 < lik[f'in/{tag}/z1'][:, D:].mean() < -3.5
    assert np.isneginf(lik[f'lik/{tag}/t0.1/loss32']) and np.isfinite(lik[f'lik/{tag}/t0.1/loss64'])       # the reference's fp32 fails
    for key in lik.files:
        if key.endswith('loss64') or (key.endswith('loss32') and 'aligned4/t0.1' not in key):
            assert np.isfinite(lik[key]), key
    for key in jsd.files:
        if key.startswith('jsd/'):
            assert np.isfinite(jsd[key]).all(), key
    assert float(jsd['jsd/2x2x8/n0/loss64']) < 0          # S is not exponentiated: a ratio above one is possible


def test_roles_mean_variance_epsilon_and_layout_matter():
    """swapping rows and columns, a product of the D densities, the biased variance, the 1e-5 on every variance, and the molecule-major
    view in the metrics all give other numbers: the restatements above are not insensitive to them"""
    z = fixture('lik')
    tag = GG.case_tag((5, 3, 24))
    z1, z2 = torch.from_numpy(z[f'in/{tag}/z1']).double(), torch.from_numpy(z[f'in/{tag}/z2']).double()
    ref = float(z[f'lik/{tag}/t0.1/loss64'])
    assert abs(lik_loss(z1, z2, tau=0.1).item() - ref) < 1e-10 * abs(ref)
    assert abs(lik_loss(z1, z2, tau=0.1, swap_roles=True).item() - ref) > 1e-3 * abs(ref)
    assert abs(lik_loss(z1, z2, tau=0.1, product=True).item() - ref) > 1e-3 * abs(ref)
    for k, name in enumerate(('positive_prob', 'negative_prob')):
        ref = float(z[f'metrics/{tag}/{name}'])
        assert abs(prob_metrics(z1, z2)[k].item() - ref) < 1e-10 * abs(ref)
        assert abs(prob_metrics(z1, z2, conformer_major=False)[k].item() - ref) > 1e-3 * abs(ref)
    neg = float(z[f'metrics/{tag}/negative_prob'])
    L = lik_matrix(z1, z2, conformer_major=True)
    assert abs((L.sum() - torch.diagonal(L).sum()).item() / 5 / 4 - neg) > 0.5 * neg          # a sum over the negatives, not their mean

    z = fixture('jsd')
    z1, z2 = torch.from_numpy(z[f'in/{tag}/z1']).double(), torch.from_numpy(z[f'in/{tag}/z2']).double()
    ref = float(z[f'jsd/{tag}/n0/loss64'])
    assert abs(jsd_loss(z1, z2, norm=False).item() - ref) < 1e-10 * abs(ref)
    assert abs(jsd_loss(z1, z2, norm=False, swap_roles=True).item() - ref) > 1e-3 * abs(ref)
    assert abs(jsd_loss(z1, z2, norm=False, unbiased=False).item() - ref) > 1e-3 * abs(ref)
    assert abs(jsd_loss(z1, z2, norm=True).item() - ref) > 1e-3 * abs(ref)
    assert abs(jsd_loss(z1, z2, norm=False, eps_on_each_variance=True).item() - ref) > 1e-4 * abs(ref)     # log(prod v2 + 1e-5)
    tag = GG.case_tag(GG.EDGE_SHAPE, 'jitter2')            # v2 ~ 1e-4: the 1e-5 beside it in the weights is a tenth of it
    z1, z2 = torch.from_numpy(z[f'in/{tag}/z1']).double(), torch.from_numpy(z[f'in/{tag}/z2']).double()
    ref = float(z[f'jsd/{tag}/n0/loss64'])
    assert abs(jsd_loss(z1, z2, norm=False).item() - ref) < 1e-10 * abs(ref)
    assert abs(jsd_loss(z1, z2, norm=False, weight_eps=0.0).item() - ref) > 1e-3 * abs(ref)


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    metrics = importlib.import_module('3dinfomax_amd.metrics')
    names = launcher.plugin_names()
    for module, group in ((losses, LOSSES), (metrics, METRICS)):
        for name in group:
            assert name in amd.__all__ and name in alias.__all__
            assert getattr(amd, name) is getattr(alias, name) is getattr(module, name) is names[name]
    for name in LOSSES:
        assert issubclass(getattr(amd, name), losses._Separate2DBase) and getattr(amd, name)._data_parallel is False


REFERENCE_SIGNATURES = {
    'NTXentLikelihoodLoss': dict(norm=True, tau=0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0, conformer_variance_reg=0),
    'JSDMultiplePositivesLoss': dict(norm=True, tau=0.5, uniformity_reg=0, variance_reg=0, covariance_reg=0),
    'PositiveProb': dict(),
    'NegativeProb': dict(),
}


@pytest.mark.parametrize('name', sorted(REFERENCE_SIGNATURES))
def test_constructor_signatures_and_defaults_are_the_reference_s(name):
    """names, order and defaults of reference commons/losses.py:546, :326 and trainer/metrics.py:337, :368"""
    cls = getattr(amd, name)
    params = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name not in ('self', 'args', 'kwargs')]
    assert [(q.name, q.default) for q in params] == list(REFERENCE_SIGNATURES[name].items())
    d = cls()
    for k, v in REFERENCE_SIGNATURES[name].items():
        assert getattr(d, k) == v
    if params:
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


@pytest.mark.parametrize('name', LOSSES)
def test_refusals_fire_on_cpu_tensors_before_any_library_call(name, monkeypatch):
    _no_library(monkeypatch)
    cls = getattr(amd, name)
    loss = cls(tau=0.1)
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 2 * 8 + 1), torch.zeros(12, 8))         # z1 is not 2 D wide
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 3 * 8), torch.zeros(12, 8))             # the layout of the Separate2D losses
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 16), torch.zeros(13, 8))                # z2 rows not divisible by the batch
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 16), torch.zeros(2, 8))                 # fewer rows than molecules
    with pytest.raises(ValueError, match='no negatives'):
        loss(torch.zeros(1, 16), torch.zeros(3, 8))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(4, 4, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match=f'{name}: covariance_reg'):
        cls(covariance_reg=0.1)(torch.zeros(4, 16), torch.zeros(12, 8))
    with pytest.raises(NotImplementedError, match=f'{name}: uniformity_reg'):
        cls(uniformity_reg=0.1)(torch.zeros(4, 16), torch.zeros(12, 8))


def test_one_conformer_is_refused_where_a_variance_is_needed(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match='at least two'):
        amd.JSDMultiplePositivesLoss()(torch.zeros(4, 16), torch.zeros(4, 8))
    with pytest.raises(ValueError, match='conformer_variance_reg.*at least two'):
        amd.NTXentLikelihoodLoss(conformer_variance_reg=0.05)(torch.zeros(4, 16), torch.zeros(4, 8))
    with pytest.raises(AssertionError, match='no CPU fallback'):
        amd.NTXentLikelihoodLoss()(torch.zeros(4, 16), torch.zeros(4, 8))          # C = 1 is valid there; CPU tensors are not


@pytest.mark.parametrize('name', LOSSES)
def test_a_group_of_more_than_one_rank_is_refused(name, monkeypatch):
    _no_library(monkeypatch)
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss = getattr(amd, name)().attach_group(group)
    with pytest.raises(NotImplementedError, match=f'{name} on a process group'):
        loss(torch.zeros(4, 16), torch.zeros(12, 8))


def test_regularisers_on_the_views():
    """the reference hands std_loss the [B, 2, D] and [B, C, D] views; the conformer hinge is the one of NTXentMultiplePositives"""
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(4, 2, 8, generator=g), torch.randn(4, 3, 8, generator=g)
    std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()
    for name in LOSSES:
        got = getattr(amd, name)(variance_reg=0.5)._regularisers(torch.zeros(()), a, b)
        assert abs(got.item() - 0.5 * (std(a) + std(b)).item()) < 1e-6
        with pytest.raises(NotImplementedError, match='covariance_reg'):
            getattr(amd, name)(covariance_reg=0.1)._regularisers(torch.zeros(()), a, b)
        with pytest.raises(NotImplementedError, match='uniformity_reg'):
            getattr(amd, name)(uniformity_reg=0.1)._regularisers(torch.zeros(()), a, b)


def test_metrics_answer_the_trainer_s_init_call_with_nan(monkeypatch):
    """trainer/metrics.py:344: batch == dim == 2 is the call that fills the trainer's dictionary - NaN, no device work"""
    _no_library(monkeypatch)
    for name in METRICS:
        v = getattr(amd, name)()(torch.zeros(2, 2), torch.zeros(2, 2))
        assert v.dim() == 0 and torch.isnan(v)
        with pytest.raises(ValueError, match='incompatible embedding shapes'):
            getattr(amd, name)()(torch.zeros(4, 16), torch.zeros(13, 8))
        with pytest.raises(ValueError, match='incompatible embedding shapes'):
            getattr(amd, name)()(torch.zeros(4, 8), torch.zeros(12, 8))


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    ops = importlib.import_module('3dinfomax_amd.ops')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_gauss_lik_fwd', 'i3d_gauss_lik_loss', 'i3d_gauss_lik_probs', 'i3d_gauss_lik_bwd', 'i3d_gauss_jsd_fwd',
                 'i3d_gauss_jsd_bwd'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert ops.gauss_z2_strides(4, 3, 8) == (24, 8) and ops.gauss_z2_strides(4, 3, 8, conformer_major=True) == (8, 32)
    # argument validation happens on the host before any launch: no GPU needed
    lik = lambda b, c, d, ms, cs: lib.i3d_gauss_lik_fwd(None, None, b, c, d, ms, cs, None, None)
    assert lik(1, 3, 8, 24, 8) == -1 and b'no negatives' in lib.i3d_last_error()
    assert lik(4, 0, 8, 0, 8) == -1 and b'conformer' in lib.i3d_last_error()
    assert lik(4, 3, 0, 0, 0) == -1 and b'feature' in lib.i3d_last_error()
    assert lik(4, 3, 8, 24, 9) == -1 and b'strides' in lib.i3d_last_error()
    assert lik(4, 3, 8, 8, 24) == -1 and b'strides' in lib.i3d_last_error()
    assert lik(4, 3, 8, 24, 8) == -1 and b'null' in lib.i3d_last_error()                 # molecule major passes the checks
    assert lik(4, 3, 8, 8, 32) == -1 and b'null' in lib.i3d_last_error()                 # conformer major too
    assert lik(4, 1, 300, 300, 300) == -1 and b'null' in lib.i3d_last_error()            # C = 1, D above the workgroup size
    assert lib.i3d_gauss_lik_loss(None, 4, 0.0, None, None, None) == -1 and b'tau' in lib.i3d_last_error()
    assert lib.i3d_gauss_lik_loss(None, 4, 0.1, None, None, None) == -1 and b'null' in lib.i3d_last_error()
    assert lib.i3d_gauss_lik_probs(None, 4, None, None) == -1 and b'null' in lib.i3d_last_error()
    assert lib.i3d_gauss_lik_bwd(None, None, 4, 3, 8, 24, 8, None, None, 0.1, None, None, None, None, None) == -1 \
        and b'null' in lib.i3d_last_error()
    assert lib.i3d_gauss_jsd_fwd(None, None, 4, 1, 8, None, None, None, None, None) == -1 and b'two conformers' in lib.i3d_last_error()
    assert lib.i3d_gauss_jsd_bwd(None, None, 4, 1, 8, None, None, None, None, None, None) == -1 and b'two conformers' in lib.i3d_last_error()
    assert lib.i3d_gauss_jsd_fwd(None, None, 1, 2, 8, None, None, None, None, None) == -1 and b'no negatives' in lib.i3d_last_error()
    assert lib.i3d_gauss_jsd_fwd(None, None, 4, 9, 300, None, None, None, None, None) == -1 and b'null' in lib.i3d_last_error()
