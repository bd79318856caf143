"""KLDivergenceMultiplePositives on the host: an fp64 restatement of the closed form against the reference's own fp64 results (fixture:
tests/golden/gen_golden_kl.py) - which pins the direction KL(N2 || N1), the unbiased variance and its 1e-6 -, the plugin surface, the
refusals that fire before any library call, and the C ABI's argument checks."""
import importlib

import pytest
import torch

from helpers import amd, load

import gen_golden_kl as GK

launcher = importlib.import_module('launch_reference')
NAME = 'KLDivergenceMultiplePositives'
METRICS = ('Conformer3DVariance', 'Conformer2DVariance')
CASES = GK.ALL_CASES
CASE_IDS = [GK.case_tag(*c, j) for c, j in CASES]


def kl_restated(z1, z2, norm=False, reverse=False, var_eps=1e-6, unbiased=True):
    """mean_b 0.5 sum_d (s1 - log v2 + (v2 + (m2 - m1)^2) exp(-s1) - 1): KL(N(m2, v2) || N(m1, exp(s1))) of diagonal Gaussians;
    reverse: KL(N1 || N2)"""
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.reshape(B, 2, D), z2.reshape(B, -1, D)
    if norm:
        a, b = torch.nn.functional.normalize(a, dim=2), torch.nn.functional.normalize(b, dim=2)
    m1, s1 = a[:, 0], a[:, 1]
    m2, v2 = b.mean(dim=1), b.var(dim=1, unbiased=unbiased) + var_eps
    d2 = (m2 - m1) ** 2
    if reverse:
        kl = 0.5 * (torch.log(v2) - s1 + (torch.exp(s1) + d2) / v2 - 1.0).sum(dim=1)
    else:
        kl = 0.5 * (s1 - torch.log(v2) + (v2 + d2) * torch.exp(-s1) - 1.0).sum(dim=1)
    return kl.mean()


def restated(z1, z2, dtype=torch.float64, **kw):
    """-> (loss, dz1, dz2) of the restatement in `dtype`"""
    a = torch.as_tensor(z1).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(dtype).clone().requires_grad_(True)
    loss = kl_restated(a, b, **kw)
    loss.backward()
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize('norm', [False, True], ids=['raw', 'norm'])
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_fp64_restatement_reproduces_the_reference(case, norm):
    (B, C, D), jitter = case
    z = load('kl_multiple_positives.npz')
    tag = GK.case_tag(B, C, D, jitter)
    z1, z2 = z[f'loss/{tag}/z1'], z[f'loss/{tag}/z2']
    assert z1.shape == (B, 2 * D) and z2.shape == (B * C, D)
    p = f'loss/{tag}/n{int(norm)}/'
    loss, g1, g2 = restated(z1, z2, norm=norm)
    for name, got, ref in (('loss', loss, z[p + 'loss64']), ('dz1', g1, z[p + 'dz1_64']), ('dz2', g2, z[p + 'dz2_64'])):
        ref = torch.as_tensor(ref)
        assert ref.dtype == torch.float64
        err = (got - ref).abs().max().item()
        assert err <= 1e-10 * max(1.0, ref.abs().max().item()), (name, err)


def test_direction_variance_and_epsilon_matter():
    """the opposite direction KL(N1 || N2), the biased variance and a missing 1e-6 all give other numbers: the restatement above is not
    insensitive to them"""
    z = load('kl_multiple_positives.npz')
    tag = GK.case_tag(5, 3, 24)
    z1, z2 = torch.from_numpy(z[f'loss/{tag}/z1']).double(), torch.from_numpy(z[f'loss/{tag}/z2']).double()
    ref = float(z[f'loss/{tag}/n0/loss64'])
    assert abs(kl_restated(z1, z2).item() - ref) < 1e-10 * abs(ref)
    assert abs(kl_restated(z1, z2, reverse=True).item() - ref) > 1e-3 * abs(ref)
    assert abs(kl_restated(z1, z2, unbiased=False).item() - ref) > 1e-3 * abs(ref)
    tag = GK.case_tag(5, 3, 24, True)          # near-coincident conformers: v2 ~ 1e-4, the 1e-6 is 1 % of it
    z1, z2 = torch.from_numpy(z[f'loss/{tag}/z1']).double(), torch.from_numpy(z[f'loss/{tag}/z2']).double()
    ref = float(z[f'loss/{tag}/n0/loss64'])
    assert abs(kl_restated(z1, z2).item() - ref) < 1e-10 * abs(ref)
    assert abs(kl_restated(z1, z2, var_eps=0.0).item() - ref) > 1e-4 * abs(ref)


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    metrics = importlib.import_module('3dinfomax_amd.metrics')
    names = launcher.plugin_names()
    assert NAME in amd.__all__ and NAME in alias.__all__
    assert getattr(amd, NAME) is getattr(alias, NAME) is getattr(losses, NAME) is names[NAME]
    for name in METRICS:
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(amd, name) is getattr(alias, name) is getattr(metrics, name) is names[name]
        assert getattr(amd, name)().norm is False and getattr(amd, name)(normalize=True).norm is True
    loss = amd.KLDivergenceMultiplePositives()
    assert loss.norm is False and loss.tau == 0.5
    assert (loss.uniformity_reg, loss.variance_reg, loss.covariance_reg) == (0, 0, 0)
    loss = amd.KLDivergenceMultiplePositives(norm=True, tau=0.1, uniformity_reg=0, variance_reg=0.5, covariance_reg=0)
    assert loss.norm is True and loss.tau == 0.1 and loss.variance_reg == 0.5          # tau: accepted (the config passes it), unused


def _no_library(monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)


def test_refusals_fire_on_cpu_tensors_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    loss = amd.KLDivergenceMultiplePositives(tau=0.1)
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 2 * 8 + 1), torch.zeros(12, 8))         # z1 is not 2 D wide
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 3 * 8), torch.zeros(12, 8))             # the layout of the Separate2D losses
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 16), torch.zeros(13, 8))                # z2 rows not divisible by the batch
    with pytest.raises(ValueError, match='at least two'):
        loss(torch.zeros(4, 16), torch.zeros(4, 8))                 # one conformer: its variance is undefined
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(4, 4, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match='covariance_reg'):
        amd.KLDivergenceMultiplePositives(covariance_reg=0.1)(torch.zeros(4, 16), torch.zeros(12, 8))
    with pytest.raises(NotImplementedError, match='uniformity_reg'):
        amd.KLDivergenceMultiplePositives(uniformity_reg=0.1)(torch.zeros(4, 16), torch.zeros(12, 8))


def test_shard_counts_that_do_not_describe_the_batch_are_refused_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2)
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda g=None: 0)
    loss = amd.KLDivergenceMultiplePositives().attach_group(group)
    for counts in ([3, 3], [4, 3, 1], [3, 4]):
        loss.set_shard_counts(counts)
        with pytest.raises(ValueError, match='shard counts'):
            loss(torch.zeros(4, 16), torch.zeros(12, 8))


def test_variance_regulariser_works_on_the_views_and_the_other_two_are_refused():
    """the reference hands its regularisers the [B, 2, D] and [B, C, D] views: std_loss works on them, cov_loss and uniformity_loss raise"""
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(4, 2, 8, generator=g), torch.randn(4, 3, 8, generator=g)
    std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()
    got = amd.KLDivergenceMultiplePositives(variance_reg=0.5)._regularisers(torch.zeros(()), a, b)
    assert abs(got.item() - 0.5 * (std(a) + std(b)).item()) < 1e-6
    with pytest.raises(NotImplementedError, match='covariance_reg'):
        amd.KLDivergenceMultiplePositives(covariance_reg=0.1)._regularisers(torch.zeros(()), a, b)
    with pytest.raises(NotImplementedError, match='uniformity_reg'):
        amd.KLDivergenceMultiplePositives(uniformity_reg=0.1)._regularisers(torch.zeros(()), a, b)


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_kl_mp_fwd', 'i3d_kl_mp_bwd'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    # argument validation happens on the host before any launch: no GPU needed
    assert lib.i3d_kl_mp_fwd(None, None, 4, 1, 8, 0.25, None, None, None) == -1 and b'two conformers' in lib.i3d_last_error()
    assert lib.i3d_kl_mp_bwd(None, None, 4, 1, 8, 0.25, None, None, None, None) == -1 and b'two conformers' in lib.i3d_last_error()
    assert lib.i3d_kl_mp_fwd(None, None, 0, 2, 8, 1.0, None, None, None) == -1 and b'batch' in lib.i3d_last_error()
    assert lib.i3d_kl_mp_fwd(None, None, 4, 2, 0, 0.25, None, None, None) == -1 and b'feature' in lib.i3d_last_error()
    assert lib.i3d_kl_mp_fwd(None, None, 4, 9, 8, 0.25, None, None, None) == -1 and b'null' in lib.i3d_last_error()   # C = 9 passes the shape check
