"""BarlowTwinsLoss / CosineSimilarityLoss / RegularizationLoss / CriticLoss on the host: fp64 restatements of the four formulas against
the reference's own fp64 results (fixture: tests/golden/gen_golden_batchstat.py), the backward formulas of csrc/batchstat.hip restated in
fp64 against autograd, the hinge conditions of the fixture, the plugin surface, D = 1, and the refusals that fire before any library call."""
import importlib
import inspect

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_batchstat as GB
import gen_golden_hardneg as GH

launcher = importlib.import_module('launch_reference')
NAMES = dict(GB.LOSSES)
CASES = GB.all_cases()
CASE_IDS = [GB.case_prefix(*c).strip('/').replace('/', '-') for c in CASES]
DEFAULTS = {'barlow': dict(scale_loss=1 / 32, lambd=3.9e-3, uniformity_reg=0, variance_reg=0, covariance_reg=0),
            'cosine': dict(uniformity_reg=0, variance_reg=0, covariance_reg=0),
            'regularization': dict(uniformity_reg=0, variance_reg=1, covariance_reg=0.04), 'critic': {}}


def case_setup(z, key, shape, tag):
    """(the two arguments the loss is called with, constructor kwargs, R) of a fixture case"""
    kw, R = next((k, r) for t, k, r in GB.parameter_sets(key) if t == tag)
    B, D = shape
    x, y = GB.case_inputs(z[f'in/{B}x{D}/z1'], z[f'in/{B}x{D}/z2'], kw, R)
    return x, y, kw, R


def std_term(x):
    return torch.relu(1.0 - torch.sqrt(x.var(dim=0) + 1e-4)).mean()


def cov_term(x):
    n, dim = x.shape
    c = x - x.mean(dim=0)
    cov = c.T @ c / (n - 1)
    off = ~torch.eye(dim, dtype=torch.bool)
    return (cov[off] ** 2).sum() / dim


def uniformity_term(x1, x2, t=2):
    return 0.5 * sum(torch.pdist(x, p=2).pow(2).mul(-t).exp().mean().log() for x in (x1, x2))


def normalised(x, dim):
    return x / x.norm(dim=dim, keepdim=True).clamp_min(1e-12)


def restated_loss(key, x, y, scale_loss=1 / 32, lambd=3.9e-3, uniformity_reg=0, variance_reg=0, covariance_reg=0):
    """the formulas of csrc/batchstat.hip as a torch expression in the dtype of x; the off-diagonal sums run over the off-diagonal
    entries, never `whole sum - diagonal`"""
    if key == 'critic':
        return ((normalised(x, 1)[:, :, None] - normalised(y, 1)) ** 2).sum(dim=1).mean()
    B, D = x.shape
    if key == 'barlow':
        a = (x - x.mean(dim=0)) / x.std(dim=0)
        b = (y - y.mean(dim=0)) / y.std(dim=0)
        C = a.T @ b / B
        off = ~torch.eye(D, dtype=torch.bool)
        loss = scale_loss * (((torch.diagonal(C) - 1) ** 2).sum() + lambd * (C[off] ** 2).sum())
    elif key == 'cosine':
        loss = ((normalised(x, 1) - normalised(y, 1)) ** 2).sum(dim=1).mean()
    else:
        loss = ((x - y) ** 2).mean()
    if variance_reg > 0:
        loss = loss + variance_reg * (std_term(x) + std_term(y))
    if covariance_reg > 0:
        loss = loss + covariance_reg * (cov_term(x) + cov_term(y))
    if uniformity_reg > 0:
        loss = loss + uniformity_reg * uniformity_term(x, y)
    return loss


def restated(key, x, y, dtype=torch.float64, **kw):
    """-> (loss, gradient of the first argument, of the second) of the restatement in `dtype`"""
    a = torch.as_tensor(x).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(y).to(dtype).clone().requires_grad_(True)
    loss = restated_loss(key, a, b, **kw)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def restated_kwargs(key, kw):
    """constructor kwargs of a case -> kwargs of `restated`, the class's defaults filled in (`norm` has no effect)"""
    out = dict(DEFAULTS[key])
    out.update({k: v for k, v in kw.items() if k != 'norm'})
    return out


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_fp64_restatement_reproduces_the_reference(case):
    """loss at 1e-10; gradients at 1e-9 of their largest entry (the fixture stores them in steps of 4.7e-10 of it) plus 1e-14: the
    BarlowTwins gradient at B = 2 is analytically zero - both standardised views are +-2^-1/2 whatever the input - and is rounding noise
    of 1e-17 in the reference as in the restatement"""
    key, shape, tag = case
    z = load('batchstat.npz')
    p = GB.case_prefix(key, shape, tag)
    x, y, kw, R = case_setup(z, key, shape, tag)
    assert y.shape == ((shape[0], shape[1], R) if R else shape)
    loss, g1, g2 = restated(key, x, y, **restated_kwargs(key, kw))
    assert z[p + 'loss64'].dtype == np.float64
    assert abs(loss.item() - float(z[p + 'loss64'])) <= 1e-10 * max(1.0, abs(float(z[p + 'loss64'])))
    for name, got in (('g1', g1), ('g2', g2)):
        ref = torch.from_numpy(GH.decode(z, p, name))
        assert ref.shape == got.shape
        assert (got - ref).abs().max().item() <= 1e-9 * float(z[p + name + '_scale']) + 1e-14, name
    assert z[p + 'err32'].shape == (3,) and (z[p + 'err32'] >= 0).all() and np.isfinite(z[p + 'err32']).all()
    if not (key == 'barlow' and shape[0] == 2):
        assert (z[p + 'err32'] < 1e-4).all()


@pytest.mark.parametrize('shape', GB.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_fixture_inputs_regenerate_and_meet_the_hinge_conditions(shape):
    """every column further than 1e-3 from the kink of the hinge, 20 % .. 80 % of the columns of the pair active from B = 5 on"""
    B, D = shape
    z = load('batchstat.npz')
    z1, z2 = GB.pair(B, D, int(z[f'in/{B}x{D}/seed']))
    assert np.array_equal(z[f'in/{B}x{D}/z1'], z1.numpy()) and np.array_equal(z[f'in/{B}x{D}/z2'], z2.numpy())
    ok, share, margin = GB.hinge_ok(z1, z2)
    assert ok and margin > GB.MARGIN
    if B >= 5:
        assert 0.2 <= share <= 0.8
    rec = GB.reconstruction(z1, z2, 10)
    assert rec.shape == (B, D, 10) and rec.is_contiguous()
    assert torch.equal(GB.reconstruction(z1, z2, 3), rec[:, :, :3])


def kernel_column_backward(z1, z2, barlow=None, var_w=0.0, cov_w=0.0):
    """the launch structure of csrc/batchstat.hip in fp64 torch: moments, the D x D pass that leaves G = dL/dC in place, two products
    da = b G^T and db = a G (covariance: one, dc = c G), and per column
        dz = sa (da - mean(da) - a sum(da a) / (n - 1)) / std + sc (dc - mean(dc)) + hc_j (z - mean_j)
    -> (loss, dz1, dz2)"""
    n, dim = z1.shape
    views = (z1, z2)
    mean = [v.mean(dim=0) for v in views]
    var = [((v - m) ** 2).sum(dim=0) / (n - 1) for v, m in zip(views, mean)]
    diag = torch.eye(dim, dtype=torch.bool)
    loss = torch.zeros((), dtype=z1.dtype)
    dz = [torch.zeros_like(v) for v in views]
    if barlow is not None:
        scale_loss, lambd = barlow
        a = [(v - m) / s.sqrt() for v, m, s in zip(views, mean, var)]
        C = a[0].T @ a[1] / n
        loss = loss + scale_loss * (((C[diag] - 1) ** 2).sum() + lambd * (C[~diag] ** 2).sum())
        G = torch.where(diag, 2 * scale_loss * (C - 1), 2 * scale_loss * lambd * C)
        for k, da in enumerate((a[1] @ G.T, a[0] @ G)):
            dz[k] += (1.0 / n) * (da - da.mean(dim=0) - a[k] * (da * a[k]).sum(dim=0) / (n - 1)) / var[k].sqrt()
    for k, v in enumerate(views):
        if cov_w:
            c = v - mean[k]
            cov = c.T @ c / (n - 1)
            loss = loss + cov_w / dim * (cov[~diag] ** 2).sum()
            dc = c @ torch.where(diag, torch.zeros_like(cov), 2 * cov_w / dim * cov)
            dz[k] += 2.0 / (n - 1) * (dc - dc.mean(dim=0))
        if var_w:
            sv = (var[k] + 1e-4).sqrt()
            loss = loss + var_w * torch.relu(1 - sv).mean()
            hc = torch.where(1 - sv > 0, -var_w / (dim * (n - 1) * sv), torch.zeros_like(sv))
            dz[k] += hc * (v - mean[k])
    return loss, dz[0], dz[1]


@pytest.mark.parametrize('shape', [(5, 13), (67, 13), (64, 64)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('terms', [dict(barlow=(1 / 32, 3.9e-3)), dict(barlow=(1.0, 1.0), var_w=1.0, cov_w=0.04), dict(var_w=1.0, cov_w=0.04),
                                   dict(cov_w=0.5), dict(var_w=0.5)], ids=['barlow', 'barlow+regs', 'regs', 'cov', 'var'])
def test_restated_backward_of_the_column_kernels_is_autograd_s(shape, terms):
    """the backward of the standardisation, of the centring under a symmetric G and of the variance hinge, as the kernels compute them,
    against autograd of the plain formulas in fp64: 1e-12 of the largest gradient entry"""
    z = load('batchstat.npz')
    z1 = torch.from_numpy(z[f'in/{shape[0]}x{shape[1]}/z1']).double()
    z2 = torch.from_numpy(z[f'in/{shape[0]}x{shape[1]}/z2']).double()
    loss, dz1, dz2 = kernel_column_backward(z1, z2, **terms)
    barlow = terms.get('barlow')
    kw = dict(variance_reg=terms.get('var_w', 0), covariance_reg=terms.get('cov_w', 0))
    if barlow is not None:
        want = restated('barlow', z1, z2, scale_loss=barlow[0], lambd=barlow[1], **kw)
    else:
        want = restated('regularization', z1, z2, **kw)
        mse = restated('regularization', z1, z2, variance_reg=0, covariance_reg=0)
        want = tuple(w - m for w, m in zip(want, mse))
    assert abs(loss.item() - want[0].item()) <= 1e-12 * max(1.0, abs(want[0].item()))
    for got, ref in ((dz1, want[1]), (dz2, want[2])):
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def kernel_row_backward(x, y, eps=1e-12):
    """csrc/batchstat.hip's row backward in fp64 torch for x [B, D], y [B, D, R]: gx = k (R x_hat - sum_r y_hat_r), dx = (gx - x_hat
    <x_hat, gx>) / nx' (a norm below the clamp: dx = gx / nx'), the same per repeat for y with gy_r = -k (x_hat - y_hat_r)"""
    B, D, R = y.shape
    k = 2.0 / (B * R)
    nx, ny = x.norm(dim=1, keepdim=True), y.norm(dim=1, keepdim=True)
    inx, iny = 1 / nx.clamp_min(eps), 1 / ny.clamp_min(eps)
    xh, yh = x * inx, y * iny
    loss = ((xh[:, :, None] - yh) ** 2).sum(dim=1).mean()
    gx = k * (R * xh - yh.sum(dim=2))
    dx = (gx - xh * torch.where(nx >= eps, (xh * gx).sum(dim=1, keepdim=True), torch.zeros_like(nx))) * inx
    gy = -k * (xh[:, :, None] - yh)
    dy = (gy - yh * torch.where(ny >= eps, (yh * gy).sum(dim=1, keepdim=True), torch.zeros_like(ny))) * iny
    return loss, dx, dy


@pytest.mark.parametrize('R', GB.REPEATS)
def test_restated_backward_of_the_row_kernels_is_autograd_s(R):
    """with one all-zero row in each argument: F.normalize's constant denominator 1e-12 in the backward too"""
    z = load('batchstat.npz')
    z1, z2 = torch.from_numpy(z['in/67x13/z1']).double(), torch.from_numpy(z['in/67x13/z2']).double()
    x, y = z2.clone(), GB.reconstruction(z1, z2, R).double()
    x[3] = 0
    y[5, :, R - 1] = 0
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    want = ((torch.nn.functional.normalize(a, dim=1, p=2)[..., None].repeat(1, 1, R) - torch.nn.functional.normalize(b, dim=1, p=2)) ** 2
            ).sum(dim=1).mean()
    want.backward()
    loss, dx, dy = kernel_row_backward(x, y)
    assert abs(loss.item() - want.item()) <= 1e-12
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all()
    zero_x, zero_y = torch.zeros(67, 1, dtype=torch.bool), torch.zeros(67, 1, R, dtype=torch.bool)
    zero_x[3], zero_y[5, :, R - 1] = True, True
    for got, ref, zero in ((dx, a.grad, zero_x), (dy, b.grad, zero_y)):
        for part in (zero, ~zero):                           # the zero vectors' gradients are g / 1e-12: judged apart from the rest
            g, r = got * part, ref * part
            assert (g - r).abs().max().item() <= 1e-12 * r.abs().max().item()
    assert a.grad[3].abs().max() > 1e6 and b.grad[5, :, R - 1].abs().max() > 1e6


def test_one_column_has_no_off_diagonal_terms():
    """D = 1 is legal: BarlowTwins is scale_loss (C_00 - 1)^2 and the covariance term is 0"""
    g = torch.Generator().manual_seed(1)
    z1 = torch.randn(33, 1, generator=g, dtype=torch.float64)
    z2 = 0.5 * z1 + torch.randn(33, 1, generator=g, dtype=torch.float64)
    a, b = (z1 - z1.mean()) / z1.std(), (z2 - z2.mean()) / z2.std()
    c00 = (a * b).sum() / 33
    loss, dz1, dz2 = kernel_column_backward(z1, z2, barlow=(1 / 32, 3.9e-3), cov_w=0.04)
    assert abs(loss.item() - ((c00 - 1) ** 2 / 32).item()) <= 1e-15
    assert cov_term(z1).item() == 0.0
    want = restated('barlow', z1, z2, covariance_reg=0.04)
    assert abs(want[0].item() - loss.item()) <= 1e-15 and (dz1 - want[1]).abs().max() <= 1e-13 and (dz2 - want[2]).abs().max() <= 1e-13


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    names = launcher.plugin_names()
    for name in NAMES.values():
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(amd, name) is getattr(alias, name) is getattr(losses, name) is names[name]
        assert not hasattr(getattr(amd, name), 'attach_group')          # no data-parallel form


def test_the_launcher_binds_the_four_names_and_builds_them_from_the_configs():
    """configs/byol.yml (loss_func: CosineSimilarityLoss) and configs/old_configs/philosophy.yml (loss_func: RegularizationLoss,
    critic_loss: CriticLoss) give no loss_params: train.py constructs the classes with **{}"""
    namespace = {name: object() for name in NAMES.values()}
    replaced = launcher.rebind(namespace, launcher.plugin_names())
    for name in NAMES.values():
        assert name in replaced and namespace[name] is getattr(amd, name)
        assert isinstance(namespace[name](**{}), torch.nn.Module)
    assert isinstance(namespace['RegularizationLoss'](norm=False, variance_reg=0.5, covariance_reg=0.1), torch.nn.Module)
    assert isinstance(namespace['BarlowTwinsLoss'](scale_loss=1 / 16, lambd=5e-3), torch.nn.Module)


REFERENCE_SIGNATURES = {
    'BarlowTwinsLoss': dict(scale_loss=1 / 32, lambd=3.9e-3, uniformity_reg=0, variance_reg=0, covariance_reg=0),
    'CosineSimilarityLoss': dict(uniformity_reg=0, variance_reg=0, covariance_reg=0),
    'RegularizationLoss': dict(norm=True, uniformity_reg=0, variance_reg=1, covariance_reg=0.04),
    'CriticLoss': dict(),
}


@pytest.mark.parametrize('name', sorted(REFERENCE_SIGNATURES))
def test_constructor_signatures_and_defaults_are_the_reference_s(name):
    """names, order and defaults of reference commons/losses.py:34, :46, :77, :107; forward(z1, z2, **kwargs), CriticLoss
    forward(z2, reconstruction, **kwargs)"""
    cls = getattr(amd, name)
    params = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != 'self']
    assert [(q.name, q.default) for q in params] == list(REFERENCE_SIGNATURES[name].items())
    d = cls()
    for k, v in REFERENCE_SIGNATURES[name].items():
        assert getattr(d, k) == v
    values = [0.25 + i for i in range(len(params))]
    c = cls(*values)
    assert [getattr(c, q.name) for q in params] == values
    fwd = list(inspect.signature(cls.forward).parameters.values())
    assert [q.name for q in fwd] == (['self', 'z2', 'reconstruction', 'kwargs'] if name == 'CriticLoss' else ['self', 'z1', 'z2', 'kwargs'])
    assert fwd[-1].kind is inspect.Parameter.VAR_KEYWORD


def _no_library(monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)


@pytest.mark.parametrize('name', ['BarlowTwinsLoss', 'CosineSimilarityLoss', 'RegularizationLoss'])
def test_two_view_losses_refuse_before_any_library_call(name, monkeypatch):
    _no_library(monkeypatch)
    loss = getattr(amd, name)()
    for a, b in ((torch.zeros(4, 8), torch.zeros(4, 7)), (torch.zeros(4, 8), torch.zeros(5, 8)), (torch.zeros(4, 8), torch.zeros(4, 8, 1)),
                 (torch.zeros(32), torch.zeros(32)), (torch.zeros(0, 8), torch.zeros(0, 8))):
        with pytest.raises(ValueError, match=name):
            loss(a, b)
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        loss(torch.zeros(4, 8), torch.zeros(4, 8))                  # fp32, but not on the device
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.float16))


def test_a_batch_of_one_is_refused_where_the_formula_divides_by_batch_minus_one(monkeypatch):
    """always for BarlowTwinsLoss; for the others only with a variance or covariance weight above 0 - then a batch of one passes the shape
    checks and reaches the device check"""
    _no_library(monkeypatch)
    one = torch.zeros(1, 8)
    for loss in (amd.BarlowTwinsLoss(), amd.BarlowTwinsLoss(variance_reg=1), amd.CosineSimilarityLoss(variance_reg=1),
                 amd.CosineSimilarityLoss(covariance_reg=0.04), amd.RegularizationLoss(), amd.RegularizationLoss(variance_reg=0)):
        with pytest.raises(ValueError, match='batch of 1'):
            loss(one, one)
    for loss in (amd.CosineSimilarityLoss(), amd.CosineSimilarityLoss(uniformity_reg=1), amd.RegularizationLoss(variance_reg=0, covariance_reg=0)):
        with pytest.raises(NotImplementedError, match='no CPU fallback'):
            loss(one, one)
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        amd.BarlowTwinsLoss()(torch.zeros(2, 1), torch.zeros(2, 1))          # two rows and one column pass the shape checks


def test_critic_loss_refuses_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    ops = importlib.import_module('3dinfomax_amd.ops')
    loss = amd.CriticLoss()
    for z2, rec in ((torch.zeros(4, 8), torch.zeros(4, 8)), (torch.zeros(4, 8), torch.zeros(4, 7, 3)), (torch.zeros(4, 8), torch.zeros(5, 8, 3)),
                    (torch.zeros(4, 8, 1), torch.zeros(4, 8, 3)), (torch.zeros(4, 8), torch.zeros(4, 8, 0))):
        with pytest.raises(ValueError, match='reconstruction'):
            loss(z2, rec)
    with pytest.raises(NotImplementedError, match=f'1..{ops.BATCHSTAT_MAX_REPEATS}'):
        loss(torch.zeros(4, 8), torch.zeros(4, 8, ops.BATCHSTAT_MAX_REPEATS + 1))
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 8, 3, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        loss(torch.zeros(1, 8), torch.zeros(1, 8, 16))              # a batch of one is legal here; CPU tensors are not


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    ops = importlib.import_module('3dinfomax_amd.ops')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_bs_max_repeats', 'i3d_bs_pass_blocks', 'i3d_bs_moments', 'i3d_bs_matrix_pass', 'i3d_bs_finish', 'i3d_bs_col_bwd',
                 'i3d_bs_rows_fwd', 'i3d_bs_rows_bwd'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_bs_max_repeats() == ops.BATCHSTAT_MAX_REPEATS == 32
    # the D x D pass takes 2048 entries per workgroup
    assert [lib.i3d_bs_pass_blocks(d) for d in (0, 1, 45, 46, 256)] == [0, 1, 1, 2, 32]
    # argument validation happens on the host before any launch: no GPU needed
    assert lib.i3d_bs_moments(None, None, 4, 8, None, None, None, None, None, None) == -1 and b'bad arguments' in lib.i3d_last_error()
    assert lib.i3d_bs_matrix_pass(None, 1, 8, 1.0, 1.0, 1.0, 1.0, None, None) == -1 and b'bad arguments' in lib.i3d_last_error()
    assert lib.i3d_bs_finish(None, 3, 1.0, None, 0, 0, 0.0, None, None) == -1 and b'bad arguments' in lib.i3d_last_error()
    assert lib.i3d_bs_col_bwd(*([None] * 8), 4, 8, None, 1.0, 1.0, 0.0, 1.0, None, None, None, None) == -1
    assert lib.i3d_bs_rows_fwd(None, None, 4, 8, 1, None, None, None) == -1 and b'bad arguments' in lib.i3d_last_error()
    assert lib.i3d_bs_rows_bwd(None, None, 4, 8, 1, None, 1.0, None, None, None, None) == -1 and b'bad arguments' in lib.i3d_last_error()
