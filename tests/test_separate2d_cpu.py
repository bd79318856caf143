"""NTXentMultiplePositivesSeparate2D / NTXentMMDSeparate2D on the host: an fp64 restatement of both formulas against the reference's own
fp64 results (fixture: tests/golden/gen_golden_separate2d.py) - which pins the orientation of the MMD matrix and the constant bandwidth -,
the plugin surface, and the refusals that fire before any library call."""
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_separate2d as GS

launcher = importlib.import_module('launch_reference')
NAMES = {'sep': 'NTXentMultiplePositivesSeparate2D', 'mmd': 'NTXentMMDSeparate2D'}
CASES = [(c, False) for c in GS.CASES] + [(GS.JITTER_CASE, True)]


def sep_restated(z1, z2, tau, norm=True, const_norm=False):
    """P = exp(S' / tau) over rows (i, l) and columns (j, u); positives: the matched conformers; the denominator leaves the whole
    C x C diagonal block out.  No epsilon.  const_norm: the norms carry no gradient (the scale of the terms the normalisation's
    projection cancels - see tests/test_gpu_separate2d.py)."""
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.reshape(B, -1, D), z2.reshape(B, -1, D)
    C = a.shape[1]
    S = torch.einsum('ilk,juk->ijlu', a, b)
    if norm:
        n = a.norm(dim=2)[:, None, :, None] * b.norm(dim=2)[None, :, None, :]
        S = S / (n.detach() if const_norm else n)
    P = torch.exp(S / tau)
    M = P.sum(dim=(2, 3))
    idx = torch.arange(B)
    pos = P[idx, idx][:, torch.arange(C), torch.arange(C)].sum(dim=1)
    return -torch.log(pos / (M.sum(dim=1) - M[idx, idx])).mean()


def mmd_restated(z1, z2, tau, norm=True, kernel_num=5, kernel_mul=2.0, const_norm=False):
    """entry [a, b]: the 2C points are the C 2D embeddings of molecule b followed by the C 3D embeddings of molecule a (rows index the
    3D view); the bandwidth is detached.  One row a at a time: nothing of size [B, B, 2C, 2C, D]."""
    B, D = z1.shape[0], z2.shape[1]
    x, y = z1.reshape(B, -1, D), z2.reshape(B, -1, D)
    C = x.shape[1]
    if norm:
        nx, ny = x.norm(dim=2, keepdim=True).clamp_min(1e-12), y.norm(dim=2, keepdim=True).clamp_min(1e-12)
        x, y = x / (nx.detach() if const_norm else nx), y / (ny.detach() if const_norm else ny)
    rows = []
    for a in range(B):
        pts = torch.cat([x, y[a].expand(B, C, D)], dim=1)                          # [B (the column b), 2C, D]
        L2 = ((pts[:, :, None, :] - pts[:, None, :, :]) ** 2).sum(dim=3)
        bw = L2.detach().sum(dim=(1, 2)) / ((2 * C) ** 2 - 2 * C) / kernel_mul ** (kernel_num // 2)
        K = sum(torch.exp(-L2 / (bw * kernel_mul ** k)[:, None, None]) for k in range(kernel_num))
        mmd = (K[:, :C, :C] + K[:, C:, C:] - K[:, :C, C:] - K[:, C:, :C]).mean(dim=(1, 2))
        rows.append(1.0 / (mmd + 1.0))
    P = torch.exp(torch.stack(rows) / tau)
    pos = torch.diagonal(P)
    return -torch.log(pos / (P.sum(dim=1) - pos)).mean()


RESTATED = {'sep': sep_restated, 'mmd': mmd_restated}


def restated(key, z1, z2, tau, dtype=torch.float64, **kw):
    """-> (loss, dz1, dz2) of the restatement in `dtype`"""
    a = torch.as_tensor(z1).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(dtype).clone().requires_grad_(True)
    loss = RESTATED[key](a, b, tau, **kw)
    loss.backward()
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize('case', CASES, ids=[GS.case_tag(*c, j) for c, j in CASES])
@pytest.mark.parametrize('key', ['sep', 'mmd'])
def test_fp64_restatement_reproduces_the_reference(key, case):
    (B, C, D), jitter = case
    z = load('separate2d.npz')
    p = f'{key}/{GS.case_tag(B, C, D, jitter)}/'
    assert z[p + 'z1'].shape == (B, C * D) and z[p + 'z2'].shape == (B * C, D)
    loss, g1, g2 = restated(key, z[p + 'z1'], z[p + 'z2'], GS.TAU)
    for name, got, ref in (('loss', loss, z[p + 'loss64']), ('dz1', g1, z[p + 'dz1_64']), ('dz2', g2, z[p + 'dz2_64'])):
        ref = torch.as_tensor(ref)
        assert ref.dtype == torch.float64
        err = (got - ref).abs().max().item()
        assert err <= 1e-10 * max(1.0, ref.abs().max().item()), (name, err)


def test_mmd_orientation_and_constant_bandwidth_matter():
    """the transposed matrix and a differentiated bandwidth both give other numbers: the restatement above is not insensitive to them"""
    z = load('separate2d.npz')
    p = f'mmd/{GS.case_tag(5, 3, 24)}/'
    z1, z2 = torch.from_numpy(z[p + 'z1']).double(), torch.from_numpy(z[p + 'z2']).double()
    # rows <-> columns: hand the views over swapped (z2 as the 2D view)
    swapped = mmd_restated(z2.reshape(5, -1), z1.reshape(15, -1), GS.TAU)
    assert abs(swapped.item() - float(z[p + 'loss64'])) > 1e-6
    a = z1.clone().requires_grad_(True)
    x, y = a.reshape(5, 3, 24), z2.reshape(5, 3, 24)
    pts = torch.cat([torch.nn.functional.normalize(x[1], dim=1), torch.nn.functional.normalize(y[0], dim=1)])
    L2 = ((pts[:, None] - pts[None]) ** 2).sum(2)
    with_grad = torch.exp(-L2 / (L2.sum() / 30)).sum()
    const = torch.exp(-L2 / (L2.detach().sum() / 30)).sum()
    g_with, = torch.autograd.grad(with_grad, a, retain_graph=True)
    g_const, = torch.autograd.grad(const, a)
    assert (g_with - g_const).abs().max() > 1e-6


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    names = launcher.plugin_names()
    for name in NAMES.values():
        assert name in amd.__all__ and name in alias.__all__
        assert getattr(amd, name) is getattr(alias, name) is getattr(losses, name) is names[name]
    sep = amd.NTXentMultiplePositivesSeparate2D(norm=False, tau=0.1, uniformity_reg=0, variance_reg=0, covariance_reg=0)
    assert sep.tau == 0.1 and sep.norm is False
    mmd = amd.NTXentMMDSeparate2D(tau=0.2, kernel_num=3, kernel_mul=1.5)
    assert (mmd.tau, mmd.kernel_num, mmd.kernel_mul, mmd.norm) == (0.2, 3, 1.5, True)
    assert amd.NTXentMMDSeparate2D().kernel_num == 5 and amd.NTXentMMDSeparate2D().kernel_mul == 2.0 and amd.NTXentMMDSeparate2D().tau == 0.5


@pytest.mark.parametrize('name', sorted(NAMES.values()))
def test_refusals_fire_on_cpu_tensors_before_any_library_call(name, monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)
    loss = getattr(amd, name)(tau=0.1)
    with pytest.raises(ValueError, match='columns'):
        loss(torch.zeros(4, 3 * 8 + 1), torch.zeros(12, 8))          # z1 is not C D wide
    with pytest.raises(ValueError, match='multiple'):
        loss(torch.zeros(4, 24), torch.zeros(13, 8))                # z2 rows not divisible by the batch
    with pytest.raises(NotImplementedError, match='1..8'):
        loss(torch.zeros(2, 9 * 4), torch.zeros(18, 4))             # nine conformers
    with pytest.raises(NotImplementedError, match='fp32'):
        loss(torch.zeros(2, 8, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    loss.attach_group(group)
    with pytest.raises(NotImplementedError, match=name):
        loss(torch.zeros(4, 24), torch.zeros(12, 8))


def test_regularisers_follow_the_reference_on_three_dimensional_views():
    """the reference hands [B, C, D] views to its regularisers: std_loss works on them, cov_loss (2-D unpack) and uniformity_loss
    (torch.pdist) raise - stated here in torch, and the classes refuse the latter two by name before any device work"""
    v = torch.randn(4, 3, 8, generator=torch.Generator().manual_seed(0))
    assert torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean().dim() == 0
    with pytest.raises(ValueError):
        batch_size, metric_dim = v.size()
    with pytest.raises(RuntimeError):
        torch.pdist(v, p=2)
    for name in NAMES.values():
        with pytest.raises(NotImplementedError, match='covariance_reg'):
            getattr(amd, name)(covariance_reg=0.1, tau=0.1)._regularisers(torch.zeros(()), v, v)
        with pytest.raises(NotImplementedError, match='uniformity_reg'):
            getattr(amd, name)(uniformity_reg=0.1, tau=0.1)._regularisers(torch.zeros(()), v, v)
        got = getattr(amd, name)(variance_reg=0.5, tau=0.1)._regularisers(torch.zeros(()), v, v)
        assert abs(got.item() - torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean().item()) < 1e-6


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_row_normalize_fwd', 'i3d_row_normalize_bwd', 'i3d_sep2d_max_conformers', 'i3d_sep2d_fwd', 'i3d_sep2d_bwd',
                 'i3d_mmd_pair_fwd', 'i3d_mmd_pair_bwd'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    ops = importlib.import_module('3dinfomax_amd.ops')
    assert lib.i3d_sep2d_max_conformers() == ops.SEP2D_MAX_CONFORMERS == 8
    # argument validation happens on the host before any launch: no GPU needed
    assert lib.i3d_sep2d_fwd(None, None, None, 4, 9, 0.1, None, None, None, None) == -1 and b'1..8' in lib.i3d_last_error()
    assert lib.i3d_mmd_pair_fwd(None, None, 1, 2, 8, 5, 2.0, None, None, None, None, None) == -1
    assert b'two molecules' in lib.i3d_last_error()
