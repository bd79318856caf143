"""NTXentMultiplePositivesSeparate2D / NTXentMMDSeparate2D on the MI355X (csrc/sep2d.hip): accuracy against the reference's fp64 results
with the reference's own fp32 error as the yardstick, shapes past the kernels' tile and wave edges, the composed paths, the row
normalisation alone, determinism, the end-to-end fixture, memory, and the absence of host synchronisation.

The rule of every accuracy check: err = error against fp64, err_ref = error of the reference (fixture) or of the same formula in torch
fp32 (shapes computed here) against fp64 on the same inputs; err <= max(4 err_ref, 1e-6).  The factor covers another summation order
and the device exp; the floor covers cases where fp32 torch happens to be exact.  Errors are max-norm: a gradient's relative to its
largest entry, the loss's relative to max(|loss|, 1) - the loss is a difference of logarithms of size up to 1 / tau >= 1 and is exactly 0
for the MMD loss at C = 1 (the bandwidth scales with the only distance there is, so every similarity is the same number).

Every check prints err_ref and the kernel's error before it asserts; the table of DESIGN.md ('Conformer-wise losses') holds err_ref per
fixture case, the kernel column there is still open."""
import functools
import importlib

import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz

import gen_golden_separate2d as GS
from test_separate2d_cpu import CASES, NAMES, restated

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
losses = importlib.import_module('3dinfomax_amd.losses')
DEV = torch.device('cuda:0')
FLOOR = 1e-6


def _loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def _grad_err(got, ref, scale=None):
    a, b = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    denom = max(b.abs().max().item(), scale or 0.0, 1e-6)          # a gradient that is exactly zero in fp64 has to stay below 1e-12
    return (a - b).abs().max().item() / denom


def _ours(key, z1, z2, tau=GS.TAU, **kw):
    a = torch.as_tensor(z1).to(DEV).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(DEV).clone().requires_grad_(True)
    loss = getattr(amd, NAMES[key])(tau=tau, **kw)(a, b)
    loss.backward()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _judge(what, ours, ref32, ref64, scales=(None, None)):
    """print every figure, then assert the rule on loss, dz1, dz2"""
    rows = [('loss', _loss_err(ours[0], ref64[0]), _loss_err(ref32[0], ref64[0]))]
    for k, name in ((1, 'dz1'), (2, 'dz2')):
        rows.append((name, _grad_err(ours[k], ref64[k], scales[k - 1]), _grad_err(ref32[k], ref64[k], scales[k - 1])))
    for name, e, e_ref in rows:
        print(f'{what} {name}: err_ref {e_ref:.3e} kernel {e:.3e}')
    for o in ours:
        assert torch.isfinite(torch.as_tensor(o)).all()
    bad = [(name, e, e_ref) for name, e, e_ref in rows if not e <= max(4 * e_ref, FLOOR)]
    assert not bad, bad


@pytest.mark.parametrize('case', CASES, ids=[GS.case_tag(*c, j) for c, j in CASES])
@pytest.mark.parametrize('key', ['sep', 'mmd'])
def test_matches_reference_fixture(key, case):
    """loss, dz1 and dz2 of every fixture case against the fixture's fp64 values; err_ref = the fixture's fp32 values against them"""
    (B, C, D), jitter = case
    z = load('separate2d.npz')
    p = f'{key}/{GS.case_tag(B, C, D, jitter)}/'
    ours = _ours(key, z[p + 'z1'], z[p + 'z2'])
    ref32 = (z[p + 'loss32'], z[p + 'dz1_32'], z[p + 'dz2_32'])
    ref64 = (z[p + 'loss64'], z[p + 'dz1_64'], z[p + 'dz2_64'])
    _judge(p, ours, ref32, ref64)


def _inputs(B, C, D, scale=1.0):
    g = torch.Generator().manual_seed(100 * B + 10 * C + D)
    return scale * torch.randn(B, C * D, generator=g), scale * torch.randn(B * C, D, generator=g)


@functools.lru_cache(maxsize=None)
def _references(key, B, C, D, scale=1.0, kw=()):
    """(fp32, fp64, (scale of dz1, of dz2)) of the restatement of tests/test_separate2d_cpu.py, computed once per case.  At D = 1 with
    normalisation the projection of the normalisation's backward removes the whole gradient: what is left in any fp32 implementation is
    the rounding of the two cancelling terms, so the error is taken relative to those terms - the gradient with the norms held constant."""
    z1, z2 = _inputs(B, C, D, scale)
    kw = dict(kw)
    r32 = restated(key, z1, z2, GS.TAU, torch.float32, **kw)
    r64 = restated(key, z1, z2, GS.TAU, torch.float64, **kw)
    scales = (None, None)
    if D == 1 and kw.get('norm', True):
        _, g1, g2 = restated(key, z1, z2, GS.TAU, torch.float64, const_norm=True, **kw)
        scales = (g1.abs().max().item(), g2.abs().max().item())
    assert torch.isfinite(r64[0]) and torch.isfinite(r64[1]).all() and torch.isfinite(r64[2]).all()
    return r32, r64, scales


@pytest.mark.parametrize('shape', [(65, 3, 256), (33, 5, 256), (2, 8, 1)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key', ['sep', 'mmd'])
def test_kernel_boundaries_match_fp64(key, shape):
    """B C = 195 and 165 (no multiple of the 64-wide tiles, of the 8 rows of the gradient kernel or of the 16 columns of the column pass),
    D = 256 (eight LDS chunks; one full feature block of the gradient kernel) and D = 1 with the largest C"""
    B, C, D = shape
    r32, r64, scales = _references(key, B, C, D)
    z1, z2 = _inputs(B, C, D)
    _judge(f'{key} {shape}', _ours(key, z1, z2), r32, r64, scales)


def test_separate2d_without_normalisation():
    B, C, D = 5, 3, 24
    kw = (('norm', False),)
    r32, r64, scales = _references('sep', B, C, D, 0.2, kw)
    z1, z2 = _inputs(B, C, D, 0.2)
    _judge('sep norm=False', _ours('sep', z1, z2, norm=False), r32, r64, scales)


def test_mmd_with_three_kernels_and_another_multiplier():
    B, C, D = 5, 3, 24
    kw = (('kernel_mul', 1.5), ('kernel_num', 3))
    r32, r64, scales = _references('mmd', B, C, D, 1.0, kw)
    z1, z2 = _inputs(B, C, D)
    _judge('mmd kernel_num=3 kernel_mul=1.5', _ours('mmd', z1, z2, kernel_num=3, kernel_mul=1.5), r32, r64, scales)
    # and without normalisation (the composed path that skips the row-normalise kernels)
    kw = (('norm', False),)
    r32, r64, scales = _references('mmd', B, C, D, 0.2, kw)
    z1, z2 = _inputs(B, C, D, 0.2)
    _judge('mmd norm=False', _ours('mmd', z1, z2, norm=False), r32, r64, scales)


def test_variance_regulariser_on_the_views():
    B, C, D = 5, 3, 24
    z1, z2 = _inputs(B, C, D)
    for key in ('sep', 'mmd'):
        base = _ours(key, z1, z2)
        got = _ours(key, z1, z2, variance_reg=0.5)
        a, b = z1.double().reshape(B, C, D), z2.double().reshape(B, C, D)
        if key == 'mmd':
            a, b = torch.nn.functional.normalize(a, dim=2), torch.nn.functional.normalize(b, dim=2)
        std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()
        assert abs((got[0] - base[0]).item() - 0.5 * (std(a) + std(b)).item()) < 1e-5
        assert (got[1] - base[1]).abs().max() > 0
    for key in ('sep', 'mmd'):
        with pytest.raises(NotImplementedError, match='covariance_reg'):
            _ours(key, z1, z2, covariance_reg=0.1)
        with pytest.raises(NotImplementedError, match='uniformity_reg'):
            _ours(key, z1, z2, uniformity_reg=0.1)


def test_row_normalise_with_an_all_zero_row():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(7, 37, generator=g)
    x[2] = 0
    dy = torch.randn(7, 37, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = losses._RowNormalizeFn.apply(xd)
    y.backward(dy.to(DEV))
    x64 = x.double().requires_grad_(True)
    y64 = torch.nn.functional.normalize(x64, dim=1)
    y64.backward(dy.double())
    assert torch.count_nonzero(y[2]) == 0
    assert torch.isfinite(xd.grad).all()
    keep = [0, 1, 3, 4, 5, 6]
    assert rel_err(y.detach().cpu()[keep], y64.detach()[keep]) < 1e-6
    assert rel_err(xd.grad.cpu()[keep], x64.grad[keep]) < 1e-6
    assert rel_err(xd.grad.cpu()[2], x64.grad[2]) < 1e-6          # below the clamp: dy / 1e-12, as torch


@pytest.mark.parametrize('key', ['sep', 'mmd'])
def test_two_runs_are_bit_identical(key):
    z1, z2 = _inputs(33, 5, 256)
    a, b = _ours(key, z1, z2), _ours(key, z1, z2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _e2e_batch(z):
    mols = mols_from_npz(z, 'e2e/mol')
    coords, off, items = z['e2e/conf_coords'], 0, []
    for m in mols:
        cs = []
        for _ in range(GS.E2E_CONF):
            cs.append(amd.complete_graph(m, coords[off:off + m.n_atoms]))
            off += m.n_atoms
        items.append((amd.bond_graph(m), amd.batch(cs)))
    (g2,), (g3,) = amd.conformer_collate(items)
    return g2.to(DEV), g3.to(DEV)


@pytest.mark.parametrize('key', ['sep', 'mmd'])
def test_end_to_end_matches_reference_fixture(key):
    """4 molecules x 2 conformers through PNA and Net3D: loss and embeddings at 1e-4, parameter gradients by helpers.grads_close at the
    5e-4 of the other small-model fixtures"""
    z = load('separate2d.npz')
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **GS.PNA_KW)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **GS.NET3D_KW)
    pna.load_state_dict(sd_from_npz(z, 'e2e/pna_sd'), strict=True)
    net.load_state_dict(sd_from_npz(z, 'e2e/net3d_sd'), strict=True)
    pna.to(DEV).train(), net.to(DEV).train()
    g2, g3 = _e2e_batch(z)
    z1, z2 = pna(g2), net(g3)
    loss = getattr(amd, NAMES[key])(tau=GS.TAU)(z1, z2)
    loss.backward()
    p = f'e2e/{key}/'
    print(f'{p} loss {loss.item():.7f} reference {float(z[p + "loss"]):.7f} z1 {rel_err(z1.detach().cpu(), z[p + "z1"]):.2e} '
          f'z2 {rel_err(z2.detach().cpu(), z[p + "z2"]):.2e}')
    assert rel_err(z1.detach().cpu(), z[p + 'z1']) < 1e-4 and rel_err(z2.detach().cpu(), z[p + 'z2']) < 1e-4
    assert abs(loss.item() - float(z[p + 'loss'])) < 1e-4 * abs(float(z[p + 'loss']))
    for model, tag in ((pna, 'pna_grad'), (net, 'net3d_grad')):
        ref = sd_from_npz(z, p + tag)
        got = {k: q.grad.detach().cpu() for k, q in model.named_parameters() if q.grad is not None}
        assert set(got) == set(ref)
        grads_close(got, ref, 5e-4, what=f'{p}{tag}: ')


def test_mmd_memory_stays_far_below_the_pairwise_tensor():
    """(256, 5, 256): the reference's [B, B, 2C, 2C, D] tensor is 1.3 GB per copy; forward + backward here allocate B^2 C^2 floats twice
    (cross and its gradient, 6.5 MB each) plus the views"""
    B, C, D = 256, 5, 256
    z1, z2 = _inputs(B, C, D)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = amd.NTXentMMDSeparate2D(tau=GS.TAU)
    loss_fn(a, b).backward()          # the library's first load, workspaces
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = loss_fn(a, b)
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f'mmd (256, 5, 256): peak growth {growth / 2 ** 20:.1f} MB')
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert growth < 64 * 2 ** 20


@pytest.mark.parametrize('key', ['sep', 'mmd'])
def test_step_does_not_synchronise(key):
    z1, z2 = _inputs(33, 5, 256)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = getattr(amd, NAMES[key])(tau=GS.TAU)

    def step():
        loss = loss_fn(a, b)
        (2.0 * loss).backward()
        return loss
    step()                                   # allocations, workspaces, the library's first load
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
