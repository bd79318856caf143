"""BarlowTwinsLoss / CosineSimilarityLoss / RegularizationLoss / CriticLoss on the MI355X (csrc/batchstat.hip): accuracy against the
reference's fp64 results with the reference's own fp32 error as the yardstick, shapes at the kernels' edges, a zero row, cross-checks that
need no reference, a non-unit upstream gradient, determinism and the absence of host synchronisation.

The rule of every accuracy check (that of tests/test_gpu_hardneg.py): err = max-norm error against fp64, a gradient's relative to its
largest entry, the loss's relative to max(|loss|, 1); err_ref = the error of the reference's fp32 (fixture: 'err32') or of the same formula
in torch fp32 on the CPU (shapes computed here) against fp64 on the same inputs; err <= max(4 err_ref, 1e-6).  Every check prints err_ref
and the kernel's error before it asserts.

Inputs outside the fixture follow the fixture's recipe and meet its hinge condition: every column further than 1e-3 from the kink of
relu(1 - sqrt(var + 1e-4)) in fp64, so the kernels, fp32 torch and fp64 torch take the same side."""
import functools
import importlib

import pytest
import torch

from helpers import amd, load

import gen_golden_batchstat as GB
import gen_golden_hardneg as GH
from test_batchstat_cpu import CASES, CASE_IDS, case_setup, restated, restated_kwargs

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
DEV = torch.device('cuda:0')
FLOOR = 1e-6
NAMES = dict(GB.LOSSES)
REGS = dict(GB.REGS)


def _ours(key, x, y, scale=1.0, **kw):
    a = torch.as_tensor(x).to(DEV).clone().requires_grad_(True)
    b = torch.as_tensor(y).to(DEV).clone().requires_grad_(True)
    loss = getattr(amd, NAMES[key])(**kw)(a, b)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (scale * loss).backward()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _judge(what, ours, ref64, err_ref):
    """print every figure, then assert the rule on the loss and the two gradients"""
    rows = [('loss', GH.loss_err(ours[0], ref64[0]), err_ref[0])]
    for k, name in ((1, 'g1'), (2, 'g2')):
        rows.append((name, GH.grad_err(ours[k], ref64[k]), err_ref[k]))
    for name, e, e_ref in rows:
        print(f'{what} {name}: err_ref {e_ref:.3e} kernel {e:.3e}')
    for o, r in zip(ours, ref64):
        assert torch.isfinite(torch.as_tensor(o)).all() and tuple(torch.as_tensor(o).shape) == tuple(torch.as_tensor(r).shape)
    bad = [(name, e, e_ref) for name, e, e_ref in rows if not e <= max(4 * e_ref, FLOOR)]
    assert not bad, bad


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_matches_reference_fixture(case):
    """loss and both gradients of every fixture case against the fixture's fp64 values.  (2, 8) is the smallest legal batch: one pass of
    the column kernel with 14 of its 16 row lanes idle; BarlowTwins' gradient is analytically zero there (both standardised views are
    +-2^-1/2 whatever the input), so 'err32' and the kernel's error are both rounding noise over the 1e-6 floor of the measure"""
    key, shape, tag = case
    z = load('batchstat.npz')
    p = GB.case_prefix(key, shape, tag)
    x, y, kw, _ = case_setup(z, key, shape, tag)
    ref64 = (z[p + 'loss64'], GH.decode(z, p, 'g1'), GH.decode(z, p, 'g2'))
    _judge(p, _ours(key, x, y, **kw), ref64, tuple(z[p + 'err32']))


def _restated_errors(r32, r64):
    return (GH.loss_err(r32[0], r64[0]), GH.grad_err(r32[1], r64[1]), GH.grad_err(r32[2], r64[2]))


@functools.lru_cache(maxsize=None)
def _pair(B, D):
    z1, z2, seed = GB.base_inputs(B, D)
    print(f'pair {(B, D)}: seed {seed}')
    return z1, z2


@functools.lru_cache(maxsize=None)
def _case(key, B, D, R=0, **kw):
    """(the loss's two arguments, fp64 reference, err_ref) of a shape outside the fixture, computed once and left unchanged"""
    x, y = GB.case_inputs(*_pair(B, D), kw, R)
    rk = restated_kwargs(key, kw)
    r32, r64 = restated(key, x, y, torch.float32, **rk), restated(key, x, y, torch.float64, **rk)
    assert all(torch.isfinite(t).all() for t in r32 + r64)
    return x, y, r64, _restated_errors(r32, r64)


EDGES = [(257, 40), (300, 256), (66, 7), (20, 46), (33, 1)]


@pytest.mark.parametrize('shape', EDGES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key,kw', [('barlow', REGS), ('cosine', REGS), ('regularization', {})], ids=['barlow', 'cosine', 'regularization'])
def test_kernel_edges_match_fp64(key, kw, shape):
    """every term switched on.  The column kernels' workgroups are 16 columns x 16 row lanes, the D x D pass takes 2048 entries per
    workgroup, the row kernels one 256-thread workgroup per row, the final sum one workgroup:
    (257, 40): one row past 16 full passes of the row lanes; three column workgroups, the last half empty; 257 row terms: a second pass
        of the final sum; a row of the row kernel shorter than its workgroup
    (300, 256): the configs' width: 16 column workgroups, 32 workgroups of the D x D pass, a row exactly one pass of the row kernel
    (66, 7): odd width, one column workgroup with 9 idle columns; two rows past 64
    (20, 46): 46^2 = 2116 entries: a second workgroup of the D x D pass with 68 entries
    (33, 1): one column: the off-diagonal sums are empty and the covariance term is 0
    (the smallest legal batch, (2, 8), is in the fixture)"""
    x, y, r64, err_ref = _case(key, *shape, **kw)
    _judge(f'{key} {shape}', _ours(key, x, y, **kw), r64, err_ref)


@pytest.mark.parametrize('shape', [(33, 24, 10), (5, 13, 1), (64, 256, 3), (9, 40, 32)], ids=lambda s: 'x'.join(map(str, s)))
def test_critic_loss_matches_fp64(shape):
    """(33, 24, 10): the repeats of configs/old_configs/philosophy.yml; 250 of the 256 threads keep a repeat each (256 is no multiple of
    10), 240 floats per row: less than one pass; (5, 13, 1): the two-view layout; (64, 256, 3): the configs' width, 255 threads, 768 floats
    per row: four passes, the last partial; (9, 40, 32): the largest repeat count, all 256 threads, five full passes"""
    B, D, R = shape
    x, y, r64, err_ref = _case('critic', B, D, R)
    assert y.shape == shape
    _judge(f'critic {shape}', _ours('critic', x, y), r64, err_ref)


def test_a_zero_row_keeps_the_constant_denominator():
    """CosineSimilarityLoss with one all-zero row in z1: x_hat = 0 / 1e-12 = 0 and the row's gradient is g / 1e-12, as F.normalize's; the
    zero row and the other rows are judged apart, each by the rule, since the zero row's gradient is 1e12 times the others'"""
    z1, z2 = _pair(66, 7)
    z1 = z1.clone()
    z1[5] = 0
    r32, r64 = restated('cosine', z1, z2, torch.float32), restated('cosine', z1, z2, torch.float64)
    ours = _ours('cosine', z1, z2)
    zero = torch.zeros(66, 1, dtype=torch.bool)
    zero[5] = True
    assert r64[1][5].abs().max() > 1e6
    for what, part in (('zero row', zero), ('other rows', ~zero)):
        pick = lambda r: (r[0], r[1] * part, r[2])
        _judge(f'cosine, {what}', pick(ours), pick(r64), _restated_errors(pick(r32), pick(r64)))


def test_moments_come_from_centred_values():
    """columns with mean 1000 and standard deviation 1: E[x^2] - E[x]^2 in fp32 would keep no digit of the variance.  The kernel sums in
    fp64: mean and variance against fp64 torch at 1e-12 relative; the views a = (z - mean) / std and c = z - mean are the fp32 roundings
    of the fp64 values: 2^-24 relative and 2^-24 of the spacing of z (2^-14 at 1000) absolute for the subtraction, which is exact"""
    g = torch.Generator().manual_seed(11)
    z1 = (1000.0 + torch.randn(257, 40, generator=g)).contiguous()
    z2 = (-3.0 + 0.01 * torch.randn(257, 40, generator=g)).contiguous()
    mom, a, c = ops.bs_moments(z1.to(DEV), z2.to(DEV), standardised=True, centred=True)
    mom = mom.cpu()
    for v, z in enumerate((z1.double(), z2.double())):
        mean, var = z.mean(dim=0), z.var(dim=0)
        e_mean = ((mom[v, 0] - mean).abs() / mean.abs()).max().item()
        e_var = ((mom[v, 1] - var).abs() / var).max().item()
        print(f'view {v}: mean {e_mean:.2e} variance {e_var:.2e}')
        assert e_mean <= 1e-12 and e_var <= 1e-12
        want_c, want_a = z - mean, (z - mean) / var.sqrt()
        assert (c[v].cpu().double() - want_c).abs().max().item() <= 2.0 ** -24 * want_c.abs().max().item()
        assert (a[v].cpu().double() - want_a).abs().max().item() <= 2.0 ** -24 * want_a.abs().max().item()


def test_cosine_loss_is_two_minus_twice_the_mean_cosine():
    """from ops.row_norms and the library's GEMM.  Bound: a cosine from the fp32 product and two fp32 norms carries a few roundings of
    2^-24 each, at most 8 * 2^-24 for |cos| <= 1; twice that in 2 - 2 cos: 2^-20 = 9.5e-7"""
    z1, z2 = _pair(300, 256)
    a, b = z1.to(DEV), z2.to(DEV)
    cos = torch.diagonal(ops.gemm(a, b, trans_b=True)) / (ops.row_norms(a) * ops.row_norms(b))
    want = 2.0 - 2.0 * cos.double().mean().item()
    got = amd.CosineSimilarityLoss()(a, b).item()
    print(f'CosineSimilarityLoss {got:.8f} 2 - 2 mean cos {want:.8f}')
    assert abs(got - want) <= 2.0 ** -20


def test_critic_loss_with_one_repeat_is_the_cosine_loss():
    """the same kernel with the same arguments: the same bits"""
    x, y, _, _ = _case('critic', 33, 24, 1)
    assert y.shape == (33, 24, 1)
    critic = _ours('critic', x, y)
    cosine = _ours('cosine', x, y.squeeze(2))
    assert torch.equal(critic[0], cosine[0]) and torch.equal(critic[1], cosine[1]) and torch.equal(critic[2].squeeze(2), cosine[2])


@pytest.mark.parametrize('shape', [(66, 7), (20, 46)], ids=lambda s: 'x'.join(map(str, s)))
def test_barlow_twins_of_a_view_with_itself(shape):
    """C_ii = (B - 1) / B for a standardised view against itself, so with lambd = 0 the loss is scale_loss D / B^2.  Bound: C_ii carries
    the fp32 roundings of a (2^-24 each, twice in a square) and of the product's sum, at most 8 * 2^-24 relative to a value near 1;
    C_ii - 1 = -1 / B turns that into 8 B 2^-24 relative, and the square doubles it: 2^-20 B"""
    B, D = shape
    z1, _ = _pair(B, D)
    a = z1.to(DEV)
    got = amd.BarlowTwinsLoss(scale_loss=0.5, lambd=0)(a, a.clone()).item()
    want = 0.5 * D / B ** 2
    print(f'BarlowTwinsLoss(z, z) {got:.9e} scale_loss D / B^2 {want:.9e}')
    assert abs(got - want) <= 2.0 ** -20 * B * want


@pytest.mark.parametrize('key', sorted(NAMES))
def test_upstream_gradient_scales_the_gradients(key):
    """(3 * loss).backward(): the factor reaches both gradients through the device scalar.  Bound: the factor is applied in fp64 before
    the one fp32 rounding of a term's gradient (2^-24 of the entry, on either side); where a loss is the sum of a row term and a column
    term autograd adds the two rounded gradients with one more rounding, and the two may cancel in an entry, so the bound is relative to
    the largest entry m.  g = fl(fl(a) + fl(b)) is within 3 * 2^-24 m of a + b, the same for 3 a + 3 b within 9 * 2^-24 m, so
    |g(3) - 3 g(1)| <= 18 * 2^-24 m < 2^-19 m"""
    kw = REGS if key in ('barlow', 'cosine') else {}
    x, y, _, _ = _case(key, 66, 7, 3 if key == 'critic' else 0, **kw)
    one, three = _ours(key, x, y, **kw), _ours(key, x, y, scale=3.0, **kw)
    assert torch.equal(one[0], three[0])
    for g1, g3 in zip(one[1:], three[1:]):
        assert g1.abs().max() > 0 and (g3 - 3.0 * g1).abs().max() <= 2.0 ** -19 * g1.abs().max()


@pytest.mark.parametrize('key', sorted(NAMES))
def test_two_runs_are_bit_identical(key):
    kw = REGS if key in ('barlow', 'cosine') else {}
    x, y, _, _ = _case(key, 257, 40, 10 if key == 'critic' else 0, **kw)
    a, b = _ours(key, x, y, **kw), _ours(key, x, y, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('key', sorted(NAMES))
def test_step_does_not_synchronise(key):
    """forward and backward under torch's sync debug mode, the upstream gradient a device scalar"""
    kw = REGS if key in ('barlow', 'cosine') else {}
    x, y, _, _ = _case(key, 66, 7, 3 if key == 'critic' else 0, **kw)
    a, b = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss_fn = getattr(amd, NAMES[key])(**kw)

    def step():
        loss = loss_fn(a, b)
        (2.0 * loss).backward()
        return loss
    step()                                   # allocations, workspaces, the library's first load
    once = (a.grad.clone(), b.grad.clone())
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert torch.equal(a.grad, once[0]) and torch.equal(b.grad, once[1])
