"""InfoNCE / InfoNCEHard / NTXentHard / NTXentExtraNegatives / NTXentShuffled on the MI355X (csrc/hardneg.hip): accuracy against the
reference's fp64 results with the reference's own fp32 error as the yardstick, shapes at the kernels' edges, row shards on one GPU, the
modes against each other, both normalisation settings, the regularisers, the shuffled control, determinism and the absence of host
synchronisation.

The rule of every accuracy check (that of tests/test_gpu_confmatch.py): err = max-norm error against fp64, a gradient's relative to its
largest entry, the loss's relative to max(|loss|, 1); err_ref = the error of the reference's fp32 (fixture: 'err32') or of the same formula
in torch fp32 on the CPU (shapes computed here) against fp64 on the same inputs; err <= max(4 err_ref, 1e-6).  Every check prints err_ref
and the kernel's error before it asserts.

Inputs of the hard pair outside the fixture meet the fixture's clamp condition: every row's Ng is further than 1e-3 (relative) from the
clamp in fp64, so the fp32 kernels, fp32 torch and fp64 torch take the same branch."""
import functools
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_hardneg as GH
from test_hardneg_cpu import CASES, CASE_IDS, case_setup, restated, restated_kwargs

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
losses = importlib.import_module('3dinfomax_amd.losses')
DEV = torch.device('cuda:0')
FLOOR = 1e-6
NAMES = dict(GH.LOSSES)
KERNEL_KEYS = ['infonce', 'ntxent_hard', 'infonce_hard', 'extra']
MODE = {'infonce': 'infonce', 'ntxent_hard': 'ntxent_hard', 'infonce_hard': 'infonce_hard', 'extra': 'extra_negatives'}


def _ours(key, z1, z2, seed=None, scale=1.0, **kw):
    a = torch.as_tensor(z1).to(DEV).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(DEV).clone().requires_grad_(True)
    if seed is not None:
        torch.manual_seed(seed)
    loss = getattr(amd, NAMES[key])(**kw)(a, b)
    (scale * loss).backward()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _judge(what, ours, ref64, err_ref):
    """print every figure, then assert the rule on loss, dz1, dz2"""
    rows = [('loss', GH.loss_err(ours[0], ref64[0]), err_ref[0])]
    for k, name in ((1, 'dz1'), (2, 'dz2')):
        rows.append((name, GH.grad_err(ours[k], ref64[k]), err_ref[k]))
    for name, e, e_ref in rows:
        print(f'{what} {name}: err_ref {e_ref:.3e} kernel {e:.3e}')
    for o, r in zip(ours, ref64):
        assert torch.isfinite(torch.as_tensor(o)).all() and tuple(torch.as_tensor(o).shape) == tuple(torch.as_tensor(r).shape)
    bad = [(name, e, e_ref) for name, e, e_ref in rows if not e <= max(4 * e_ref, FLOOR)]
    assert not bad, bad


def _fixture_reference(z, p):
    return (z[p + 'loss64'], GH.decode(z, p, 'dz1'), GH.decode(z, p, 'dz2')), tuple(z[p + 'err32'])


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_matches_reference_fixture(case):
    """loss, dz1 and dz2 of every fixture case against the fixture's fp64 values; NTXentShuffled under the fixture's seed"""
    key, shape, tag = case
    z = load('hardneg.npz')
    p = GH.case_prefix(key, shape, tag)
    z1, z2, kw, _ = case_setup(z, key, shape, tag)
    ref64, err_ref = _fixture_reference(z, p)
    _judge(p, _ours(key, z1, z2, seed=int(z[p + 'seed']) if key == 'shuffled' else None, **kw), ref64, err_ref)


def _restated_errors(r32, r64):
    return (GH.loss_err(r32[0], r64[0]), GH.grad_err(r32[1], r64[1]), GH.grad_err(r32[2], r64[2]))


@functools.lru_cache(maxsize=None)
def _case(key, B, D, U=0, norm=None, **kw):
    """(z1, z2, constructor kwargs, fp64 reference, err_ref) of a shape outside the fixture, computed once and left unchanged: inputs by
    the fixture's recipe with a pool of U extras, from the first seed of 1000 B + D, + 100000, ... whose fp32 results are finite and -
    hard pair - whose rows keep the fixture's margin from the clamp"""
    norm = GH.DEFAULT_NORM[key] if norm is None else norm
    ctor = dict(kw, norm=norm)
    rk = restated_kwargs(key, ctor)
    seed = 1000 * B + D
    while True:
        g = torch.Generator().manual_seed(seed)
        z1 = torch.randn(B, D, generator=g)
        z2 = torch.tensor([0.0, 0.5, 3.0])[torch.arange(B) % 3][:, None] * z1 + torch.randn(B, D, generator=g)
        x = torch.randn(B, max(U, 1), D, generator=g)
        z1, z2 = GH.case_inputs(z1, z2, x, norm, U)
        r32 = restated(key, z1, z2, torch.float32, **rk)
        finite = all(torch.isfinite(t).all() for t in r32)
        margin = GH.clamp_figures(z1, z2, norm, **{k: rk[k] for k in ('tau', 'tau_plus', 'beta')})[1] if key in GH.HARD else 1.0
        if finite and margin > GH.MARGIN:
            break
        seed += 100000
    r64 = restated(key, z1, z2, torch.float64, **rk)
    assert all(torch.isfinite(t).all() for t in r64)
    print(f'{key} {(B, D, U)} {ctor}: seed {seed} margin {margin:.2e}')
    return z1, z2, ctor, r64, _restated_errors(r32, r64)


@pytest.mark.parametrize('shape', [(257, 40), (300, 256), (66, 7)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key', ['infonce', 'ntxent_hard', 'infonce_hard'])
def test_kernel_edges_match_fp64(key, shape):
    """(257, 40): one column past a 256-thread pass of the row kernel, 33 column workgroups of 8, rows read one float at a time; (300, 256):
    the size of the configs, rows read four floats at a time, a second pass of the column workgroups' 256 rows; (66, 7): odd width, two
    columns past 64.  tau = 0.1 for the normalised pair; InfoNCEHard, which does not normalise, at its default tau = 0.5.  Without
    normalisation at tau = 0.1 the logits reach 30 here, and the rounding a 256-term fp32 dot product accumulates is multiplied by 1 / tau
    and by the cancellation in Ng: at (300, 256) the fp32 CPU result itself is 4.4e-6 from fp64 with one host's sgemm and 5.5e-5 with
    another's (the kernels: 6.4e-5), so that input has no stable yardstick.  The fixture pins InfoNCEHard at tau = 0.1 up to (64, 64)."""
    z1, z2, kw, r64, err_ref = _case(key, *shape, **({} if key == 'infonce_hard' else {'tau': 0.1}))
    _judge(f'{key} {shape}', _ours(key, z1, z2, **kw), r64, err_ref)


@pytest.mark.parametrize('weight', [1, 50])
def test_ten_extra_negatives_match_fp64(weight):
    """U = 10 at (33, 24), the count of configs/old_configs/contrastive_training_noised_3d.yml"""
    z1, z2, kw, r64, err_ref = _case('extra', 33, 24, 10, tau=0.1, extra_negatives_weight=weight)
    assert z2.shape == (33 * 11, 24)
    _judge(f'extra U=10 w={weight}', _ours('extra', z1, z2, **kw), r64, err_ref)


def test_no_extra_negatives_is_ntxent_without_epsilon():
    """U = 0 is a valid layout: the loss of NTXentShuffled's formula under the identity permutation"""
    z1, z2, _, _, _ = _case('infonce', 66, 7, tau=0.1)
    rk = dict(norm=True, tau=0.1, perm=np.arange(66))
    r64 = restated('shuffled', z1, z2, torch.float64, **rk)
    err_ref = _restated_errors(restated('shuffled', z1, z2, torch.float32, **rk), r64)
    _judge('extra U=0', _ours('extra', z1, z2, tau=0.1), r64, err_ref)


@pytest.mark.parametrize('key', KERNEL_KEYS)
def test_row_shards_add_up_to_the_full_batch(key):
    """z1 in row blocks of 20, 1 and 46 rows, each with its pos_offset and the global batch of 67: the shares sum to the loss, the blocks'
    dz2 sum to dz2, their dz1 concatenate to dz1 - all against the fixture's fp64 by the rule"""
    tag = {'extra': 'tau0.1_U3_w1'}.get(key, 'tau0.1')
    z = load('hardneg.npz')
    p = GH.case_prefix(key, (67, 13), tag)
    z1, z2, kw, U = case_setup(z, key, (67, 13), tag)
    ref64, err_ref = _fixture_reference(z, p)
    B = 67
    rk = restated_kwargs(key, kw)
    other = z2[:B].to(DEV)
    share_sum, dz1_blocks, dz2_sum, dx_blocks = 0.0, [], torch.zeros(B, 13, dtype=torch.float64), []
    for lo, hi in ((0, 20), (20, 21), (21, 67)):
        a = z1[lo:hi].to(DEV).requires_grad_(True)
        b = other.clone().requires_grad_(True)
        x = z2[B + lo * U:B + hi * U].to(DEV).requires_grad_(True) if U else None
        share = losses._HardNegFn.apply(a, b, x, ops.HARDNEG_MODES[MODE[key]], rk['norm'], rk['tau'], rk.get('tau_plus', 0.0),
                                        rk.get('beta', 0.0), float(rk.get('extra_negatives_weight', 1)), lo, B)
        share.backward()
        share_sum += share.item()
        dz1_blocks.append(a.grad.cpu())
        dz2_sum += b.grad.cpu().double()
        if U:
            dx_blocks.append(x.grad.cpu().double())
    ours = (torch.tensor(share_sum), torch.cat(dz1_blocks), torch.cat([dz2_sum] + dx_blocks))
    _judge(f'{key} shards', ours, ref64, err_ref)


def test_the_modes_are_not_aliases_of_each_other():
    z = load('hardneg.npz')
    z1, z2, _, _ = case_setup(z, 'infonce', (67, 13), 'tau0.1')
    a, b = z1.to(DEV), z2.to(DEV)
    values = {name: getattr(amd, name)(tau=0.1)(a, b).item() for name in ('InfoNCE', 'NTXentHard', 'NTXent')}
    values['InfoNCEHard'] = amd.InfoNCEHard(norm=True, tau=0.1)(a, b).item()
    print(values)
    names = sorted(values)
    for i, m in enumerate(names):
        for n in names[i + 1:]:
            assert abs(values[m] - values[n]) > 1e-3, (m, n)


def test_hard_weights_switched_off_give_ntxent_without_epsilon():
    """beta = 0 and tau_plus = 0: Ng_i = S_i, which normalised inputs never clamp (every P_ij >= e^(-1/tau))"""
    z1, z2, _, _, _ = _case('infonce', 257, 40, tau=0.1)
    rk = dict(norm=True, tau=0.1, perm=np.arange(257))
    r64 = restated('shuffled', z1, z2, torch.float64, **rk)
    err_ref = _restated_errors(restated('shuffled', z1, z2, torch.float32, **rk), r64)
    ours = _ours('ntxent_hard', z1, z2, tau=0.1, beta=0, tau_plus=0)
    _judge('NTXentHard(beta=0, tau_plus=0)', ours, r64, err_ref)
    a, b = z1.to(DEV), z2.to(DEV)
    plain = losses.NTXentFn.apply(a, b, 0.1, 0.0, 1, 0, 257, True).item()
    print(f'NTXent(eps=0) {plain:.7f} NTXentHard(beta=0, tau_plus=0) {ours[0].item():.7f}')
    assert GH.loss_err(plain, r64[0]) <= max(4 * err_ref[0], FLOOR)


@pytest.mark.parametrize('key,norm', [('infonce_hard', False), ('infonce_hard', True), ('ntxent_hard', False), ('infonce', False),
                                      ('extra', False)], ids=lambda v: str(v))
def test_the_other_normalisation_setting(key, norm):
    """InfoNCEHard without normalisation (its default) and with it; the other modes without it, on inputs scaled by D^-1/2"""
    z1, z2, kw, r64, err_ref = _case(key, 67, 13, 3 if key == 'extra' else 0, norm, tau=0.1)
    _judge(f'{key} norm={norm}', _ours(key, z1, z2, **kw), r64, err_ref)


@pytest.mark.parametrize('key', ['infonce', 'extra'])
def test_regularisers_see_the_first_batch_of_rows(key):
    """variance, covariance and uniformity terms of reference commons/losses.py:946-964 on z1 and z2[:B], in fp64"""
    B, D, U = 33, 24, (10 if key == 'extra' else 0)
    z1, z2, kw, _, _ = _case(key, B, D, U, tau=0.1, **({'extra_negatives_weight': 1} if U else {}))
    z1, z2 = 0.2 * z1, 0.2 * z2          # squared distances near 2: the uniformity term's exp(-2 d^2) stays inside fp32
    base = _ours(key, z1, z2, **kw)
    got = _ours(key, z1, z2, variance_reg=0.5, covariance_reg=0.25, uniformity_reg=0.125, **kw)
    a, b = z1.double(), z2[:B].double()
    std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()

    def cov(v):
        c = v - v.mean(dim=0)
        c = c.T @ c / (B - 1)
        return (c - torch.diag(torch.diagonal(c))).pow(2).sum() / D
    uni = lambda v: torch.pdist(v, p=2).pow(2).mul(-2).exp().mean().log()
    want = 0.5 * (std(a) + std(b)) + 0.25 * (cov(a) + cov(b)) + 0.125 * 0.5 * (uni(a) + uni(b))
    print(f'{key}: regularisers {want.item():.7f} kernel {(got[0] - base[0]).item():.7f}')
    assert abs((got[0] - base[0]).item() - want.item()) < 1e-5 * max(1.0, abs(want.item()))
    assert (got[1] - base[1]).abs().max() > 0 and (got[2][:B] - base[2][:B]).abs().max() > 0
    if U:
        assert torch.equal(got[2][B:], base[2][B:])          # the extras are outside the regularisers


def test_shuffled_is_the_ntxent_path_on_the_permuted_rows():
    z = load('hardneg.npz')
    p = GH.case_prefix('shuffled', (67, 13), 'tau0.1')
    z1, z2, kw, _ = case_setup(z, 'shuffled', (67, 13), 'tau0.1')
    seed, perm = int(z[p + 'seed']), torch.from_numpy(z[p + 'perm'])
    ours = _ours('shuffled', z1, z2, seed=seed, **kw)
    a = z1.to(DEV).requires_grad_(True)
    b = z2[perm].to(DEV).requires_grad_(True)
    plain = losses.NTXentFn.apply(a, b, 0.1, 0.0, 1, 0, 67, True)
    plain.backward()
    assert torch.equal(ours[0], plain.detach().cpu()) and torch.equal(ours[1], a.grad.cpu())
    back = torch.empty_like(ours[2])
    back[perm] = b.grad.cpu()
    assert torch.equal(ours[2], back)
    again = _ours('shuffled', z1, z2, seed=seed + 1, **kw)
    assert not torch.equal(again[0], ours[0])               # another seed, another permutation


def test_individual_kernels_through_the_ops_wrappers():
    """norms, row pass and backward launch called one by one: the row statistics against fp64, and the gradients composed from dsim and
    the norm-path coefficients against fp64 by the rule.  Bound of the statistics: every P = exp(t) carries the rounding of s' (a few
    ulp) times |t| <= 1 / tau, and P^(1 + beta) that times 1 + beta; the fp64 sums of positive terms keep the relative error:
    8 * 2^-23 * (2 + (1 + beta) / tau) = 1.6e-5 at tau = 0.1, beta = 0.5."""
    z1, z2, kw, r64, err_ref = _case('ntxent_hard', 67, 13, tau=0.1, beta=0.5)
    a, b = z1.to(DEV), z2.to(DEV)
    mode = ops.HARDNEG_MODES['ntxent_hard']
    n1, n2, xdot, xn = ops.hardneg_norms(a, b)
    assert xdot is None and xn is None
    sim = ops.gemm(a, b, trans_b=True)
    stats, coef, loss = ops.hardneg_fwd(mode, sim, n1, n2, 0, 0.1, tau_plus=0.1, beta=0.5, loss_scale=1.0 / 67)
    t = (z1.double() @ z2.double().T) / (z1.double().norm(dim=1)[:, None] * z2.double().norm(dim=1)[None, :]) / 0.1
    off = ~torch.eye(67, dtype=torch.bool)
    want = torch.stack([torch.exp(torch.diagonal(t)), (torch.exp(t) * off).sum(1), (torch.exp(0.5 * t) * off).sum(1),
                        (torch.exp(1.5 * t) * off).sum(1)], dim=1)
    rel = ((stats.cpu()[:, :4] - want).abs() / want).max().item()
    bound = 8 * 2.0 ** -23 * (2 + 1.5 / 0.1)
    print(f'row statistics: relative error {rel:.3e} bound {bound:.3e}')
    assert rel <= bound
    assert abs(stats[:, 4].sum().item() / 67 - loss.item()) <= 1e-6 * max(1.0, abs(loss.item()))
    dsim, ca, cb, dz1, dz2, dx = ops.hardneg_bwd(mode, sim, n1, n2, coef, a, b, 0, 0.1, beta=0.5, grad_scale=1.0 / 67)
    assert dx is None
    assert torch.equal(dz1, ca[:, None] * a) and torch.equal(dz2, cb[:, None] * b)
    full = (loss.cpu().reshape(()), (dz1.double() + dsim.double() @ b.double()).cpu(), (dz2.double() + dsim.double().T @ a.double()).cpu())
    _judge('composed from the wrappers', full, r64, err_ref)


@pytest.mark.parametrize('key,shape', [(k, (257, 40)) for k in ['infonce', 'ntxent_hard', 'infonce_hard']] + [('extra', (33, 24))],
                         ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_two_runs_are_bit_identical(key, shape):
    z1, z2, kw, _, _ = _case(key, *shape, **({'U': 10, 'extra_negatives_weight': 50} if key == 'extra' else {}), tau=0.1)
    a, b = _ours(key, z1, z2, **kw), _ours(key, z1, z2, **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('key', sorted(NAMES))
def test_step_does_not_synchronise(key):
    """forward and backward under torch's sync debug mode, the upstream gradient a device scalar; its factor 2 reaches the gradients"""
    U = 3 if key == 'extra' else 0
    z1, z2, kw, _, _ = _case('extra' if U else 'infonce', 67, 13, U, tau=0.1)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = getattr(amd, NAMES[key])(tau=0.1, norm=True)

    def step():
        loss = loss_fn(a, b)
        (2.0 * loss).backward()
        return loss
    torch.manual_seed(5)
    step()                                   # allocations, workspaces, the library's first load
    once = (a.grad.clone(), b.grad.clone())
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.manual_seed(5)
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert torch.equal(a.grad, once[0]) and torch.equal(b.grad, once[1])
    torch.manual_seed(5)
    single = _ours(key, z1, z2, seed=5, tau=0.1, norm=True)
    assert torch.allclose(a.grad.cpu(), 2.0 * single[1], rtol=1e-6, atol=0) and torch.allclose(b.grad.cpu(), 2.0 * single[2], rtol=1e-6, atol=0)
