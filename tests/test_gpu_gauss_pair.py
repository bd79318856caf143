"""NTXentLikelihoodLoss, JSDMultiplePositivesLoss, PositiveProb and NegativeProb on the MI355X (csrc/gausspair.hip): accuracy against the
reference's fp64 results with the reference's own fp32 error as the yardstick, the metrics, the regularisers, determinism, the absence of
host synchronisation, identical conformers, the end-to-end fixture and the refusals.

The rule of every accuracy check (that of tests/test_gpu_separate2d.py): err = error against fp64, err_ref = error of the reference's fp32
results (fixture) against its fp64 ones on the same inputs; err <= max(4 err_ref, 1e-6).  The factor covers another summation order and
the device exp / log; the floor covers cases where fp32 torch happens to be exact.  Errors are max-norm: a gradient's relative to its
largest entry, the loss's relative to max(|loss|, 1).  Where the reference's fp32 result is not finite ('aligned4' at tau = 0.1: its `row
sum - positive` rounds to zero) err_ref is the error of the fp32 restatement of tests/test_gauss_pair_cpu.py, which sums the negatives
directly and takes the row maximum out of the exponent; the kernel's loss has to be finite there.  The metrics have fp64 fixture values
only: err_ref is the fp32 restatement's error.

The shapes of the fixture are the edges of the kernels: two molecules (fewer than the four waves that split a backward sum), 65 (more
than one 8-wide tile and one 64-wide one), one conformer, nine (three groups of the dz2 pass, the last with one), D = 7 and 8 (one
partial 64-feature chunk), 256 and 300 (more than one pass of the 256-thread stride loop, a partial last chunk).

Every check prints err_ref and the kernel's error before it asserts; the table of DESIGN.md ('Gaussian pair losses') holds them."""
import functools
import importlib

import numpy as np
import pytest
import torch

from helpers import amd, grads_close, mols_from_npz, rel_err, sd_from_npz

import gen_golden_gauss as GG
from test_gauss_pair_cpu import JSD_IDS, JSD_SETTINGS, LIK_IDS, LIK_SETTINGS, fixture, jsd_loss, lik_loss, prob_metrics, restated

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR = 1e-6


def _loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def _grad_err(got, ref):
    a, b = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _ours(loss_fn, z1, z2, scale=None):
    a = torch.as_tensor(z1).to(DEV).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(DEV).clone().requires_grad_(True)
    loss = loss_fn(a, b)
    assert loss.dim() == 0
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _judge(what, ours, ref32, ref64):
    """print every figure, then assert the rule on loss, dz1, dz2"""
    rows = [('loss', _loss_err(ours[0], ref64[0]), _loss_err(ref32[0], ref64[0]))]
    for k, name in ((1, 'dz1'), (2, 'dz2')):
        rows.append((name, _grad_err(ours[k], ref64[k]), _grad_err(ref32[k], ref64[k])))
    for name, e, e_ref in rows:
        print(f'{what} {name}: err_ref {e_ref:.3e} kernel {e:.3e}')
    for o in ours:
        assert torch.isfinite(torch.as_tensor(o)).all()
    bad = [(name, e, e_ref) for name, e, e_ref in rows if not e <= max(4 * e_ref, FLOOR)]
    assert not bad, bad


def _stored(z, p):
    return ((z[p + 'loss32'], z[p + 'dz1_32'], z[p + 'dz2_32']), (z[p + 'loss64'], z[p + 'dz1_64'], z[p + 'dz2_64']))


@pytest.mark.parametrize('setting', LIK_SETTINGS, ids=LIK_IDS)
def test_likelihood_matches_reference_fixture(setting):
    shape, edge, tau = setting
    z = fixture('lik')
    tag = GG.case_tag(shape, edge)
    z1, z2 = z[f'in/{tag}/z1'], z[f'in/{tag}/z2']
    p = f'lik/{tag}/t{tau}/'
    ref32, ref64 = _stored(z, p)
    if not all(np.isfinite(r).all() for r in ref32):
        assert (edge, tau) == ('aligned4', 0.1)
        ref32 = restated(lik_loss, z1, z2, torch.float32, tau=tau)
        assert all(torch.isfinite(r).all() for r in ref32)
    _judge(p, _ours(amd.NTXentLikelihoodLoss(tau=tau), z1, z2), ref32, ref64)


@pytest.mark.parametrize('setting', JSD_SETTINGS, ids=JSD_IDS)
def test_jsd_matches_reference_fixture(setting):
    shape, edge, norm = setting
    z = fixture('jsd')
    tag = GG.case_tag(shape, edge)
    p = f'jsd/{tag}/n{int(norm)}/'
    ref32, ref64 = _stored(z, p)
    _judge(p, _ours(amd.JSDMultiplePositivesLoss(norm=norm), z[f'in/{tag}/z1'], z[f'in/{tag}/z2']), ref32, ref64)


def test_metrics_match_reference_fixture():
    """both metrics on every likelihood case, z2 read conformer major; each value a 0-dim CPU tensor, the pair from one device pass"""
    M = importlib.import_module('3dinfomax_amd.metrics')
    z = fixture('lik')
    bad = []
    for case in GG.LIK_CASES:
        tag = GG.case_tag(*case)
        z1, z2 = torch.from_numpy(z[f'in/{tag}/z1']), torch.from_numpy(z[f'in/{tag}/z2'])
        ref32 = prob_metrics(z1, z2)
        a, b = z1.to(DEV), z2.to(DEV)
        pos = amd.PositiveProb()(a, b)
        vals = M._prob_cache['values']
        torch.cuda.set_sync_debug_mode('error')
        try:
            neg = amd.NegativeProb()(a, b)                  # finds the first one's pass: no device work
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert M._prob_cache['values'] is vals
        for k, (name, got) in enumerate((('positive_prob', pos), ('negative_prob', neg))):
            assert got.dim() == 0 and not got.is_cuda
            ref = float(z[f'metrics/{tag}/{name}'])
            e, e_ref = _loss_err(vals[name], ref), _loss_err(ref32[k], ref)
            print(f'metrics/{tag}/{name}: {vals[name]:.9g} reference {ref:.9g} err_ref {e_ref:.3e} kernel {e:.3e}')
            assert abs(got.item() - vals[name]) <= 1e-7 * abs(vals[name])
            if not e <= max(4 * e_ref, FLOOR):
                bad.append((tag, name, e, e_ref))
    assert not bad, bad
    v = amd.PositiveProb()(torch.zeros(2, 2, device=DEV), torch.zeros(2, 2, device=DEV))          # the trainer's init call
    assert torch.isnan(v) and not v.is_cuda


def _inputs(B, C, D):
    return GG.case_inputs((B, C, D))


def test_regularisers_on_the_views():
    B, C, D = 5, 3, 24
    z1, z2 = _inputs(B, C, D)
    a, b = z1.double().reshape(B, 2, D), z2.double().reshape(B, C, D)
    std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()
    conf = torch.relu(1 - torch.sqrt(b.var(dim=1) + 1e-4)).mean()
    base = _ours(amd.NTXentLikelihoodLoss(tau=0.1), z1, z2)
    got = _ours(amd.NTXentLikelihoodLoss(tau=0.1, variance_reg=0.5, conformer_variance_reg=0.25), z1, z2)
    want = 0.5 * (std(a) + std(b)).item() + 0.25 * conf.item()
    print(f'likelihood regularisers: added {(got[0] - base[0]).item():.7f} reference {want:.7f}')
    assert abs((got[0] - base[0]).item() - want) < 1e-5
    assert (got[1] - base[1]).abs().max() > 0 and (got[2] - base[2]).abs().max() > 0
    base = _ours(amd.JSDMultiplePositivesLoss(norm=False), z1, z2)
    got = _ours(amd.JSDMultiplePositivesLoss(norm=False, variance_reg=0.5), z1, z2)
    print(f'jsd variance_reg: added {(got[0] - base[0]).item():.7f} reference {0.5 * (std(a) + std(b)).item():.7f}')
    assert abs((got[0] - base[0]).item() - 0.5 * (std(a) + std(b)).item()) < 1e-5
    for cls in (amd.NTXentLikelihoodLoss, amd.JSDMultiplePositivesLoss):
        with pytest.raises(NotImplementedError, match='covariance_reg'):
            _ours(cls(covariance_reg=0.1), z1, z2)
        with pytest.raises(NotImplementedError, match='uniformity_reg'):
            _ours(cls(uniformity_reg=0.1), z1, z2)


LOSS_FNS = {'likelihood': lambda: amd.NTXentLikelihoodLoss(tau=0.1), 'jsd': lambda: amd.JSDMultiplePositivesLoss(),
            'jsd_raw': lambda: amd.JSDMultiplePositivesLoss(norm=False)}


@pytest.mark.parametrize('which', sorted(LOSS_FNS))
def test_two_runs_are_bit_identical(which):
    z1, z2 = _inputs(33, 5, 200)
    a, b = _ours(LOSS_FNS[which](), z1, z2), _ours(LOSS_FNS[which](), z1, z2)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)


@pytest.mark.parametrize('which', sorted(LOSS_FNS))
def test_step_does_not_synchronise(which):
    """forward and backward under torch's sync-debug mode; the upstream gradient (a power of two) is multiplied in on the device"""
    z1, z2 = _inputs(9, 3, 70)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = LOSS_FNS[which]()

    def step():
        loss = loss_fn(a, b)
        (2.0 * loss).backward()
        return loss
    step()                                   # allocations, the library's first load
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    ref = _ours(LOSS_FNS[which](), z1, z2)
    assert torch.equal(loss.detach().cpu(), ref[0])
    if which == 'jsd':                        # the gradient passes through the row normalisation's backward: compared at 1e-6
        assert _grad_err(a.grad.cpu(), 2.0 * ref[1]) < 1e-6 and _grad_err(b.grad.cpu(), 2.0 * ref[2]) < 1e-6
    else:
        assert torch.equal(a.grad.cpu(), 2.0 * ref[1]) and torch.equal(b.grad.cpu(), 2.0 * ref[2])


def test_jsd_identical_conformers_stay_finite():
    """every conformer of a molecule identical: v2 = 0, the weights 1e5, prod v2 = 0.  The reference raises here (from MultivariateNormal
    objects whose values it discards); the formula is evaluated.  No accuracy claim."""
    B, C, D = 4, 3, 40
    z1, z2 = _inputs(B, C, D)
    z2 = z2.reshape(B, C, D)[:, :1].expand(B, C, D).reshape(B * C, D).contiguous()
    for norm in (False, True):
        loss, g1, g2 = _ours(amd.JSDMultiplePositivesLoss(norm=norm), z1, z2)
        print(f'identical conformers norm={norm}: loss {loss.item():.4f} |dz1|max {g1.abs().max().item():.3e} |dz2|max '
              f'{g2.abs().max().item():.3e}')
        assert torch.isfinite(loss) and torch.isfinite(g1).all() and torch.isfinite(g2).all()


def _e2e_batch(z):
    mols = mols_from_npz(z, 'e2e/mol')
    coords, off, items = z['e2e/conf_coords'], 0, []
    for m in mols:
        cs = []
        for _ in range(GG.E2E_CONF):
            cs.append(amd.complete_graph(m, coords[off:off + m.n_atoms]))
            off += m.n_atoms
        items.append((amd.bond_graph(m), amd.batch(cs)))
    (g2,), (g3,) = amd.conformer_collate(items)
    return g2.to(DEV), g3.to(DEV)


def test_end_to_end_matches_reference_fixture():
    """4 molecules x 2 conformers through PNA and Net3D against the reference's fp64 results on the same fp32 weights and inputs: loss and
    embeddings at 1e-4, parameter gradients by helpers.grads_close at the 5e-4 of the other small-model fixtures (the generator asserts
    that the reference's own fp32 gradients stay within a quarter of that bound)"""
    z = fixture('e2e')
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **GG.PNA_KW)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **GG.NET3D_KW)
    pna.load_state_dict(sd_from_npz(z, 'e2e/pna_sd'), strict=True)
    net.load_state_dict(sd_from_npz(z, 'e2e/net3d_sd'), strict=True)
    pna.to(DEV).train(), net.to(DEV).train()
    g2, g3 = _e2e_batch(z)
    z1, z2 = pna(g2), net(g3)
    loss = amd.NTXentLikelihoodLoss(tau=GG.E2E_TAU, conformer_variance_reg=GG.E2E_CONF_REG)(z1, z2)
    loss.backward()
    print(f'e2e loss {loss.item():.7f} reference {float(z["e2e/loss"]):.7f} z1 {rel_err(z1.detach().cpu(), z["e2e/z1"]):.2e} '
          f'z2 {rel_err(z2.detach().cpu(), z["e2e/z2"]):.2e}')
    assert rel_err(z1.detach().cpu(), z['e2e/z1']) < 1e-4 and rel_err(z2.detach().cpu(), z['e2e/z2']) < 1e-4
    assert abs(loss.item() - float(z['e2e/loss'])) < 1e-4 * abs(float(z['e2e/loss']))
    for model, tag in ((pna, 'pna_grad'), (net, 'net3d_grad')):
        ref = sd_from_npz(z, 'e2e/' + tag)
        got = {k: q.grad.detach().cpu() for k, q in model.named_parameters() if q.grad is not None}
        assert set(got) == set(ref)
        grads_close(got, ref, 5e-4, what=f'e2e/{tag}: ')


def test_refusals_fire_on_device_tensors_before_any_launch(monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')
    zeros = functools.partial(torch.zeros, device=DEV)
    torch.cuda.synchronize()

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)
    for cls in (amd.NTXentLikelihoodLoss, amd.JSDMultiplePositivesLoss):
        loss = cls(tau=0.1)
        with pytest.raises(ValueError, match='columns'):
            loss(zeros(4, 17), zeros(12, 8))
        with pytest.raises(ValueError, match='multiple'):
            loss(zeros(4, 16), zeros(13, 8))
        with pytest.raises(ValueError, match='no negatives'):
            loss(zeros(1, 16), zeros(3, 8))
        with pytest.raises(NotImplementedError, match='fp32'):
            loss(zeros(4, 16, dtype=torch.float64), zeros(12, 8, dtype=torch.float64))
        with pytest.raises(NotImplementedError, match='covariance_reg'):
            cls(covariance_reg=0.1)(zeros(4, 16), zeros(12, 8))
        with pytest.raises(NotImplementedError, match='uniformity_reg'):
            cls(uniformity_reg=0.1)(zeros(4, 16), zeros(12, 8))
    with pytest.raises(ValueError, match='at least two'):
        amd.JSDMultiplePositivesLoss()(zeros(4, 16), zeros(4, 8))
    with pytest.raises(ValueError, match='at least two'):
        amd.NTXentLikelihoodLoss(conformer_variance_reg=0.05)(zeros(4, 16), zeros(4, 8))
    group = object()
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2 if g is group else 1)
    for cls in (amd.NTXentLikelihoodLoss, amd.JSDMultiplePositivesLoss):
        with pytest.raises(NotImplementedError, match='process group'):
            cls().attach_group(group)(zeros(4, 16), zeros(12, 8))
