"""KLDivergenceMultiplePositives and the metrics of its config on the MI355X (csrc/klmp.hip): accuracy against the reference's fp64 results
with the reference's own fp32 error as the yardstick, shapes at the edges of the stride loop, the workgroup sum and the conformer loop,
the variance regulariser, determinism, the absence of host synchronisation, coincident conformers, the end-to-end fixture, memory, the
data-parallel share, and the four metrics.

The rule of every accuracy check (that of tests/test_gpu_separate2d.py): err = error against fp64, err_ref = error of the reference
(fixture) or of the same formula in torch fp32 (shapes computed here) against fp64 on the same inputs; err <= max(4 err_ref, 1e-6).  The
factor covers another summation order and the device exp / log; the floor covers cases where fp32 torch happens to be exact.  Errors are
max-norm: a gradient's relative to its largest entry, the loss's relative to max(|loss|, 1).

Every check prints err_ref and the kernel's error before it asserts; the table of DESIGN.md ('KLDivergenceMultiplePositives') holds
err_ref per fixture case, the kernel columns there are still open."""
import functools
import importlib

import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz

import gen_golden_kl as GK
from test_kl_multiple_positives_cpu import CASE_IDS, CASES, restated

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR = 1e-6


def _loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def _grad_err(got, ref):
    a, b = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _ours(z1, z2, loss_fn=None, **kw):
    a = torch.as_tensor(z1).to(DEV).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(DEV).clone().requires_grad_(True)
    loss = (loss_fn or amd.KLDivergenceMultiplePositives(**kw))(a, b)
    assert loss.dim() == 0
    loss.backward()
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


@pytest.mark.parametrize('norm', [False, True], ids=['raw', 'norm'])
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_matches_reference_fixture(case, norm):
    """loss, dz1 and dz2 of every fixture case against the fixture's fp64 values; err_ref = the fixture's fp32 values against them"""
    (B, C, D), jitter = case
    z = load('kl_multiple_positives.npz')
    tag = GK.case_tag(B, C, D, jitter)
    p = f'loss/{tag}/n{int(norm)}/'
    ours = _ours(z[f'loss/{tag}/z1'], z[f'loss/{tag}/z2'], norm=norm)
    ref32 = (z[p + 'loss32'], z[p + 'dz1_32'], z[p + 'dz2_32'])
    ref64 = (z[p + 'loss64'], z[p + 'dz1_64'], z[p + 'dz2_64'])
    _judge(p, ours, ref32, ref64)


def _inputs(B, C, D):
    g = torch.Generator().manual_seed(100 * B + 10 * C + D)
    return torch.randn(B, 2 * D, generator=g), torch.randn(B * C, D, generator=g)


@functools.lru_cache(maxsize=None)
def _references(B, C, D):
    """(fp32, fp64) of the restatement of tests/test_kl_multiple_positives_cpu.py, computed once per shape"""
    z1, z2 = _inputs(B, C, D)
    r32, r64 = restated(z1, z2, torch.float32), restated(z1, z2, torch.float64)
    assert torch.isfinite(r64[0]) and torch.isfinite(r64[1]).all() and torch.isfinite(r64[2]).all()
    return r32, r64


EDGES = [(3, 2, 1), (2, 3, 255), (2, 3, 257), (2, 3, 300), (65, 2, 64), (2, 9, 33), (1, 2, 256)]


@pytest.mark.parametrize('shape', EDGES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_edges_match_fp64(shape):
    """one feature; D below, one past and well past one 256-thread pass of the stride loop; 65 molecules (the one-workgroup sum of kl_b
    crosses a wave boundary); nine conformers (more than the sep2d kernels take); a single molecule"""
    B, C, D = shape
    r32, r64 = _references(B, C, D)
    _judge(f'kl {shape}', _ours(*_inputs(B, C, D)), r32, r64)


def test_variance_regulariser_on_the_views():
    B, C, D = 5, 3, 24
    z1, z2 = _inputs(B, C, D)
    base = _ours(z1, z2)
    got = _ours(z1, z2, variance_reg=0.5)
    a, b = z1.double().reshape(B, 2, D), z2.double().reshape(B, C, D)
    std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()
    print(f'variance_reg: added {(got[0] - base[0]).item():.7f} reference {0.5 * (std(a) + std(b)).item():.7f}')
    assert abs((got[0] - base[0]).item() - 0.5 * (std(a) + std(b)).item()) < 1e-5
    assert (got[1] - base[1]).abs().max() > 0
    with pytest.raises(NotImplementedError, match='covariance_reg'):
        _ours(z1, z2, covariance_reg=0.1)
    with pytest.raises(NotImplementedError, match='uniformity_reg'):
        _ours(z1, z2, uniformity_reg=0.1)


def test_two_runs_are_bit_identical():
    z1, z2 = _inputs(33, 5, 256)
    a, b = _ours(z1, z2), _ours(z1, z2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_step_does_not_synchronise():
    z1, z2 = _inputs(33, 5, 256)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = amd.KLDivergenceMultiplePositives(tau=0.1)

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
    ref = _ours(z1, z2)
    assert torch.equal(a.grad.cpu(), 2.0 * ref[1]) and torch.equal(b.grad.cpu(), 2.0 * ref[2])      # the upstream 2 is a power of two


def test_coincident_conformers_stay_finite():
    """every conformer of a molecule identical: v2 = 1e-6, 1 / v2 at its largest.  No accuracy claim."""
    B, C, D = 4, 3, 40
    z1, z2 = _inputs(B, C, D)
    z2 = z2.reshape(B, C, D)[:, :1].expand(B, C, D).reshape(B * C, D).contiguous()
    for norm in (False, True):
        loss, g1, g2 = _ours(z1, z2, norm=norm)
        print(f'coincident conformers norm={norm}: loss {loss.item():.4f} |dz2|max {g2.abs().max().item():.3e}')
        assert torch.isfinite(loss) and torch.isfinite(g1).all() and torch.isfinite(g2).all()


def _e2e_batch(z):
    mols = mols_from_npz(z, 'e2e/mol')
    coords, off, items = z['e2e/conf_coords'], 0, []
    for m in mols:
        cs = []
        for _ in range(GK.E2E_CONF):
            cs.append(amd.complete_graph(m, coords[off:off + m.n_atoms]))
            off += m.n_atoms
        items.append((amd.bond_graph(m), amd.batch(cs)))
    (g2,), (g3,) = amd.conformer_collate(items)
    return g2.to(DEV), g3.to(DEV)


def test_end_to_end_matches_reference_fixture():
    """4 molecules x 2 conformers through PNA and Net3D against the reference's fp64 results on the same fp32 weights and inputs: loss and
    embeddings at 1e-4, parameter gradients by helpers.grads_close at the 5e-4 of the other small-model fixtures (the generator asserts
    that the reference's own fp32 gradients stay within a quarter of that bound on these conformers)"""
    z = load('kl_multiple_positives.npz')
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **GK.PNA_KW)
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **GK.NET3D_KW)
    pna.load_state_dict(sd_from_npz(z, 'e2e/pna_sd'), strict=True)
    net.load_state_dict(sd_from_npz(z, 'e2e/net3d_sd'), strict=True)
    pna.to(DEV).train(), net.to(DEV).train()
    g2, g3 = _e2e_batch(z)
    z1, z2 = pna(g2), net(g3)
    loss = amd.KLDivergenceMultiplePositives()(z1, z2)
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


def test_memory_stays_far_below_one_covariance_tensor():
    """(256, 3, 256): ONE [B, D, D] fp32 tensor of the reference's MultivariateNormal form is 64 MiB and it builds two; forward + backward
    here allocate the outputs (1.25 MiB) and [B, 3] doubles"""
    B, C, D = 256, 3, 256
    z1, z2 = _inputs(B, C, D)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = amd.KLDivergenceMultiplePositives()
    loss_fn(a, b).backward()          # the library's first load
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = loss_fn(a, b)
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f'kl (256, 3, 256): peak growth {growth / 2 ** 20:.2f} MiB')
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert growth < 8 * 2 ** 20


def test_data_parallel_share(monkeypatch):
    """rank 0 of 2 with shard counts [B, 3]: this rank's share is the single-process loss times B / (B + 3), the gradients alike"""
    B, C, D = 5, 3, 24
    z1, z2 = _inputs(B, C, D)
    single = _ours(z1, z2)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda g=None: 2)
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda g=None: 0)
    loss_fn = amd.KLDivergenceMultiplePositives().attach_group(object()).set_shard_counts([B, 3])
    share = _ours(z1, z2, loss_fn)
    f = B / (B + 3)
    for name, s, one in zip(('loss', 'dz1', 'dz2'), share, single):
        err = (s.double() - f * one.double()).abs().max().item() / (f * one.double().abs().max().item())
        print(f'data parallel {name}: relative difference from B / (B + 3) of the single-process value {err:.3e}')
        assert err < 1e-6
    for counts in ([B + 1, 3], [B, 3, 1], [3, B]):
        loss_fn.set_shard_counts(counts)
        with pytest.raises(ValueError, match='shard counts'):
            _ours(z1, z2, loss_fn)


def test_metrics_of_the_config():
    """z1 [5, 48], z2 [15, 24] of the fixture: the four metrics within 1e-5 relative of the reference's, the conformer pair from one
    device-to-host copy, and the pairwise metrics still refused on these shapes"""
    M = importlib.import_module('3dinfomax_amd.metrics')
    z = load('kl_multiple_positives.npz')
    tag = GK.case_tag(5, 3, 24)
    z1, z2 = torch.from_numpy(z[f'loss/{tag}/z1']).to(DEV), torch.from_numpy(z[f'loss/{tag}/z2']).to(DEV)
    assert z1.shape == (5, 48) and z2.shape == (15, 24)
    p = f'metrics/{tag}/'
    checks = [('batch_variance', amd.BatchVariance()), ('dimension_covariance', amd.DimensionCovariance())]
    for n in (0, 1):
        checks += [(f'conformer_3d_variance_n{n}', amd.Conformer3DVariance(normalize=bool(n))),
                   (f'conformer_2d_variance_n{n}', amd.Conformer2DVariance(normalize=bool(n)))]
    bad = []
    for name, m in checks:
        v = m(z1, z2)
        assert v.dim() == 0 and not v.is_cuda
        ref = float(z[p + name])
        print(f'{name}: {v.item():.9g} reference {ref:.9g} relative {abs(v.item() - ref) / abs(ref):.2e}')
        if not abs(v.item() - ref) <= 1e-5 * abs(ref):
            bad.append(name)
    assert not bad, bad
    # the pair shares one pass: the second metric finds the first one's values, and runs without touching the device
    a = amd.Conformer3DVariance()(z1, z2).item()
    vals = M._conformer_cache['values']
    torch.cuda.set_sync_debug_mode('error')
    try:
        b = amd.Conformer2DVariance()(z1, z2).item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert M._conformer_cache['values'] is vals and a == pytest.approx(vals['conformer_3d_variance'])
    assert b == pytest.approx(vals['conformer_2d_variance'])
    amd.BatchVariance()(z1, z2)
    vals = M._per_tensor_cache['values']
    amd.DimensionCovariance()(z1, z2)
    assert M._per_tensor_cache['values'] is vals
    old = M._conformer_cache['values']
    z1.mul_(0.5)                                            # an in-place update bumps the version -> recomputed
    c = amd.Conformer2DVariance()(z1, z2).item()
    assert M._conformer_cache['values'] is not old and c != b
    with pytest.raises(ValueError, match='incompatible embedding shapes'):
        amd.PositiveSimilarity()(z1, z2)
