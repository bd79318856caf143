"""NTXentMinimumMatching / NTXentMaximumSimilarity / NTXentMultiplePositivesV2 / NTXentMultiplePositivesV3 on the MI355X
(csrc/confmatch.hip): accuracy against the reference's fp64 results with the reference's own fp32 error as the yardstick, shapes at the
kernels' wave, workgroup and feature-chunk edges, the path without normalisation, the regularisers, determinism, V2's unused columns, the
end-to-end fixture, memory, and the absence of host synchronisation.

The rule of every accuracy check (that of tests/test_gpu_separate2d.py): err = max-norm error against fp64, a gradient's relative to its
largest entry, the loss's relative to max(|loss|, 1); err_ref = the error of the reference's fp32 (fixture) or of the same formula in
torch fp32 on the CPU (shapes computed here) against fp64 on the same inputs; err <= max(4 err_ref, 1e-6).  Every check prints err_ref
and the kernel's error before it asserts.

The inputs of the matching losses meet the selection condition of the fixture (tests/golden/gen_golden_confmatch.py): every minimum,
maximum and positive is decided by more than 1e-4 in fp64, so the fp32 kernels, fp32 torch and fp64 torch select the same entries."""
import functools
import importlib

import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz

import gen_golden_confmatch as GC
import gen_golden_separate2d as GS
from test_confmatch_cpu import CASES, CASE_IDS, MATCHING, NAMES, PER_CONFORMER, gapped_inputs, restated

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
DEV = torch.device('cuda:0')
FLOOR = 1e-6
ALL = sorted(NAMES)


def _loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def _grad_err(got, ref):
    a, b = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _ours(key, z1, z2, tau=GC.TAU, **kw):
    a = torch.as_tensor(z1).to(DEV).clone().requires_grad_(True)
    b = torch.as_tensor(z2).to(DEV).clone().requires_grad_(True)
    loss = getattr(amd, NAMES[key])(tau=tau, **kw)(a, b)
    loss.backward()
    return loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()


def _judge(what, ours, ref32, ref64):
    """print every figure, then assert the rule on loss, dz1, dz2"""
    rows = [('loss', _loss_err(ours[0], ref64[0]), _loss_err(ref32[0], ref64[0]))]
    for k, name in ((1, 'dz1'), (2, 'dz2')):
        rows.append((name, _grad_err(ours[k], ref64[k]), _grad_err(ref32[k], ref64[k])))
    for name, e, e_ref in rows:
        print(f'{what} {name}: err_ref {e_ref:.3e} kernel {e:.3e}')
    for o, r in zip(ours, ref64):
        assert torch.isfinite(torch.as_tensor(o)).all() and tuple(torch.as_tensor(o).shape) == tuple(torch.as_tensor(r).shape)
    bad = [(name, e, e_ref) for name, e, e_ref in rows if not e <= max(4 * e_ref, FLOOR)]
    assert not bad, bad


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('key', ALL)
def test_matches_reference_fixture(key, case):
    """loss, dz1 and dz2 of every fixture case against the fixture's fp64 values; err_ref = the fixture's fp32 values against them"""
    (B, C, D), near = case
    z = load('confmatch.npz')
    p = f'{key}/{GC.case_tag(B, C, D, near)}/'
    ours = _ours(key, z[p + 'z1'], z[p + 'z2'])
    ref32 = (z[p + 'loss32'], z[p + 'dz1_32'], z[p + 'dz2_32'])
    ref64 = (z[p + 'loss64'], z[p + 'dz1_64'], z[p + 'dz2_64'])
    _judge(p, ours, ref32, ref64)


@functools.lru_cache(maxsize=None)
def _case(key, B, C, D, scale=1.0, norm=True):
    """(z1, z2, fp32 reference, fp64 reference) of a shape outside the fixture, computed once and left unchanged"""
    if key in GC.MATCHING:
        z1, z2, seed, gap = gapped_inputs(B, C, D, scale, norm)
        print(f'matching inputs {(B, C, D)}: seed {seed} gap {gap:.2e}')
    else:
        z1, z2 = GC.per_conformer_inputs(B, C, D)
        z1, z2 = scale * z1, scale * z2
    r32 = restated(key, z1, z2, GC.TAU, torch.float32, norm=norm)
    r64 = restated(key, z1, z2, GC.TAU, torch.float64, norm=norm)
    assert torch.isfinite(r64[0]) and torch.isfinite(r64[1]).all() and torch.isfinite(r64[2]).all()
    return z1, z2, r32, r64


@pytest.mark.parametrize('shape', [(9, 8, 24), (6, 8, 260), (13, 3, 7), (66, 1, 24), (34, 2, 40)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key', MATCHING)
def test_matching_kernel_boundaries_match_fp64(key, shape):
    """(9, 8, 24): all 64 lanes of the pair wave, B no multiple of the four waves of a workgroup; (6, 8, 260): a second feature chunk, no
    multiple of 64; (13, 3, 7): nine lanes, odd everything; (66, 1, 24): one lane, where a positive's entry can be a negative's too, and more
    pairs per row than a wave; (34, 2, 40)"""
    z1, z2, r32, r64 = _case(key, *shape)
    _judge(f'{key} {shape}', _ours(key, z1, z2), r32, r64)


@pytest.mark.parametrize('shape', [(65, 3, 256), (33, 10, 256), (2, 1, 3), (3, 16, 7)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key', PER_CONFORMER)
def test_per_conformer_kernel_boundaries_match_fp64(key, shape):
    """B C = 195 (below one pass of the row kernel, no multiple of the column pass's 16) and 330 (above it, the configs' C = 10: a stride
    of 250 columns), the smallest batch with one conformer, and C = 16 with three molecules"""
    z1, z2, r32, r64 = _case(key, *shape)
    _judge(f'{key} {shape}', _ours(key, z1, z2), r32, r64)


@pytest.mark.parametrize('key', ALL)
def test_without_normalisation(key):
    z1, z2, r32, r64 = _case(key, 5, 3, 24, 0.2, False)
    _judge(f'{key} norm=False', _ours(key, z1, z2, norm=False), r32, r64)


@pytest.mark.parametrize('key', ALL)
def test_variance_regulariser_on_the_views(key):
    B, C, D = 5, 3, 24
    z1, z2, _, _ = _case(key, B, C, D)
    base = _ours(key, z1, z2)
    got = _ours(key, z1, z2, variance_reg=0.5)
    a = z1.double().reshape(B, C, D) if key in GC.MATCHING else z1.double()
    b = z2.double().reshape(B, C, D)
    std = lambda v: torch.relu(1 - torch.sqrt(v.var(dim=0) + 1e-4)).mean()
    assert abs((got[0] - base[0]).item() - 0.5 * (std(a) + std(b)).item()) < 1e-5
    assert (got[1] - base[1]).abs().max() > 0
    with pytest.raises(NotImplementedError, match='covariance_reg'):
        _ours(key, z1, z2, covariance_reg=0.1)
    with pytest.raises(NotImplementedError, match='uniformity_reg'):
        _ours(key, z1, z2, uniformity_reg=0.1)


@pytest.mark.parametrize('key,shape', [(k, (9, 8, 24)) for k in ALL] + [(k, (33, 10, 256)) for k in PER_CONFORMER],
                         ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_two_runs_are_bit_identical(key, shape):
    z1, z2, _, _ = _case(key, *shape)
    a, b = _ours(key, z1, z2), _ours(key, z1, z2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_v2_leaves_the_other_molecules_later_conformers_alone():
    """dS is exactly zero in the columns (j, u >= 1) of the other molecules; through dz2: those rows get their gradient from their own
    molecule's positive alone, compared with fp64"""
    B, C, D = 5, 3, 24
    z1, z2, _, _ = _case('v2', B, C, D)
    a, b = z1.to(DEV), z2.to(DEV)
    n1, n2 = ops.row_norms(a), ops.row_norms(b)
    sim = ops.gemm(a, b, trans_b=True)
    den, pos, _ = ops.per_conf_fwd(sim, n1, n2, B, C, ops.PER_CONF_MODES['v2'], GC.TAU)
    dsim, _, _ = ops.per_conf_bwd(sim, n1, n2, den, pos, B, C, ops.PER_CONF_MODES['v2'], GC.TAU, torch.ones(1, device=DEV))
    dsim = dsim.cpu().reshape(B, B, C)
    other = ~torch.eye(B, dtype=torch.bool)
    assert torch.count_nonzero(dsim[other][:, 1:]) == 0
    assert torch.count_nonzero(dsim[other][:, 0]) == other.sum() and torch.count_nonzero(dsim[~other]) == B * C

    def positives_only(dtype):
        x, y = z1.to(dtype), z2.to(dtype).clone().requires_grad_(True)
        yv = y.reshape(B, C, D)
        s = torch.einsum('ik,iuk->iu', x, yv) / (x.norm(dim=1)[:, None] * yv.norm(dim=2))
        g, = torch.autograd.grad(-torch.log(torch.exp(s / GC.TAU).sum(dim=1)).mean(), y)
        return g.reshape(B, C, D)[:, 1:]
    ref64, ref32 = positives_only(torch.float64), positives_only(torch.float32)
    ours = _ours('v2', z1, z2)[2].reshape(B, C, D)[:, 1:]
    full = restated('v2', z1, z2, GC.TAU)[2].reshape(B, C, D)[:, 1:]
    assert (full - ref64).abs().max() < 1e-12          # the statement itself, in fp64
    e, e_ref = _grad_err(ours, ref64), _grad_err(ref32, ref64)
    print(f'v2 rows (j, u >= 1) of dz2: err_ref {e_ref:.3e} kernel {e:.3e}')
    assert e <= max(4 * e_ref, FLOOR)


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


@pytest.mark.parametrize('key', sorted(GC.E2E))
def test_end_to_end_matches_reference_fixture(key):
    """4 molecules x 2 conformers through PNA and Net3D: loss and embeddings at 1e-4, parameter gradients by helpers.grads_close at the
    5e-4 of the other small-model fixtures"""
    z = load('confmatch.npz')
    p = f'e2e/{key}/'
    pna = amd.PNA(avg_d=1.0, device='cuda:0', **GC.E2E[key])
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **GS.NET3D_KW)
    pna.load_state_dict(sd_from_npz(z, p + 'pna_sd'), strict=True)
    net.load_state_dict(sd_from_npz(z, p + 'net3d_sd'), strict=True)
    pna.to(DEV).train(), net.to(DEV).train()
    g2, g3 = _e2e_batch(z)
    z1, z2 = pna(g2), net(g3)
    loss = getattr(amd, NAMES[key])(tau=GC.TAU)(z1, z2)
    loss.backward()
    print(f'{p} loss {loss.item():.7f} reference {float(z[p + "loss"]):.7f} z1 {rel_err(z1.detach().cpu(), z[p + "z1"]):.2e} '
          f'z2 {rel_err(z2.detach().cpu(), z[p + "z2"]):.2e}')
    assert rel_err(z1.detach().cpu(), z[p + 'z1']) < 1e-4 and rel_err(z2.detach().cpu(), z[p + 'z2']) < 1e-4
    assert abs(loss.item() - float(z[p + 'loss'])) < 1e-4 * abs(float(z[p + 'loss']))
    for model, tag in ((pna, 'pna_grad'), (net, 'net3d_grad')):
        ref = sd_from_npz(z, p + tag)
        got = {k: q.grad.detach().cpu() for k, q in model.named_parameters() if q.grad is not None}
        assert set(got) == set(ref)
        grads_close(got, ref, 5e-4, what=f'{p}{tag}: ')


@pytest.mark.parametrize('key', MATCHING)
def test_matching_memory_stays_below_a_dense_gradient(key):
    """(256, 5, 256), N = 1280: forward + backward may grow the peak allocation by less than 2 N^2 floats = 13.1 MB.  S is 6.55 MB, the
    pair tables about 1 MB, the two gradients 2.6 MB; a dense dL/dS would add another 6.55 MB and cross the cap.  Loss and finiteness
    only: random data of this size cannot meet the selection condition."""
    B, C, D = 256, 5, 256
    g = torch.Generator().manual_seed(1000 * B + 10 * C + D)
    a = torch.randn(B, C * D, generator=g).to(DEV).requires_grad_(True)
    b = torch.randn(B * C, D, generator=g).to(DEV).requires_grad_(True)
    loss_fn = getattr(amd, NAMES[key])(tau=GC.TAU)
    loss_fn(a, b).backward()          # the library's first load, workspaces
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = loss_fn(a, b)
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f'{key} (256, 5, 256): peak growth {growth / 1e6:.2f} MB, loss {loss.item():.6f}')
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert a.grad.abs().max() > 0 and b.grad.abs().max() > 0
    assert growth < 2 * (B * C) ** 2 * 4


@pytest.mark.parametrize('key', ALL)
def test_step_does_not_synchronise(key):
    z1, z2, _, _ = _case(key, 9, 8, 24)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    loss_fn = getattr(amd, NAMES[key])(tau=GC.TAU)

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
