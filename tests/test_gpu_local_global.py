"""Local-global pre-training on the MI355X: NTXentLocalGlobal / NTXentGlobalLocal (csrc/localglobal.hip) against the reference's fp64
run (the fixture cases) and against the fp64 oracle of tests/test_local_global_cpu.py (pinned there to that fixture), and PNALocal
against the reference's outputs and gradients (tests/golden/gen_golden_local_global.py).

Bounds come from the reference, never from the kernels: a fixture case may be 8 x the fp32 reference's own error against its fp64
run away from the fp64 values (8: a different summation order than torch's); an oracle case 8 x the error of an fp32 torch-eager
evaluation of the same formula at the same inputs.  The scalar loss is one rounded fp32 number, so its recorded error is floored at
the rounding unit 2^-24 (gen_golden_local_global.py's docstring).  dzn is compared row by row (row_rel_err): a zero node row carries
a gradient of order 1 / (N tau 1e-10), ten orders of magnitude above the others."""
import importlib
import math

import pytest
import torch

from helpers import amd, grads_close, load, mols_from_npz, rel_err, sd_from_npz

import gen_golden_local_global as GL
from test_local_global_cpu import lg_oracle

pytestmark = pytest.mark.gpu
ops = importlib.import_module('3dinfomax_amd.ops')
DEV = torch.device('cuda:0')
FACTOR = 8
CHUNK = ops.LG_ROW_CHUNK


def _ours(zn, zg, npg, tau, norm=True, upstream=None, swapped=False):
    """-> loss (python float), loss tensor bits, dzn, dzg (CPU) of one forward + backward on the kernels"""
    zn, zg = (torch.as_tensor(t).to(DEV).requires_grad_(True) for t in (zn, zg))
    if swapped:
        loss = amd.NTXentGlobalLocal(tau=tau, norm=norm)(zg, zn, npg)
    else:
        loss = amd.NTXentLocalGlobal(tau=tau, norm=norm)(zn, zg, npg)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if upstream is None else loss * upstream).backward()
    return loss.item(), loss.detach().cpu(), zn.grad.cpu(), zg.grad.cpu()


def _errors(loss, dzn, dzg, loss64, dzn64, dzg64):
    return dict(loss=abs(float(loss) - float(loss64)) / abs(float(loss64)), dzn=GL.row_rel_err(dzn, dzn64), dzg=rel_err(dzg, dzg64))


def _assert_within(what, err, ref_err):
    for q in ('loss', 'dzn', 'dzg'):
        print(f'{what}: {q} err {err[q]:.3e} reference fp32 err {ref_err[q]:.3e} ratio {err[q] / ref_err[q]:.2f} (allowed {FACTOR})')
    for q in ('loss', 'dzn', 'dzg'):
        assert err[q] <= FACTOR * ref_err[q], (what, q, err[q], ref_err[q])


class _Oracle:
    """fp64 oracle and the fp32 eager evaluation's own error, once per case"""
    cache = {}

    @classmethod
    def get(cls, key, zn, zg, npg, tau, norm=True, upstream=1.0):
        if key not in cls.cache:
            l64, dn64, dg64 = lg_oracle(zn, zg, npg, tau, norm=norm, upstream=upstream)
            l32, dn32, dg32 = lg_oracle(zn, zg, npg, tau, norm=norm, upstream=upstream, dtype=torch.float32)
            ref_err = _errors(l32, dn32, dg32, l64, dn64, dg64)
            ref_err['loss'] = max(ref_err['loss'], 2.0 ** -24)
            assert torch.isfinite(l32) and torch.isfinite(dn32).all() and torch.isfinite(dg32).all()
            cls.cache[key] = (l64, dn64, dg64, ref_err)
        return cls.cache[key]


def _check_against_oracle(key, zn, zg, npg, tau, norm=True, upstream=None):
    l64, dn64, dg64, ref_err = _Oracle.get(key, zn, zg, npg, tau, norm, 1.0 if upstream is None else upstream)
    loss, _, dzn, dzg = _ours(zn, zg, npg, tau, norm, upstream)
    assert math.isfinite(loss) and torch.isfinite(dzn).all() and torch.isfinite(dzg).all()
    _assert_within(key, _errors(loss, dzn, dzg, l64, dn64, dg64), ref_err)
    return loss, dzn, dzg


def _inputs(npg, dim, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(sum(npg), dim, generator=gen) * scale, torch.randn(len(npg), dim, generator=gen) * scale


@pytest.mark.parametrize('case', ['b2', 'zero', 'long'])
def test_fixture_cases_match_the_reference_fp64_run(case):
    """cases 1-3: [5, 9] D = 6 with an all-zero ReLU row; [1, 7, 64, 3, 1] with row 3 zero; [70, 70, 70, 1, 129] D = 256"""
    z = load('local_global.npz')
    p, c = f'loss/{case}/', GL.LOSS_CASES[case]
    loss, _, dzn, dzg = _ours(z[p + 'zn'], z[p + 'zg'], z[p + 'nodes_per_graph'].tolist(), c['tau'])
    assert math.isfinite(loss) and torch.isfinite(dzn).all() and torch.isfinite(dzg).all()
    err = _errors(loss, dzn, dzg, z[p + 'loss64'], z[p + 'dzn64'], z[p + 'dzg64'])
    _assert_within(case, err, {q: float(z[p + 'ref_err/' + q]) for q in ('loss', 'dzn', 'dzg')})
    if case != 'long':          # the zero row: a finite gradient of order 1 / eps that matches, no norm-path term
        i = int((torch.from_numpy(z[p + 'zn']).abs().sum(1) == 0).nonzero()[0])
        ref = torch.from_numpy(z[p + 'dzn64'][i])
        print(f'{case}: zero row {i} max |dzn| {float(dzn[i].abs().max()):.4e} reference {float(ref.abs().max()):.4e}')
        assert float(ref.abs().max()) > 1e8 and rel_err(dzn[i], ref) <= FACTOR * float(z[p + 'ref_err/dzn'])


def test_more_graphs_than_a_wave():
    """case 4: B = 67 graphs of 1..9 nodes: two column strides per lane, the second partly empty; D = 33 is no multiple of 4"""
    npg = [(7 * j) % 9 + 1 for j in range(67)]
    assert len(npg) == 67 and set(npg) == set(range(1, 10))
    zn, zg = _inputs(npg, 33, 4)
    _check_against_oracle('b67', zn, zg, npg, 0.2)


def test_empty_graphs_are_negatives_for_every_row():
    """case 5: [4, 0, 6, 0, 3]: the upper bound skips the empty segments; their columns stay in every row's negatives"""
    npg = [4, 0, 6, 0, 3]
    zn, zg = _inputs(npg, 8, 5)
    loss, dzn, dzg = _check_against_oracle('empty', zn, zg, npg, 0.3)
    assert float(dzg[1].abs().max()) > 0 and float(dzg[3].abs().max()) > 0


@pytest.mark.parametrize('n', [2 * CHUNK + 3, 1024 + 5, 2048 + 7], ids=['two-chunks', 'k-slices', 'k-slices-2048'])
def test_row_chunks_and_long_k(n):
    """case 6: N = 2 LG_ROW_CHUNK + 3 over five graphs with a segment across each chunk boundary; and the two row counts from which
    the K = N product H^T zn is cut into slices (1024, 2048: csrc/gemm.hip), which meet in a fixed order through the scratch"""
    bounds = [CHUNK - 56, CHUNK + 44, 2 * CHUNK - 62, 2 * CHUNK - 2, n] if n == 2 * CHUNK + 3 else \
        [CHUNK - 56, 2 * CHUNK + 44, 3 * CHUNK + 32, n - 3, n]
    npg = [b - a for a, b in zip([0] + bounds[:-1], bounds)]
    assert sum(npg) == n and min(npg) > 0
    inside = lambda r: any(a < r < b for a, b in zip([0] + bounds[:-1], bounds))      # noqa: E731
    assert all(inside(k * CHUNK) for k in range(1, n // CHUNK + 1))
    zn, zg = _inputs(npg, 12, 6 + n)
    _check_against_oracle(f'chunks{n}', zn, zg, npg, 0.1)
    a, b = _ours(zn, zg, npg, 0.1), _ours(zn, zg, npg, 0.1)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_aligned_positives_stay_finite():
    """case 7: B = 3, tau = 0.1, every node equal to its own graph's embedding, the other two graphs' embeddings its negation: the
    positive is e^10, the two negatives e^-10, loss = log(2) - 20.  rowsum - pos is 0 in fp32 and gives inf.  One embedding cannot be
    the negation of both others for all three graphs at once, so each graph takes its turn as the one that holds the nodes.  The
    analytic gradient is zero (cosines at their extrema): the gradients are fp32 noise and only have to be finite and small.
    Bound of the value: 8 half-ulps of 20, the size of s'/tau's two terms."""
    base = torch.tensor([1.0, -2.0, 0.5, 3.0, -1.5, 0.25, 2.0, -0.75])
    want = math.log(2.0) - 20.0
    for own, count in enumerate([3, 1, 2]):
        zg = -base.repeat(3, 1)
        zg[own] = base
        zn = base.repeat(count, 1)
        npg = [count if j == own else 0 for j in range(3)]
        l64, _, _ = lg_oracle(zn, zg, npg, 0.1)
        assert abs(float(l64) - want) < 1e-8
        value, _, dzn, dzg = _ours(zn, zg, npg, 0.1)
        print(f'aligned positives, graph {own}: loss {value:.7f} log(2) - 20 = {want:.7f} max |dzn| {float(dzn.abs().max()):.2e}')
        assert math.isfinite(value) and torch.isfinite(dzn).all() and torch.isfinite(dzg).all()
        assert abs(value - want) <= FACTOR * 2.0 ** -24 * 20.0
        assert float(dzn.abs().max()) < 1e-4 and float(dzg.abs().max()) < 1e-4


def test_without_normalisation():
    """case 8: norm=False, small-norm inputs (the plain dot product over tau; no eps, no norm-path term)"""
    npg = [3, 70, 1, 9]
    zn, zg = _inputs(npg, 16, 8, scale=0.3)
    _check_against_oracle('nonorm', zn, zg, npg, 0.5, norm=False)


def test_upstream_scalar_is_applied_on_the_device():
    """case 9: (loss * 3.0).backward()"""
    npg = [5, 2, 11]
    zn, zg = _inputs(npg, 10, 9)
    _, dzn3, dzg3 = _check_against_oracle('upstream', zn, zg, npg, 0.2, upstream=3.0)
    _, _, dzn1, dzg1 = _ours(zn, zg, npg, 0.2)
    assert GL.row_rel_err(dzn3, 3.0 * dzn1) < 1e-5 and rel_err(dzg3, 3.0 * dzg1) < 1e-5


def test_global_local_is_the_swapped_call_and_inputs_may_live_anywhere():
    """case 10: NTXentGlobalLocal(zg, zn, npg) equals NTXentLocalGlobal(zn, zg, npg) bit for bit, gradients on the right tensors;
    nodes_per_graph as a list, a CPU tensor and a device tensor give the same bits"""
    npg = [6, 1, 9, 4]
    zn, zg = _inputs(npg, 24, 10)
    a = _ours(zn, zg, npg, 0.1)
    b = _ours(zn, zg, npg, 0.1, swapped=True)
    assert a[2].shape == zn.shape and a[3].shape == zg.shape and b[2].shape == zn.shape and b[3].shape == zg.shape
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    for form in (torch.tensor(npg), torch.tensor(npg, dtype=torch.int32), torch.tensor(npg).to(DEV)):
        c = _ours(zn, zg, form, 0.1)
        assert all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))


def test_two_runs_are_bit_identical():
    """case 11, at the fixture's long case and on a tall batch whose K = N product runs in slices"""
    z = load('local_global.npz')
    p = 'loss/long/'
    runs = [_ours(z[p + 'zn'], z[p + 'zg'], z[p + 'nodes_per_graph'].tolist(), 0.1) for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(runs[0][1:], runs[1][1:]))
    npg = [37 * (j % 5) + 11 for j in range(40)]          # N = 3400, B = 40
    zn, zg = _inputs(npg, 64, 11)
    runs = [_ours(zn, zg, npg, 0.1) for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(runs[0][1:], runs[1][1:]))


def _model_step(z):
    model = amd.PNALocal(**GL.MODEL)
    model.load_state_dict(sd_from_npz(z, 'model/sd'), strict=True)
    model.to(DEV).train()
    g = amd.batch([amd.bond_graph(m) for m in mols_from_npz(z, 'model/mol')]).to(DEV)
    y = model(g)
    loss = amd.NTXentLocalGlobal(tau=GL.MODEL_TAU)(y, torch.from_numpy(z['model/zg']).to(DEV), g.batch_num_nodes())
    loss.backward()
    return model, g, y, loss.item(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


def test_pna_local_matches_reference_fixture():
    """case 12: output, loss, every parameter gradient, the BatchNorm buffers after the step and the ndata['feat'] side effect, with
    the bounds tests/test_gpu_egnn.py uses for its fixture: 1e-4 on the output and the loss, max(1e-3, 4 x ref_err) per gradient,
    1e-5 on the running statistics."""
    z = load('local_global.npz')
    model, g, y, loss, got = _model_step(z)
    assert y.shape == z['model/out'].shape and g.ndata['feat'] is y and float(y.detach().min()) >= 0.0
    print(f'model: out rel_err {rel_err(y.detach().cpu(), z["model/out64"]):.2e} loss {loss:.8f} ref {float(z["model/loss64"]):.8f}')
    ref = sd_from_npz(z, 'model/grad')
    assert set(got) == set(ref)
    scale = max(float(v.abs().max()) for v in ref.values())
    for k, v in ref.items():
        rtol = max(1e-3, 4 * float(z[f'model/ref_err/grad/{k}']))
        err = float((got[k].double() - v.double()).abs().max())
        print(f'model: grad {k}: err {err:.3e} max {float(v.abs().max()):.3e} rtol {rtol:.1e} scale {scale:.3e}')
    assert rel_err(y.detach().cpu(), z['model/out']) < 1e-4
    assert abs(loss - float(z['model/loss'])) < 1e-4 * abs(float(z['model/loss']))
    for k, v in ref.items():
        rtol = max(1e-3, 4 * float(z[f'model/ref_err/grad/{k}']))
        grads_close({k: got[k], '_scale': torch.tensor([scale])}, {k: v, '_scale': torch.tensor([scale])}, rtol, what='model: ')
    sd = model.state_dict()
    for k, v in sd_from_npz(z, 'model/buf_after').items():
        if 'running' in k:
            assert rel_err(sd[k].cpu(), v) < 1e-5, k
        else:
            assert int(sd[k]) == int(v), k


def test_pna_local_step_is_bit_identical_and_eval_runs():
    z = load('local_global.npz')
    m0, _, y0, l0, g0 = _model_step(z)
    m1, _, y1, l1, g1 = _model_step(z)
    assert torch.equal(y0, y1) and l0 == l1 and all(torch.equal(g0[k], g1[k]) for k in g0)
    m0.eval()
    g = amd.batch([amd.bond_graph(m) for m in mols_from_npz(z, 'model/mol')]).to(DEV)
    with torch.no_grad():
        y = m0(g)
    assert y.shape == y0.shape and torch.isfinite(y).all() and g.ndata['feat'] is y
