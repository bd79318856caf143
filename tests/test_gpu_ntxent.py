"""-m gpu: the NT-Xent kernels of csrc/ntxent.hip against the fp64 reference of tests/ntxent_reference.py - every element of
every output inside the DERIVED rounding bound of that file (no chosen tolerance), at the shapes where the thread maps split
(ntxent_reference.CASES) and on random, aligned, collapsed, zero-row and unnormalised inputs (ntxent_reference.kinds_of).

  the row kernels alone     ops.row_norms, ops.ntxent_fwd, ops.ntxent_bwd on a given fp32 sim, n1, n2
  the default form          i3d_ntxent_loss_fwd / _bwd through ctypes, scratch and work read back, guard bands behind every buffer
  both forms                losses.NTXentFn with LOSS_COMPOSITE on and off: loss, dz1, dz2; two runs give the same bits; the
                            generation that ran is counted; shards summed against the whole batch; the modules on conf = 3
  an upstream gradient      (loss * 0.25).backward() inside the same bound

Every check prints its worst error / bound ratio, and the element where it occurs, before it asserts.
"""
import importlib

import pytest
import torch

import ntxent_reference as R

pytestmark = pytest.mark.gpu
ops = None
lib = None
losses = None
DEV = None
FILL = 0x7FC0BEEF             # a quiet NaN with a payload: nothing computes it


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    global ops, lib, losses, DEV
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    ops = importlib.import_module('3dinfomax_amd.ops')
    lib = importlib.import_module('3dinfomax_amd._lib')
    losses = importlib.import_module('3dinfomax_amd.losses')
    DEV = torch.device('cuda:0')
    yield


def g(t):
    return t.to(DEV)


def _filled(n, guard=64):
    return torch.full((n + guard,), FILL, dtype=torch.int32, device=DEV).view(torch.float32)


def _keeps_fill(buf, start):
    return bool((buf[start:].view(torch.int32) == FILL).all().item())


NORM_COMBOS = [(c, k) for c, k in R.COMBOS if k != 'unnormalised']
NORM_IDS = [f'{c}-{k}' for c, k in NORM_COMBOS]


@pytest.mark.parametrize('case_id,kind', R.COMBOS, ids=R.COMBO_IDS)
def test_row_kernels_alone(case_id, kind):
    I = R.inputs(case_id, kind)
    R.input_conditions(I)
    ref = I.ref_rows
    print(f'\n{case_id}-{kind}: row kernels')
    if I.norm:
        R.check('n1', ops.row_norms(g(I.z1)), I.ref.n1, I.ref.e_n1)
        R.check('n2', ops.row_norms(g(I.z2)), I.ref.n2, I.ref.e_n2)
    sim, n1, n2 = (g(x) for x in I.given)
    rs, rp, loss = ops.ntxent_fwd(sim, n1, n2, I.b1, I.b2, I.conf, I.pos_offset, I.tau, I.eps, I.loss_scale)
    up = torch.ones(1, device=DEV)
    dsim, ca, cb = ops.ntxent_bwd(sim, n1, n2, rs, rp, I.b1, I.b2, I.conf, I.pos_offset, I.tau, I.eps, I.loss_scale, up)
    R.check('row_sum', rs, ref.row_sum, ref.e_row_sum)
    R.check('row_pos', rp, ref.row_pos, ref.e_row_pos)
    R.check('loss', loss, ref.loss, ref.e_loss)
    R.check('dsim', dsim, ref.dsim, ref.e_dsim)
    R.check('ca', ca, ref.ca, ref.e_ca)
    R.check('cb', cb, ref.cb, ref.e_cb)
    if kind == 'zero_rows':
        z1r, z2r = R.zero_rows_of(I.case)
        assert ca[z1r].item() == 0.0 and cb[z2r].item() == 0.0


@pytest.mark.parametrize('case_id,kind', NORM_COMBOS, ids=NORM_IDS)
def test_default_form_through_ctypes(case_id, kind):
    """i3d_ntxent_loss_fwd / _bwd with the test's own buffers: scratch = n1 | n2 | row_sum | row_pos | sim, each part padded to
    four floats; work = dsim (the fused form writes no ca / cb behind it)"""
    I = R.inputs(case_id, kind)
    ref = I.ref
    L = lib.load()
    b1, b2, b2c, dim = I.b1, I.b2, I.ncol, I.dim

    def al(n):
        return (n + 3) & ~3

    ns = L.i3d_ntxent_loss_scratch_floats(b1, b2c)
    assert ns == 3 * al(b1) + al(b2c) + al(b1 * b2c)
    nw = al(b1 * b2c) + al(b1) + al(b2c)
    scratch, work, loss = _filled(ns), _filled(nw), _filled(1)
    dz1, dz2 = _filled(b1 * dim), _filled(b2c * dim)
    z1, z2 = g(I.z1), g(I.z2)
    up = torch.ones(1, device=DEV)
    lib.check(L.i3d_ntxent_loss_fwd(z1.data_ptr(), z2.data_ptr(), b1, b2, I.conf, dim, I.pos_offset, float(I.tau), float(I.eps),
                                    I.loss_scale, scratch.data_ptr(), loss.data_ptr(), ops._stream()), 'i3d_ntxent_loss_fwd')
    lib.check(L.i3d_ntxent_loss_bwd(z1.data_ptr(), z2.data_ptr(), b1, b2, I.conf, dim, I.pos_offset, float(I.tau), float(I.eps),
                                    I.loss_scale, scratch.data_ptr(), up.data_ptr(), work.data_ptr(), dz1.data_ptr(),
                                    dz2.data_ptr(), ops._stream()), 'i3d_ntxent_loss_bwd')
    torch.cuda.synchronize()
    o = 0
    parts = {}
    for name, n in (('n1', b1), ('n2', b2c), ('row_sum', b1), ('row_pos', b1), ('sim', b1 * b2c)):
        parts[name] = scratch[o:o + n]
        o += al(n)
    print(f'\n{case_id}-{kind}: default form, one C call per direction')
    R.check('n1', parts['n1'], ref.n1, ref.e_n1)
    R.check('n2', parts['n2'], ref.n2, ref.e_n2)
    R.check('sim', parts['sim'], ref.sim, ref.e_sim)
    R.check('row_sum', parts['row_sum'], ref.row_sum, ref.e_row_sum)
    R.check('row_pos', parts['row_pos'], ref.row_pos, ref.e_row_pos)
    R.check('loss', loss[:1], ref.loss, ref.e_loss)
    R.check('dsim', work[:b1 * b2c], ref.dsim, ref.e_dsim)
    R.check('dz1', dz1[:b1 * dim], ref.dz1, ref.e_dz1)
    R.check('dz2', dz2[:b2c * dim], ref.dz2, ref.e_dz2)
    assert _keeps_fill(work, b1 * b2c), 'words of work behind dsim were written'
    assert _keeps_fill(scratch, ns) and _keeps_fill(loss, 1), 'guard band behind scratch / loss'
    assert _keeps_fill(dz1, b1 * dim) and _keeps_fill(dz2, b2c * dim), 'guard band behind dz1 / dz2'


class _Counts:
    """counts the calls of the two backward generations: ops.ntxent_bwd (sequenced from Python) and i3d_ntxent_loss_bwd"""

    def __init__(self, monkeypatch):
        self.sequenced = self.fused = 0
        L = lib.load()
        seq, fus = ops.ntxent_bwd, L.i3d_ntxent_loss_bwd

        def count_seq(*a, **k):
            self.sequenced += 1
            return seq(*a, **k)

        def count_fus(*a):
            self.fused += 1
            return fus(*a)

        monkeypatch.setattr(ops, 'ntxent_bwd', count_seq)
        monkeypatch.setattr(L, 'i3d_ntxent_loss_bwd', count_fus)

    def take(self):
        c = (self.fused, self.sequenced)
        self.sequenced = self.fused = 0
        return c


def _expected_counts(composite, norm, calls=1):
    return (calls, 0) if (composite and norm) else (0, calls)


def _run_fn(I, z1, z2, pos_offset, upstream=1.0):
    """(loss, dz1, dz2) of NTXentFn on the local rows z1 against the gathered z2"""
    a, b = g(z1).requires_grad_(True), g(z2).requires_grad_(True)
    loss = losses.NTXentFn.apply(a, b, I.tau, I.eps, I.conf, pos_offset, I.b2, I.norm)
    (loss * upstream if upstream != 1.0 else loss).backward()
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize('composite', [True, False], ids=['default', 'sequenced'])
@pytest.mark.parametrize('case_id,kind', R.COMBOS, ids=R.COMBO_IDS)
def test_both_forms_through_ntxentfn(case_id, kind, composite, monkeypatch):
    I = R.inputs(case_id, kind)
    monkeypatch.setattr(losses, 'LOSS_COMPOSITE', composite)
    counts = _Counts(monkeypatch)
    loss, dz1, dz2 = _run_fn(I, I.z1, I.z2, I.pos_offset)
    assert counts.take() == _expected_counts(composite, I.norm), 'the other generation ran'
    print(f'\n{case_id}-{kind}: NTXentFn, {"default" if composite else "sequenced"} form')
    R.check('loss', loss, I.ref.loss, I.ref.e_loss)
    R.check('dz1', dz1, I.ref.dz1, I.ref.e_dz1)
    R.check('dz2', dz2, I.ref.dz2, I.ref.e_dz2)
    loss_b, dz1_b, dz2_b = _run_fn(I, I.z1, I.z2, I.pos_offset)
    assert torch.equal(loss.view(torch.int32), loss_b.view(torch.int32))
    assert torch.equal(dz1.view(torch.int32), dz1_b.view(torch.int32)) and torch.equal(dz2.view(torch.int32), dz2_b.view(torch.int32))


@pytest.mark.parametrize('composite', [True, False], ids=['default', 'sequenced'])
@pytest.mark.parametrize('case_id,kind', R.COMBOS, ids=R.COMBO_IDS)
def test_upstream_gradient_scales_inside_the_bound(case_id, kind, composite, monkeypatch):
    I = R.inputs(case_id, kind, 0.25)
    monkeypatch.setattr(losses, 'LOSS_COMPOSITE', composite)
    loss, dz1, dz2 = _run_fn(I, I.z1, I.z2, I.pos_offset, upstream=0.25)
    print(f'\n{case_id}-{kind}: upstream 0.25, {"default" if composite else "sequenced"} form')
    R.check('loss', loss, I.ref.loss, I.ref.e_loss)
    R.check('dz1', dz1, I.ref.dz1, I.ref.e_dz1)
    R.check('dz2', dz2, I.ref.dz2, I.ref.e_dz2)


SHARD_COMBOS = [(c, k) for c, k in R.COMBOS if R.CASE_BY_ID[c].shards is not None]


@pytest.mark.parametrize('composite', [True, False], ids=['default', 'sequenced'])
@pytest.mark.parametrize('case_id,kind', SHARD_COMBOS, ids=[f'{c}-{k}' for c, k in SHARD_COMBOS])
def test_shards_sum_to_the_whole_batch(case_id, kind, composite, monkeypatch):
    """every shard of the batch through NTXentFn with its pos_offset, the shares and the gradients summed by autograd, against
    the fp64 result of the whole batch; the further fp32 additions of the sum are one u each on the sizes of the terms"""
    I = R.inputs(case_id, kind)
    full, shards = I.full, I.case.shards
    monkeypatch.setattr(losses, 'LOSS_COMPOSITE', composite)
    counts = _Counts(monkeypatch)
    a, b = g(I.z1_full).requires_grad_(True), g(I.z2).requires_grad_(True)
    total, off = None, 0
    for n in shards:
        share = losses.NTXentFn.apply(a[off:off + n], b, I.tau, I.eps, I.conf, off, I.b2, I.norm)
        total = share if total is None else total + share
        off += n
    total.backward()
    assert counts.take() == _expected_counts(composite, I.norm, len(shards)), 'the other generation ran'
    extra = len(shards) * R.U
    print(f'\n{case_id}-{kind}: {len(shards)} shards, {"default" if composite else "sequenced"} form')
    R.check('loss', total.detach(), full.loss, full.e_loss + extra * full.sum_abs_row_loss)
    R.check('dz1', a.grad, full.dz1, full.e_dz1 + extra * full.m_dz1)
    R.check('dz2', b.grad, full.dz2, full.e_dz2 + extra * full.m_dz2)


CONF3 = [(c, k) for c, k in R.COMBOS if R.CASE_BY_ID[c].conf == 3]


@pytest.mark.parametrize('composite', [True, False], ids=['default', 'sequenced'])
@pytest.mark.parametrize('case_id,kind', CONF3, ids=[f'{c}-{k}' for c, k in CONF3])
def test_multiple_positives_module(case_id, kind, composite, monkeypatch):
    """NTXentMultiplePositives on the whole batch of the conf = 3 cases (no epsilon, mean over the batch)"""
    I = R.inputs(case_id, kind)
    full = I.full
    monkeypatch.setattr(losses, 'LOSS_COMPOSITE', composite)
    counts = _Counts(monkeypatch)
    a, b = g(I.z1_full).requires_grad_(True), g(I.z2).requires_grad_(True)
    loss = losses.NTXentMultiplePositives(norm=I.norm, tau=I.tau)(a, b)
    loss.backward()
    assert counts.take() == _expected_counts(composite, I.norm), 'the other generation ran'
    print(f'\n{case_id}-{kind}: NTXentMultiplePositives, {"default" if composite else "sequenced"} form')
    R.check('loss', loss.detach(), full.loss, full.e_loss)
    R.check('dz1', a.grad, full.dz1, full.e_dz1)
    R.check('dz2', b.grad, full.dz2, full.e_dz2)
