"""The derived error bound of tests/ntxent_reference.py is neither too tight nor too loose (no GPU, no HIP library):

* the inputs of every (case, kind) meet the conditions under which no element is ambiguous,
* an fp32 emulation of the evaluation order of csrc/ntxent.hip - the per-thread stride of 256, the block tree, both backward
  generations - stays inside it on every case and kind the GPU test runs, on the row kernels alone and from the embeddings,
* so does the repository's fp32 oracle through autograd (torch's own summation order), row shards taken as row slices,
* and each of six one-line defects, injected into the emulation, leaves it on the case that was made for it.
"""
import numpy as np
import pytest

import ntxent_reference as R
from oracle import pna3d_oracle as O

ROW_NAMES = ('row_sum', 'row_pos', 'row_loss', 'loss', 'dsim', 'ca', 'cb')
Z_NAMES = ('n1', 'n2', 'sim') + ROW_NAMES + ('dz1', 'dz2')


def _ratios(tag, out, ref, names):
    """worst error / bound of every named quantity, printed with its place"""
    res = {}
    for n in names:
        r, k = R.worst(getattr(out, n), getattr(ref, n), getattr(ref, 'e_' + n))
        at = tuple(int(x) for x in np.unravel_index(k, np.shape(getattr(ref, n)))) if np.ndim(getattr(ref, n)) else ()
        res[n] = r
        print(f'  {tag} {n}: worst error/bound {r:.3f} at {at}')
    return res


def _names(I, names):
    # without normalisation there are no norms to compare and no coefficients in the gradients (they are still computed by the
    # row kernels from the unit norms, and compared there)
    return [n for n in names if I.norm or n not in ('n1', 'n2')]


@pytest.mark.parametrize('case_id,kind', R.COMBOS, ids=R.COMBO_IDS)
def test_inputs_are_unambiguous(case_id, kind):
    I = R.inputs(case_id, kind)
    R.input_conditions(I)
    worst_den = float((I.ref.e_den / I.ref.den).max())
    print(f'  {case_id}-{kind}: worst e_den / den from z {worst_den:.3e}, rows alone {float((I.ref_rows.e_den / I.ref_rows.den).max()):.3e}, '
          f'worst pos / den {float((I.ref.row_pos / I.ref.den).max()):.3e}')


@pytest.mark.parametrize('generation', ['fused', 'sequenced'])
@pytest.mark.parametrize('case_id,kind', R.COMBOS, ids=R.COMBO_IDS)
def test_emulation_stays_inside_the_bound(case_id, kind, generation):
    I = R.inputs(case_id, kind)
    rows = R.emulate(None, None, I.conf, I.pos_offset, I.tau, I.eps, I.loss_scale, generation=generation, given=I.given)
    res = _ratios('rows', rows, I.ref_rows, ROW_NAMES)
    full = R.emulate(I.z1, I.z2, I.conf, I.pos_offset, I.tau, I.eps, I.loss_scale, generation=generation, norm=I.norm)
    if not I.norm:
        full.n1, full.n2 = I.ref.n1, I.ref.n2
    res.update({'z_' + k: v for k, v in _ratios('from z', full, I.ref, _names(I, Z_NAMES)).items()})
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad
    if kind == 'zero_rows':
        z1r, z2r = R.zero_rows_of(I.case)
        assert full.ca[z1r] == 0 and full.cb[z2r] == 0 and rows.ca[z1r] == 0 and rows.cb[z2r] == 0


@pytest.mark.parametrize('case_id,kind', R.COMBOS, ids=R.COMBO_IDS)
def test_oracle_stays_inside_the_bound(case_id, kind):
    """oracle.pna3d_oracle.ntxent / ntxent_multiple_positives in fp32 on the whole batch; the rows of a shard case are the row
    slice of the whole batch's gradient"""
    I = R.inputs(case_id, kind)
    z1 = I.z1_full.clone().requires_grad_(True)
    z2 = I.z2.clone().requires_grad_(True)
    loss = O.ntxent(z1, z2, I.tau, norm=I.norm) if I.conf == 1 else O.ntxent_multiple_positives(z1, z2, I.tau, norm=I.norm)
    loss.backward()
    out = R.SimpleNamespace(loss=loss.detach(), dz1=z1.grad, dz2=z2.grad)
    res = _ratios('oracle', out, I.full, ('loss', 'dz1', 'dz2'))
    if I.case.shards is not None:
        sl = R.SimpleNamespace(dz1=z1.grad[I.pos_offset:I.pos_offset + I.b1])
        res.update({'slice_' + k: v for k, v in _ratios('oracle rows', sl, I.ref, ('dz1',)).items()})
    if kind == 'aligned':
        print(f'  oracle abs err: loss {abs(loss.item() - I.full.loss):.3e}, dz1 {np.abs(z1.grad.double().numpy() - I.full.dz1).max():.3e}')
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, bad


# the case each defect was made for (the first entry), and one where it cannot show (None: shows everywhere)
DEFECT_CASES = {
    'drop_last': ('min', None),                # the last column of a row dropped from row_sum
    'p0': ('shard_c3', 'shard_last'),          # p0 = pos_offset * conf + i: needs conf > 1
    'ca_tail': ('tail1', 'stride'),            # ca not applied to the dz1 columns from 256 onwards: needs dim > 256
    'col256': ('stride', 'tail1'),             # the fused column loop stops after 256 rows: needs b1 > 256
    'cb_sign': ('min', None),
    'gpos_den': ('min', None),                 # -gs / den for the positives
}


def _worst_from_z(I, generation, defect):
    o = R.emulate(I.z1, I.z2, I.conf, I.pos_offset, I.tau, I.eps, I.loss_scale, generation=generation, defect=defect)
    return {n: R.worst(getattr(o, n), getattr(I.ref, n), getattr(I.ref, 'e_' + n))[0] for n in ROW_NAMES + ('dz1', 'dz2')}


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_injected_defect_leaves_the_bound(defect):
    assert set(DEFECT_CASES) == set(R.DEFECTS)
    hit, miss = DEFECT_CASES[defect]
    generations = ('fused',) if defect in ('ca_tail', 'col256') else ('fused', 'sequenced')
    for generation in generations:
        res = _worst_from_z(R.inputs(hit, 'random'), generation, defect)
        print(f'  {defect} on {hit} ({generation}): ' + ', '.join(f'{k} {v:.3g}' for k, v in res.items() if v > 1.0))
        assert max(res.values()) > 1.0, (defect, hit, generation, res)
        if miss is not None:
            res = _worst_from_z(R.inputs(miss, 'random'), generation, defect)
            assert max(res.values()) <= 1.0, (defect, miss, generation, res)


def test_every_case_of_the_issue_is_there():
    shapes = {c.id: (c.b1, c.b2, c.conf, c.dim, c.pos_offset, c.tau) for c in R.CASES}
    assert shapes == {'min': (2, 2, 1, 7, 0, 0.1), 'c3wide': (9, 9, 3, 516, 0, 0.1), 'tail1': (65, 65, 1, 300, 0, 0.1),
                      'stride': (257, 257, 1, 64, 0, 0.1), 'posacross': (86, 86, 3, 36, 0, 0.1),
                      'shard_last': (16, 67, 1, 40, 51, 0.1), 'shard_c3': (5, 21, 3, 20, 16, 0.1),
                      'tau0.05': (33, 33, 1, 64, 0, 0.05), 'tau0.5': (33, 33, 1, 64, 0, 0.5)}
    for c in R.CASES:
        if c.shards is not None:
            assert sum(c.shards) == c.b2 and c.shards[-1] == c.b1 and sum(c.shards[:-1]) == c.pos_offset
