"""The derived error bound of tests/agg_reference.py is neither too tight nor too loose (no GPU, no HIP library):

* an fp32 emulation of the evaluation order of csrc/aggregate.hip (sequential j = 0 .. D-1, the kernels' expressions, every
  operation rounded to fp32) stays inside it on every case the GPU test runs,
* so does the repository's fp32 oracle (torch's own summation order; the backward through autograd),
* and each of five defects a four-rows-per-trip kernel can have, injected into the emulation, leaves it.
"""
import math

import numpy as np
import pytest
import torch

import agg_reference as R
from oracle import pna3d_oracle as O

f32 = np.float32


def _scaler_pair(D, avg, defect):
    """amp, att as scaler_values() of the kernel: rounded to fp32 from a double evaluation"""
    if defect == 'table31' and D >= 32:
        D = 31
    l = math.log(D + 1)
    return f32(l / float(f32(avg))), f32(float(f32(avg)) / l)


def _rows(e, aff, beg, D, defect):
    """the D message rows of one node as the kernel forms them, [D, F] float32"""
    x = e[beg:beg + D].copy()
    if aff is not None:
        n = 4 if defect == 'aff4' else D
        x[:n] = (x[:n] - aff[0]) * aff[1] + aff[2]           # three float32 operations
    return x


def _dropped(D, defect):
    """rows that take part in the statistics: all of them, or without the last row of a partial trip"""
    return D - 1 if (defect == 'drop_tail' and D > 4 and D % 4 != 0) else D


def emulate_fwd(e, in_ptr, aggs, scalers, avg, force, aff=None, defect=None):
    e = e.float().numpy()
    aff = None if aff is None else aff.numpy()
    eff = R.effective_scalers(scalers, force)
    N, F = in_ptr.shape[0] - 1, e.shape[1]
    out = np.zeros((N, len(eff) * len(aggs), F), dtype=f32)
    for v in range(N):
        beg, D = int(in_ptr[v]), int(in_ptr[v + 1] - in_ptr[v])
        if D <= 0:
            continue
        x = _rows(e, aff, beg, D, defect)
        s, sq, mx, mn = x[0].copy(), x[0] * x[0], x[0].copy(), x[0].copy()
        for j in range(1, _dropped(D, defect)):
            s = s + x[j]
            sq = sq + x[j] * x[j]
            mx, mn = np.maximum(mx, x[j]), np.minimum(mn, x[j])
        mean, msq = s / f32(D), sq / f32(D)
        var = np.maximum(msq - mean * mean, f32(0))
        val = {'sum': s, 'mean': mean, 'max': mx, 'min': mn, 'var': var, 'std': np.sqrt(var + f32(1e-5))}
        amp, att = _scaler_pair(D, avg, defect)
        for si, sname in enumerate(eff):
            for k, a in enumerate(aggs):
                sc = {'identity': None, 'amplification': amp, 'attenuation': att}[sname]
                if defect == 'amp_std' and sname == 'attenuation' and a == 'std':
                    sc = amp
                out[v, si * len(aggs) + k] = val[a] if sc is None else val[a] * sc
    return out.reshape(N, -1)


def emulate_bwd(gout, e, in_ptr, aggs, scalers, avg, force, aff=None, defect=None):
    e = e.float().numpy()
    aff = None if aff is None else aff.numpy()
    eff = R.effective_scalers(scalers, force)
    N, F = in_ptr.shape[0] - 1, e.shape[1]
    go = gout.numpy().reshape(N, len(eff) * len(aggs), F)
    ge = np.zeros_like(e)
    for v in range(N):
        beg, D = int(in_ptr[v]), int(in_ptr[v + 1] - in_ptr[v])
        if D <= 0:
            continue
        amp, att = _scaler_pair(D, avg, defect)
        g = {a: np.zeros(F, dtype=f32) for a in ('sum', 'mean', 'max', 'min', 'var', 'std')}
        for si, sname in enumerate(eff):
            for k, a in enumerate(aggs):
                sc = {'identity': f32(1), 'amplification': amp, 'attenuation': att}[sname]
                if defect == 'amp_std' and sname == 'attenuation' and a == 'std':
                    sc = amp
                g[a] = g[a] + go[v, si * len(aggs) + k] * sc
        x = _rows(e, aff, beg, D, defect)
        s, sq = np.zeros(F, dtype=f32), np.zeros(F, dtype=f32)
        mx, mn = np.full(F, -np.inf, dtype=f32), np.full(F, np.inf, dtype=f32)
        amax, amin = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
        for j in range(_dropped(D, defect)):
            s = s + x[j]
            sq = sq + x[j] * x[j]
            hi = x[j] >= mx if (defect == 'tie_last' and j > 0) else x[j] > mx
            lo = x[j] <= mn if (defect == 'tie_last' and j > 0) else x[j] < mn
            mx, amax = np.where(hi, x[j], mx), np.where(hi, j, amax)
            mn, amin = np.where(lo, x[j], mn), np.where(lo, j, amin)
        fD = f32(D)
        mean = s / fD
        raw = sq / fD - mean * mean
        pos = raw > 0
        sd = np.sqrt(np.maximum(raw, f32(0)) + f32(1e-5))
        kstd = np.where(pos, g['std'] / (fD * sd), f32(0))
        kvar = np.where(pos, g['var'] * f32(2) / fD, f32(0))
        gm = g['mean'] / fD + g['sum']
        for j in range(D):
            r = gm + (kstd + kvar) * (x[j] - mean)
            r = np.where(amax == j, r + g['max'], r)
            r = np.where(amin == j, r + g['min'], r)
            ge[beg + j] = r
    assert ge.dtype == f32
    return ge


def _run_emulation(inp, defect=None):
    e = inp.e
    out = emulate_fwd(e, inp.in_ptr, inp.aggs, inp.scalers, inp.avg, inp.force, inp.aff, defect)
    ge = emulate_bwd(inp.cot, e, inp.in_ptr, inp.aggs, inp.scalers, inp.avg, inp.force, inp.aff, defect)
    return out, ge


def test_the_graph_and_the_case_matrix():
    ptr = R.graph_in_ptr()
    deg = np.diff(ptr)
    assert len(deg) == 47 and deg[0] == 0 and deg[-1] == 0 and int(ptr[-1]) == 936
    assert {31, 32, 33, 64, 101} <= set(deg.tolist())
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)
    for c in R.CASES:
        if c.F % 4 == 0:
            assert (47 * c.F // 4) % 256 != 0          # the last workgroup is partial


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_fp32_emulation_of_the_kernels_stays_inside_the_bound(case_id):
    inp = R.inputs(case_id)
    out, ge = _run_emulation(inp)
    rf, rb = R.worst_ratio(out, inp.ref_fwd, inp.bound_fwd), R.worst_ratio(ge, inp.ref_bwd, inp.bound_bwd)
    print(f'{case_id}: emulation worst error / bound: forward {rf:.3f} backward {rb:.3f}')
    assert R.zero_rows_are_plus_zero(out, inp.in_ptr)
    assert rf <= 1.0 and rb <= 1.0


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_fp32_oracle_stays_inside_the_bound(case_id):
    inp = R.inputs(case_id)
    m = inp.m.clone().requires_grad_(True)
    dst = torch.from_numpy(np.repeat(np.arange(inp.N), np.diff(inp.in_ptr)))

    def reduce_fn(mb, D):
        if inp.force and len(inp.scalers) == 1:        # the oracle's reduce keeps the reference's quirk: apply the one scaler here
            return O.scale(O.pna_reduce(mb, D, inp.aggs, ['identity']), inp.scalers[0], D, inp.avg)
        return O.pna_reduce(mb, D, inp.aggs, inp.scalers, inp.avg)
    out = O.degree_bucketed_reduce(m, dst, inp.N, reduce_fn, inp.nblk * inp.F)
    (out * inp.cot).sum().backward()
    rf = R.worst_ratio(out.detach(), inp.ref_fwd, inp.bound_fwd)
    rb = R.worst_ratio(m.grad, inp.ref_bwd, inp.bound_bwd)
    print(f'{case_id}: oracle worst error / bound: forward {rf:.3f} backward {rb:.3f}')
    assert rf <= 1.0 and rb <= 1.0


@pytest.mark.parametrize('defect', ['drop_tail', 'table31', 'tie_last', 'aff4', 'amp_std'])
def test_an_injected_defect_leaves_the_bound(defect):
    """the last row of a partial trip dropped; amp[31] / att[31] used for D >= 32; a tie routed to the last index; aff applied to
    the first four rows only; the std block scaled by amp where att belongs"""
    caught = []
    for case_id in ('std12-F20-aff', 'general-F7-fp32'):
        inp = R.inputs(case_id)
        out, ge = _run_emulation(inp, defect)
        if R.worst_ratio(out, inp.ref_fwd, inp.bound_fwd) > 1.0 or R.worst_ratio(ge, inp.ref_bwd, inp.bound_bwd) > 1.0:
            caught.append(case_id)
    print(f'{defect}: caught on {caught}')
    assert caught


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_the_ambiguous_elements_are_the_constant_columns(case_id):
    """a condition on the inputs, not a measurement: the fp32 `raw > 0` test is undecided exactly where a node's column is
    constant (degree 1, the tie copy of degree 2, the constant nodes of degree 9) - nowhere else is var within e_var of 0"""
    inp = R.inputs(case_id)
    assert np.array_equal(inp.ambiguous, R.constant_elements(inp.m, inp.in_ptr))
    deg = np.diff(inp.in_ptr)
    rows_of_nine = np.repeat(deg == R.CONSTANT_DEGREE, deg)
    assert inp.ambiguous[rows_of_nine].all() and rows_of_nine.sum() == 27
