"""-m gpu: the PNA aggregation (K4) and readout (K6) kernels of csrc/aggregate.hip, through 3dinfomax_amd/ops.py, against the
fp64 reference of tests/agg_reference.py at high in-degrees - every element inside the DERIVED rounding bound of that file
(no chosen tolerance), on one graph whose degrees cross the scaler table's end (31 / 32 / 33), run the four-rows-per-trip loops
for up to 25 trips with every tail length, and include isolated nodes first, last and in between.

Per case: forward and backward, the worst error / bound ratio printed before the assert.  The cases (agg_reference.CASES):
  std12 (MODE 1), F 4 / 20 / 200:   fp32, bf16 messages, BatchNorm affine on load (aff), aff + bf16
  ident4 (MODE 2), F 20 / 200:      fp32, bf16, aff
  general / forced_amp (MODE 0):    F 20, and F 7 (the scalar kernels, V = 1 backward with long segments)
  std12 + aff, F 340 / 344:         the backward's LDS staging of aff at its limit / its per-lane global loads
  tower-major, F 36, towers of 12:  all four configurations, against the reference with the columns permuted
  readout (min, max, mean, sum):    F 200 and 7, the same pointer array as graph pointer
"""
import importlib

import numpy as np
import pytest
import torch

import agg_reference as R

pytestmark = pytest.mark.gpu
ops = None
lib = None
DEV = None


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    global ops, lib, DEV
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    ops = importlib.import_module('3dinfomax_amd.ops')
    lib = importlib.import_module('3dinfomax_amd._lib')
    DEV = torch.device('cuda:0')
    yield


def g(t):
    return None if t is None else t.to(DEV)


def _run(inp):
    """(out, grad_e) of one case on the device, in the [block][feature] column order of the reference"""
    case = inp.case
    ptr = g(torch.from_numpy(inp.in_ptr))
    e, cot = g(inp.e), g(inp.cot)
    if case.form == 'readout':
        codes = ops.agg_codes(inp.aggs)
        out = ops.segment_readout_fwd(e, ptr, inp.N, codes)
        ge = ops.segment_readout_bwd(cot, e, ptr, inp.N, codes)
        return out, ge
    ac, sc = ops.agg_codes(inp.aggs), ops.scaler_codes(inp.scalers)
    if case.form == 'tower':
        out_tm = ops.pna_aggregate_fwd(e, ptr, inp.N, ac, sc, inp.avg, inp.force, tower_feat=case.tower_feat)
        T = inp.F // case.tower_feat
        out = out_tm.reshape(inp.N, T, inp.nblk, case.tower_feat).permute(0, 2, 1, 3).reshape(inp.N, -1)
        cot_tm = g(R.to_tower_major(inp.cot, inp.nblk, case.tower_feat))
        ge = ops.pna_aggregate_bwd(cot_tm, e, ptr, inp.N, ac, sc, inp.avg, inp.force, tower_feat=case.tower_feat)
        return out, ge
    if case.form == 'fp32':
        out = ops.pna_aggregate_fwd(e, ptr, inp.N, ac, sc, inp.avg, inp.force)
        ge = ops.pna_aggregate_bwd(cot, e, ptr, inp.N, ac, sc, inp.avg, inp.force)
        return out, ge
    aff = g(inp.aff)
    out = ops.pna_aggregate_fwd_aff(e, aff, ptr, inp.N, ac, sc, inp.avg, inp.force)
    ge = ops.pna_aggregate_bwd_aff(cot, e, aff, ptr, inp.N, ac, sc, inp.avg, inp.force)
    return out, ge


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_aggregate_fwd_bwd_inside_the_derived_bound(case_id):
    inp = R.inputs(case_id)
    # the reference's messages are the kernels' messages, bit for bit (sub, mul, add in fp32; bf16 decoded exactly)
    assert torch.equal(ops.pna_messages_normalized(g(inp.e), g(inp.aff)).cpu(), inp.m)
    out, ge = _run(inp)
    torch.cuda.synchronize()
    out, ge = out.cpu(), ge.cpu()
    assert out.shape == inp.ref_fwd.shape and ge.shape == inp.ref_bwd.shape and ge.dtype == torch.float32
    rf = R.worst_ratio(out, inp.ref_fwd, inp.bound_fwd)
    rb = R.worst_ratio(ge, inp.ref_bwd, inp.bound_bwd)
    print(f'{case_id}: worst error / bound: forward {rf:.3f} backward {rb:.3f}')
    assert R.zero_rows_are_plus_zero(out, inp.in_ptr)
    assert rf <= 1.0, f'forward: worst error / bound {rf}'
    assert rb <= 1.0, f'backward: worst error / bound {rb}'


@pytest.mark.parametrize('case_id', ['std12-F200-fp32', 'std12-F200-aff_bf16'])
def test_aggregate_two_calls_give_identical_bits(case_id):
    inp = R.inputs(case_id)
    out1, ge1 = _run(inp)
    out2, ge2 = _run(inp)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(ge1.view(torch.int32), ge2.view(torch.int32))


@pytest.mark.parametrize('F', [20, 7])
@pytest.mark.parametrize('config', ['std12', 'general'])
def test_aggregate_launch_without_edges(F, config):
    """five nodes, all of degree 0: zero rows forward; an empty gradient backward, without an error - the lanes without work
    of the backward read their own node's gradient row in place of a message row that does not exist"""
    aggs, scalers, force = R.CONFIGS[config]
    ac, sc = ops.agg_codes(aggs), ops.scaler_codes(scalers)
    N = 5
    ptr = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    e = torch.empty(0, F, dtype=torch.float32, device=DEV)
    out = ops.pna_aggregate_fwd(e, ptr, N, ac, sc, R.AVG, force)
    torch.cuda.synchronize()
    assert out.shape == (N, len(aggs) * len(scalers) * F)
    o = out.cpu().numpy()
    assert np.all(o == 0.0) and not np.signbit(o).any()
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    ge = ops.pna_aggregate_bwd(cot, e, ptr, N, ac, sc, R.AVG, force)
    torch.cuda.synchronize()
    assert ge.shape == (0, F)


def test_aggregate_aff_needs_a_multiple_of_four_features_in_both_directions():
    """i3d_pna_aggregate_fwd_ex and _bwd_ex: aff with F = 7 is refused before any launch (the V = 4 kernels load aff as float4,
    the scalar kernels are not built for it; the pair is only usable together)"""
    F, N = 7, 3
    ptr = torch.tensor([0, 2, 2, 5], dtype=torch.int32, device=DEV)
    e = torch.ones(5, F, device=DEV)
    aff = torch.ones(3, F, device=DEV)
    ac, sc = ops.agg_codes(R.STD_AGGS), ops.scaler_codes(['identity'])
    with pytest.raises(lib.HipLibraryError):
        ops.pna_aggregate_fwd_aff(e, aff, ptr, N, ac, sc, 1.0)
    with pytest.raises(lib.HipLibraryError):
        ops.pna_aggregate_bwd_aff(torch.ones(N, 4 * F, device=DEV), e, aff, ptr, N, ac, sc, 1.0)
    # without aff the same shapes run
    out = ops.pna_aggregate_fwd_aff(e, None, ptr, N, ac, sc, 1.0)
    ge = ops.pna_aggregate_bwd_aff(torch.ones(N, 4 * F, device=DEV), e, None, ptr, N, ac, sc, 1.0)
    torch.cuda.synchronize()
    assert out.shape == (N, 4 * F) and ge.shape == (5, F)
