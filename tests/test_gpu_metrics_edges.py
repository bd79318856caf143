"""The contrastive monitoring metrics (csrc/metrics.hip) and losses.uniformity_loss on the MI355X against the reference's fp64 results on
offset, collapsed and aligned inputs (fixture: tests/golden/gen_golden_metrics_edges.py, shapes and inputs from the fixture's builder).

Values: |ours - fp64| <= max(4 err_ref, floor), err_ref = |reference fp32 - fp64| from the fixture, floor = 2e-6 |fp64 value| (uniformity:
2e-6 absolute - the absolute error of a log is the relative error of the mean potential).  2e-6 is 16 times the worst error (1.2e-7) of a
CPU emulation of the centred fp32 formulation and a tenth of the smallest error (2e-5) of the uncentred second-moment formulation on any
family but `plain`.  The three rates: exactly the fp64 values (the fixture keeps every pair's (cos + 1) / 2 more than 1e-4 from the
threshold).  `zero_row`: NaN exactly where the reference is NaN.  Gradients of uniformity_loss: elementwise within
max(4 gerr_ref, 16 * 2^-23) max |grad64| of the fp64 autograd gradient, gerr_ref the error of the fp32 CPU gradient in the same measure.
Every check prints err, err_ref, allowed and their ratio before it asserts; the table of DESIGN.md ('Contrastive monitoring metrics') is
where the largest ratios go."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO

import gen_golden_metrics_edges as GE
from test_metrics_edges_cpu import edge_cases

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR = 2e-6
TAGS = GE.TAGS


def _metrics():
    return importlib.import_module('3dinfomax_amd.metrics')


def metric_objects(M):
    """the nine objects as train.py:255-268 builds them"""
    return {'positive_similarity': M.PositiveSimilarity(), 'negative_similarity': M.NegativeSimilarity(),
            'contrastive_accuracy': M.ContrastiveAccuracy(threshold=GE.THRESHOLD), 'true_negative_rate': M.TrueNegativeRate(threshold=GE.THRESHOLD),
            'true_positive_rate': M.TruePositiveRate(threshold=GE.THRESHOLD), 'uniformity': M.Uniformity(t=GE.T),
            'alignment': M.Alignment(alpha=GE.ALPHA), 'batch_variance': M.BatchVariance(), 'dimension_covariance': M.DimensionCovariance()}


def allowed_error(name, v64, err_ref):
    return max(4 * err_ref, FLOOR if name == 'uniformity' else FLOOR * abs(v64))


def check_value(tag, name, got, v64, err_ref, bad):
    err = abs(got - v64)
    allowed = allowed_error(name, v64, err_ref)
    print(f'{tag} {name}: err {err:.3e} err_ref {err_ref:.3e} allowed {allowed:.3e} ratio {err / allowed:.3f}')
    if not err <= allowed:
        bad.append((name, got, v64, err, allowed))


def device_values(M, z1, z2):
    """the nine metric objects, called as the trainer calls them, and the four statistics of contrastive_metrics"""
    got = {}
    for name, m in metric_objects(M).items():
        v = m(z1, z2)
        assert v.dim() == 0 and not v.is_cuda
        got[name] = v.item()
    allv = M.contrastive_metrics(z1, z2)
    for name in ('mean_pred', 'std_pred', 'mean_targets', 'std_targets'):
        got[name] = allv[name]
    return got


def check_case(M, c, what=''):
    z1, z2 = torch.from_numpy(c['z1'].copy()).to(DEV), torch.from_numpy(c['z2'].copy()).to(DEV)
    got = device_values(M, z1, z2)
    tag, bad = c['tag'] + what, []
    for name in GE.NAMES:
        v32, v64 = float(c['v32'][name]), float(c['v64'][name])
        if math.isnan(v64):
            print(f'{tag} {name}: {got[name]} (reference NaN)')
            if not math.isnan(got[name]):
                bad.append((name, got[name], v64))
        elif name in GE.RATES:
            print(f'{tag} {name}: {got[name]!r} reference {v64!r}')
            if got[name] != v64:
                bad.append((name, got[name], v64))
        else:
            check_value(tag, name, got[name], v64, abs(v32 - v64), bad)
    assert not bad, (tag, bad)


@pytest.mark.parametrize('idx', range(len(GE.CASES)), ids=TAGS)
def test_metrics_match_the_reference_fp64_values(idx):
    """all thirteen values of every case - the B2 > B1 cases (32x64+32) with uniformity, batch_variance and dimension_covariance, which
    see the appended rows"""
    check_case(_metrics(), edge_cases()[idx])


@pytest.mark.parametrize('setting', ['bf16', 'split'])
def test_metrics_do_not_follow_the_gemm_precision_setting(setting):
    ops = importlib.import_module('3dinfomax_amd.ops')
    prev = ops.set_matmul_precision('bf16') if setting == 'bf16' else ops.set_fp32_products('split')
    try:
        for tag in ('96x64_plain', '96x64_offset30'):
            check_case(_metrics(), edge_cases()[TAGS.index(tag)], what=f' [{setting}]')
        assert (ops.get_matmul_precision() == 'bf16') if setting == 'bf16' else (ops.get_fp32_products() == 'split')
    finally:
        ops.set_matmul_precision(prev) if setting == 'bf16' else ops.set_fp32_products(prev)


def test_second_metric_object_on_the_same_tensors_makes_no_new_pass(monkeypatch):
    M = _metrics()
    calls = []
    real = M._device_pass
    monkeypatch.setattr(M, '_device_pass', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    c = edge_cases()[TAGS.index('32x64+32_offset30')]
    z1, z2 = torch.from_numpy(c['z1'].copy()).to(DEV), torch.from_numpy(c['z2'].copy()).to(DEV)
    for m in metric_objects(M).values():
        m(z1, z2).item()
    assert len(calls) == 1
    vals = M._cache['values']
    M.contrastive_metrics(z1, z2)
    assert len(calls) == 1 and M._cache['values'] is vals
    z2.add_(0.0)                                            # an in-place update bumps the version: recomputed
    M.Alignment(alpha=2)(z1, z2).item()
    assert len(calls) == 2


# ---- the per-tensor path: BatchVariance / DimensionCovariance on x1 [B, 2 D], x2 [B C, D] -----------------------------------------------
PT_B, PT_D, PT_C = 24, 32, 3


@functools.lru_cache(maxsize=None)
def per_tensor_case(family):
    """-> x1 [B, 2 D], x2 [B C, D] (fp32) and per metric (fp32 oracle, fp64 oracle), evaluated per tensor"""
    g = torch.Generator().manual_seed(2400 + len(family))
    x1, x2 = torch.randn(PT_B, 2 * PT_D, generator=g) * 0.2, torch.randn(PT_B * PT_C, PT_D, generator=g) * 0.2
    if family == 'offset30':
        off = torch.randn(2 * PT_D, generator=g) * 30
        x1, x2 = x1 + off, x2 + off[:PT_D]
    else:
        assert family == 'collapsed'
        x1 = torch.randn(1, 2 * PT_D, generator=g) + 0.005 * x1
        x2 = torch.randn(1, PT_D, generator=g) + 0.005 * x2
    ref = {name: (f(x1, x2), f(x1.double(), x2.double())) for name, f in (('batch_variance', MO.batch_variance),
                                                                          ('dimension_covariance', MO.dimension_covariance))}
    return x1, x2, ref


@pytest.mark.parametrize('family', ['offset30', 'collapsed'])
def test_per_tensor_path_matches_the_fp64_oracle(family):
    M = _metrics()
    x1, x2, ref = per_tensor_case(family)
    z1, z2 = x1.to(DEV), x2.to(DEV)
    bad = []
    for name, obj in (('batch_variance', M.BatchVariance()), ('dimension_covariance', M.DimensionCovariance())):
        v32, v64 = ref[name]
        check_value(f'per-tensor {PT_B}x{2 * PT_D}|{PT_B * PT_C}x{PT_D}_{family}', name, obj(z1, z2).item(), v64, abs(v32 - v64), bad)
    assert not bad, bad


# ---- losses.uniformity_loss ---------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(base, family) for base in ('b96', 'b257') for family in ('plain', 'offset30', 'collapsed')]


def _pdist_uniformity(x1, x2, t=2):
    """the reference's expression (commons/losses.py:946-951)"""
    return sum(torch.pdist(x, p=2).pow(2).mul(-t).exp().mean().log() for x in (x1, x2)) / 2


@functools.lru_cache(maxsize=None)
def loss_case(base, family):
    """-> z1, z2 (fp32 numpy), the pdist expression's value in fp32 and fp64, its fp64 gradients and the fp32 gradients' error / max |grad64|"""
    bases = GE.fixture_bases(importlib.import_module('helpers').load('metrics_edges.npz'))
    z1, z2 = GE.build(bases[base], family)
    out = {}
    for dt in (torch.float32, torch.float64):
        a, b = (torch.from_numpy(z.copy()).to(dt).requires_grad_(True) for z in (z1, z2))
        v = _pdist_uniformity(a, b)
        v.backward()
        out[dt] = (v.item(), a.grad, b.grad)
    v32, v64 = out[torch.float32][0], out[torch.float64][0]
    g64 = out[torch.float64][1:]
    gerr = [((g32.double() - g).abs().max() / g.abs().max()).item() for g32, g in zip(out[torch.float32][1:], g64)]
    return z1, z2, v32, v64, g64, gerr


@pytest.mark.parametrize('base,family', LOSS_CASES, ids=[GE.case_tag(b, f) for b, f in LOSS_CASES])
def test_uniformity_loss_and_gradients_match_fp64(base, family):
    losses = importlib.import_module('3dinfomax_amd.losses')
    z1, z2, v32, v64, g64, gerr_ref = loss_case(base, family)
    a, b = (torch.from_numpy(z.copy()).to(DEV).requires_grad_(True) for z in (z1, z2))
    loss = losses.uniformity_loss(a, b)
    assert loss.dim() == 0 and loss.is_cuda
    loss.backward()
    tag, bad = 'uniformity_loss ' + GE.case_tag(base, family), []
    check_value(tag, 'uniformity', loss.item(), v64, abs(v32 - v64), bad)
    for which, got, want, ref_err in (('grad x1', a.grad, g64[0], gerr_ref[0]), ('grad x2', b.grad, g64[1], gerr_ref[1])):
        gmax = want.abs().max().item()
        gerr = (got.cpu().double() - want).abs().max().item() / gmax
        allowed = max(4 * ref_err, 16 * 2.0 ** -23)
        print(f'{tag} {which}: err / max {gerr:.3e} gerr_ref {ref_err:.3e} allowed {allowed:.3e} ratio {gerr / allowed:.3f}')
        if not gerr <= allowed:
            bad.append((which, gerr, allowed))
        assert torch.isfinite(got).all()
    assert not bad, (tag, bad)
