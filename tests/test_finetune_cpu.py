"""Fine-tuning losses and metrics on the host: the plugin surface, the CPU paths against the reference's own fp64 results (fixture:
tests/golden/gen_golden_finetune.py), the refusals that fire before any device work, exact zeros at unlabelled positions, the moments
cache, and the C ABI's argument checks."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from helpers import amd, load

import gen_golden_finetune as GF

launcher = importlib.import_module('launch_reference')
LOSSES = {'bce': 'OGBNanLabelBCEWithLogitsLoss', 'mse': 'OGBNanLabelMSELoss'}
METRIC_CLASSES = ('PearsonR', 'Rsquared', 'MAE', 'MeanPredictorLoss', 'QM9DenormalizedL1', 'QM9DenormalizedL2',
                  'QM9SingleTargetDenormalizedL1')
NAMES = tuple(LOSSES.values()) + METRIC_CLASSES


@functools.lru_cache(maxsize=None)
def loss_cases():
    return GF.loss_fixture(load('finetune.npz'))


@functools.lru_cache(maxsize=None)
def metric_cases():
    return GF.metric_fixture(load('finetune.npz'))


LOSS_IDS = [GF.loss_tag(*c) for c in GF.LOSS_CASES]
METRIC_IDS = [GF.metric_tag(*c) for c in GF.METRIC_CASES]


def metric_objects(case):
    """{fixture name: metric object} of one fixture case, built as the trainer builds them"""
    objs = {'pearsonr': amd.PearsonR(), 'rsquared': amd.Rsquared(), 'mae': amd.MAE(),
            'mean_predictor_l1': amd.MeanPredictorLoss(torch.nn.L1Loss()), 'mean_predictor_mse': amd.MeanPredictorLoss(torch.nn.MSELoss())}
    ds = case['dataset']
    if ds is not None:
        objs.update({'qm9_l1': amd.QM9DenormalizedL1(ds), 'qm9_l2': amd.QM9DenormalizedL2(ds)})
        if 'qm9_single' in case['values']:
            objs['qm9_single'] = amd.QM9SingleTargetDenormalizedL1(ds, GF.task_names(case['T'])[GF.SINGLE_TASK % case['T']])
    assert set(objs) == set(case['values']), (sorted(objs), sorted(case['values']))
    return objs


def test_names_resolve_from_the_package_the_alias_and_the_launcher():
    alias = importlib.import_module('infomax3d_amd')
    losses = importlib.import_module('3dinfomax_amd.losses')
    task_metrics = importlib.import_module('3dinfomax_amd.task_metrics')
    names = launcher.plugin_names()
    for name in NAMES:
        home = losses if name in LOSSES.values() else task_metrics
        assert name in amd.__all__ and name in alias.__all__, name
        assert getattr(amd, name) is getattr(alias, name) is getattr(home, name) is names[name], name


def test_fixture_covers_what_it_has_to():
    assert {c['B'] for c in loss_cases()} >= {1, 2, 63, 64, 65, 257, 1000} and {c['T'] for c in loss_cases()} == {1, 3, 12, 65, 130}
    assert {c['T'] for c in metric_cases()} >= {1, 3, 12, 65, 130, 300} and {c['B'] for c in metric_cases()} >= {1, 2, 63, 64, 65, 257, 1000}
    for c in loss_cases():
        unl = np.isnan(c['target'])
        assert np.isfinite(c['pred'][~unl]).all()
        if c['labels'] == 'wild':
            assert unl.any() and not np.isfinite(c['pred'][unl]).any()
        if c['labels'] == 'column':
            assert unl.all(axis=0).any()
        if c['labels'] == 1.0:
            assert unl.all()
    assert any(np.abs(c['pred'][np.isfinite(c['pred'])]).max() == 40.0 for c in loss_cases())
    twelve = [c for c in metric_cases() if c['dataset'] is not None and hasattr(c['dataset'], 'eV2meV') and c['T'] == 12]
    one = [c for c in metric_cases() if c['dataset'] is not None and hasattr(c['dataset'], 'eV2meV') and c['T'] == 1]
    assert twelve and one and all(c['reference_raises'] == 1 for c in twelve) and all(c['reference_raises'] == 0 for c in one)
    assert one[0]['dataset'].eV2meV.tolist() == [1000.0]


@pytest.mark.parametrize('kind', GF.KINDS)
@pytest.mark.parametrize('idx', range(len(GF.LOSS_CASES)), ids=LOSS_IDS)
def test_cpu_loss_matches_the_reference_in_fp64(idx, kind):
    c = loss_cases()[idx]
    pred = torch.from_numpy(c['pred']).double().requires_grad_(True)
    target = torch.from_numpy(c['target']).double()
    loss = getattr(amd, LOSSES[kind])()(pred, target)
    assert loss.dim() == 0
    loss.backward()
    ref, gref = float(c[kind]['loss64']), torch.from_numpy(c[kind]['grad64'])
    if c['labels'] == 1.0:
        assert math.isnan(loss.item()) and math.isnan(ref)
    else:
        assert abs(loss.item() - ref) <= 1e-10 * max(1.0, abs(ref))
    assert (pred.grad - gref).abs().max().item() <= 1e-10 * max(1.0, gref.abs().max().item())
    unl = torch.isnan(target)
    assert (pred.grad[unl] == 0).all() and not torch.isnan(pred.grad).any()          # exactly zero, also under a NaN / inf prediction


def test_one_dimensional_input_is_a_single_task():
    c = loss_cases()[LOSS_IDS.index('64x1_nan0')]
    pred, target = torch.from_numpy(c['pred']).double(), torch.from_numpy(c['target']).double()
    for kind in GF.KINDS:
        loss = getattr(amd, LOSSES[kind])()
        assert loss(pred.reshape(-1), target.reshape(-1)).item() == loss(pred, target).item()
        assert loss(pred, target, some_batch_key=None).item() == loss(pred, target).item()      # **kwargs, as the reference's signature


class _PretendsToBeOnTheDevice(torch.Tensor):
    is_cuda = property(lambda self: True)


def _no_library(monkeypatch):
    ops = importlib.import_module('3dinfomax_amd.ops')
    L = importlib.import_module('3dinfomax_amd._lib')

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_library)
    monkeypatch.setattr(ops._lib, 'load', no_library)


def test_refusals_fire_before_any_device_work(monkeypatch):
    _no_library(monkeypatch)
    for name in LOSSES.values():
        loss = getattr(amd, name)()
        with pytest.raises(ValueError, match='same shape'):
            loss(torch.zeros(4, 3), torch.zeros(4, 2))
        with pytest.raises(ValueError, match='same shape'):
            loss(torch.zeros(4, 1), torch.zeros(4))
        with pytest.raises(ValueError, match='same shape'):
            loss(torch.zeros(4, 3), [[0.0] * 3] * 4)
        with pytest.raises(ValueError, match='batch'):
            loss(torch.zeros(2, 2, 2), torch.zeros(2, 2, 2))
        with pytest.raises(ValueError, match='at least one'):
            loss(torch.zeros(0, 3), torch.zeros(0, 3))
        for dtype in (torch.float64, torch.bfloat16, torch.float16):
            a = torch.zeros(4, 3, dtype=dtype).as_subclass(_PretendsToBeOnTheDevice)
            b = torch.zeros(4, 3, dtype=dtype).as_subclass(_PretendsToBeOnTheDevice)
            assert a.is_cuda
            with pytest.raises(NotImplementedError, match='fp32'):
                loss(a, b)
        a = torch.zeros(4, 3).as_subclass(_PretendsToBeOnTheDevice)
        with pytest.raises(NotImplementedError, match='fp32'):
            loss(a, torch.zeros(4, 3, dtype=torch.float64).as_subclass(_PretendsToBeOnTheDevice))
        assert not hasattr(loss, 'attach_group')
    with pytest.raises(ValueError, match='same shape'):
        amd.MAE()(torch.zeros(4, 3), torch.zeros(4, 2))


@pytest.mark.parametrize('idx', range(len(GF.METRIC_CASES)), ids=METRIC_IDS)
def test_cpu_metrics_match_the_reference_in_fp64(idx):
    c = metric_cases()[idx]
    pred, target = torch.from_numpy(c['pred']).double(), torch.from_numpy(c['target']).double()
    for name, obj in metric_objects(c).items():
        got = obj(pred, target)
        assert got.dim() == 0 and not got.is_cuda
        _, v64, class_only = c['values'][name]
        if not math.isfinite(v64):
            assert GF.value_class(got.item()) == GF.value_class(v64), (name, got.item(), v64)
            continue
        exact = obj.value(pred, target)               # the fp64 number; forward() hands it back as an fp32 tensor, as the device path does
        assert abs(exact - v64) <= 1e-10 * max(1.0, abs(v64)), (name, exact, v64)
        assert got.dtype == torch.float32 and got.item() == np.float32(exact)


def _counted(monkeypatch, attr):
    tm = importlib.import_module('3dinfomax_amd.task_metrics')
    calls = []
    inner = getattr(tm, attr)

    def wrapper(p, t):
        calls.append(tuple(p.shape))
        return inner(p, t)
    monkeypatch.setattr(tm, attr, wrapper)
    return calls


def check_one_moments_call_per_pair(calls, case, to_tensor):
    """shared with the device test: N metric objects on one pair cost one moments call; a new tensor object, or an in-place change,
    costs another"""
    objs = metric_objects(case)
    pred, target = to_tensor(case['pred']), to_tensor(case['target'])
    first = {k: o(pred, target).item() for k, o in objs.items()}
    assert len(objs) >= 5 and len(calls) == 1, calls
    again = {k: o(pred, target).item() for k, o in objs.items()}
    assert len(calls) == 1 and all(first[k] == again[k] or (math.isnan(first[k]) and math.isnan(again[k])) for k in first)
    pred2 = to_tensor(case['pred'])                  # same shape, same values, another object
    objs['mae'](pred2, target)
    assert len(calls) == 2
    objs['pearsonr'](pred2, target)
    assert len(calls) == 2
    before = objs['mae'](pred2, target).item()
    pred2.add_(1.0)                                  # the version counter moves
    after = objs['mae'](pred2, target).item()
    assert len(calls) == 3 and after != before
    del pred2
    pred3 = to_tensor(case['pred'])                  # very likely the address the dead tensor had: a dead weak reference never matches
    assert objs['mae'](pred3, target).item() == first['mae'] and len(calls) == 4


def test_metric_objects_share_one_moments_call(monkeypatch):
    calls = _counted(monkeypatch, '_moments_host')
    case = metric_cases()[METRIC_IDS.index('63x12_plain_qm9')]
    check_one_moments_call_per_pair(calls, case, lambda a: torch.from_numpy(a.copy()).double())


def test_mean_predictor_loss_calls_an_unknown_loss_func(monkeypatch):
    calls = _counted(monkeypatch, '_moments_host')
    c = metric_cases()[METRIC_IDS.index('65x12_plain')]
    pred, target = torch.from_numpy(c['pred']).double(), torch.from_numpy(c['target']).double()
    seen = []

    def huber(a, b):
        seen.append((a, b))
        return torch.nn.functional.smooth_l1_loss(a, b)
    got = amd.MeanPredictorLoss(huber)(pred, target)
    assert len(seen) == 1 and not calls
    with pytest.raises(NotImplementedError, match='loss_func'):
        amd.MeanPredictorLoss(huber).value(pred, target)
    assert seen[0][1] is target and torch.equal(seen[0][0], torch.full_like(target, target.mean()))
    assert got.item() == torch.nn.functional.smooth_l1_loss(torch.full_like(target, target.mean()), target).item()
    # a non-default reduction is not the table's mean either
    got = amd.MeanPredictorLoss(torch.nn.L1Loss(reduction='sum'))(pred, target)
    assert not calls and got.item() == (target - target.mean()).abs().sum().item()


def test_the_factor_applies_whenever_the_dataset_has_one():
    """the reference raises on `if eV2meV:` for twelve tasks (recorded in the fixture); here the factor applies, column by column"""
    c = metric_cases()[METRIC_IDS.index('63x12_plain_qm9')]
    pred, target = torch.from_numpy(c['pred']).double(), torch.from_numpy(c['target']).double()
    ds = c['dataset']
    plain = GF.StandInDataset(ds.targets_mean, ds.targets_std)
    scale = ds.targets_std.double() * ds.eV2meV.double()
    want = ((pred - target).abs() * scale).mean().item()
    assert abs(amd.QM9DenormalizedL1(ds)(pred, target).item() - want) <= 1e-6 * want
    assert amd.QM9DenormalizedL1(plain)(pred, target).item() < 0.1 * want            # no eV2meV attribute: no factor
    with pytest.raises(ValueError, match='task columns'):
        amd.QM9DenormalizedL1(ds)(pred[:, :5].contiguous(), target[:, :5].contiguous())
    with pytest.raises(ValueError):
        amd.QM9SingleTargetDenormalizedL1(ds, 'no_such_task')


def test_header_declares_the_kernels_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    L = importlib.import_module('3dinfomax_amd._lib')
    lib = L.load()
    declared = L.declared_symbols()
    for name in ('i3d_masked_loss_partial_floats', 'i3d_masked_loss_fwd', 'i3d_masked_loss_bwd', 'i3d_task_moments_partial_floats',
                 'i3d_task_moments'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.i3d_abi_version() == 2
    # argument validation happens on the host before any launch: no GPU needed
    assert lib.i3d_masked_loss_fwd(None, None, 0, 3, 0, None, None, None) == -1 and b'rows' in lib.i3d_last_error()
    assert lib.i3d_masked_loss_fwd(None, None, 4, 0, 0, None, None, None) == -1 and b'tasks' in lib.i3d_last_error()
    assert lib.i3d_masked_loss_fwd(None, None, 4, 3, 2, None, None, None) == -1 and b'kind' in lib.i3d_last_error()
    assert lib.i3d_masked_loss_fwd(None, None, 4, 3, 1, None, None, None) == -1 and b'null' in lib.i3d_last_error()
    assert lib.i3d_masked_loss_bwd(None, None, 4, 3, -1, None, None, None, None) == -1 and b'kind' in lib.i3d_last_error()
    assert lib.i3d_masked_loss_bwd(None, None, 4, 3, 0, None, None, None, None) == -1 and b'null' in lib.i3d_last_error()
    assert lib.i3d_task_moments(None, None, 0, 1, None, None, None) == -1 and b'rows' in lib.i3d_last_error()
    assert lib.i3d_task_moments(None, None, 1, 1, None, None, None) == -1 and b'null' in lib.i3d_last_error()
    assert lib.i3d_masked_loss_partial_floats(0, 3) == 0 and lib.i3d_task_moments_partial_floats(3, 0) == 0
    # {sum, count} per workgroup of 512 elements; seven sums per (row block, column)
    assert lib.i3d_masked_loss_partial_floats(128, 1) == 4 and lib.i3d_masked_loss_partial_floats(257, 3) == 8
    assert lib.i3d_task_moments_partial_floats(128, 1) == 14 and lib.i3d_task_moments_partial_floats(1000, 1) == 28
    assert lib.i3d_task_moments_partial_floats(5, 300) == 14 * 3 * 300
