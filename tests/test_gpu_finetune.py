"""Fine-tuning losses and metrics on the MI355X (csrc/task.hip) against the reference's fp64 results (fixture:
tests/golden/gen_golden_finetune.py; shapes from the fixture only).

Values (the loss, every metric): |ours - fp64| <= max(2 |reference fp32 - fp64|, 4 ulp of fp32 at the value's magnitude).  The kernels
accumulate in fp64, so they should land well inside the reference's own fp32 error; the floor covers the cases where the reference
happens to be exact.  Gradients: elementwise against the fp64 gradient within 8 ulp of fp32 relative to max |grad| (one rounding of an
fp64 value to fp32 is half an ulp; the rest is room for the device's exp), and bit-zero where unlabelled.  Every check prints its
figures before it asserts; the table of DESIGN.md ('Fine-tuning losses and metrics') is where they go."""
import importlib
import math

import numpy as np
import pytest
import torch

from helpers import PNA_SMALL, amd, grads_close, synth

import gen_golden_finetune as GF
from test_finetune_cpu import (LOSS_IDS, LOSSES, METRIC_IDS, _counted, check_one_moments_call_per_pair, loss_cases, metric_cases,
                               metric_objects)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ULP = 2.0 ** -23


def ulp32(v):
    """one ulp of fp32 at the magnitude of v (the smallest normal's below that)"""
    v = abs(float(v))
    return ULP * 2.0 ** math.floor(math.log2(v)) if v >= 2.0 ** -126 else 2.0 ** -149


def _run(kind, c):
    pred = torch.from_numpy(c['pred']).to(DEV).requires_grad_(True)
    target = torch.from_numpy(c['target']).to(DEV)
    loss = getattr(amd, LOSSES[kind])()(pred, target)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    return loss.detach().cpu(), pred.grad.cpu()


@pytest.mark.parametrize('kind', GF.KINDS)
@pytest.mark.parametrize('idx', range(len(GF.LOSS_CASES)), ids=LOSS_IDS)
def test_loss_and_gradient_match_the_reference(idx, kind):
    c = loss_cases()[idx]
    ref = c[kind]
    loss, grad = _run(kind, c)
    g64 = torch.from_numpy(ref['grad64'])
    unl = torch.isnan(torch.from_numpy(c['target']))
    gmax = g64.abs().max().item()
    gerr = (grad.double() - g64).abs().max().item()
    if c['labels'] == 1.0:          # no label at all - an ordinary batch of these datasets: NaN loss, the fixture's (zero) gradient
        print(f'{c["tag"]} {kind}: loss {loss.item()} (reference {ref["loss64"]}), gradient error {gerr:.3e}')
        assert math.isnan(loss.item()) and math.isnan(ref['loss64'])
        assert gmax == 0.0 and torch.equal(grad, torch.zeros_like(grad))
        return
    err, err_ref = abs(loss.item() - ref['loss64']), abs(ref['loss32'] - ref['loss64'])
    allowed = max(2 * err_ref, 4 * ulp32(ref['loss64']))
    print(f'{c["tag"]} {kind}: loss err {err:.3e} reference fp32 {err_ref:.3e} allowed {allowed:.3e} ratio {err / allowed:.3f}; '
          f'gradient err / max {gerr / gmax:.3e} (reference fp32 {ref["gerr32"]:.3e}, allowed {8 * ULP:.3e})')
    assert err <= allowed
    assert gerr <= 8 * ULP * gmax
    assert torch.equal(grad[unl], torch.zeros_like(grad[unl])) and not torch.signbit(grad[unl]).any()
    assert torch.isfinite(grad).all()


@pytest.mark.parametrize('idx', range(len(GF.METRIC_CASES)), ids=METRIC_IDS)
def test_metrics_match_the_reference(idx):
    c = metric_cases()[idx]
    pred, target = torch.from_numpy(c['pred']).to(DEV), torch.from_numpy(c['target']).to(DEV)
    bad = []
    for name, obj in metric_objects(c).items():
        got = obj(pred, target)
        assert got.dim() == 0 and not got.is_cuda
        v32, v64, class_only = c['values'][name]
        if class_only:
            print(f'{c["tag"]} {name}: {got.item()} (reference {v64}): class only')
            assert GF.value_class(got.item()) == GF.value_class(v64)
            continue
        err, err_ref = abs(got.item() - v64), abs(v32 - v64)
        allowed = max(2 * err_ref, 4 * ulp32(v64))
        print(f'{c["tag"]} {name}: err {err:.3e} reference fp32 {err_ref:.3e} allowed {allowed:.3e} ratio {err / allowed:.3f}')
        if not err <= allowed:
            bad.append((name, got.item(), v64, err, allowed))
    assert not bad, bad


def test_two_runs_are_bit_identical():
    for tag in ('257x3_nan30', '63x12_column'):
        c = loss_cases()[LOSS_IDS.index(tag)]
        for kind in GF.KINDS:
            (l1, g1), (l2, g2) = _run(kind, c), _run(kind, c)
            assert l1.view(torch.int32).item() == l2.view(torch.int32).item() and torch.equal(g1, g2)
    ops = importlib.import_module('3dinfomax_amd.ops')
    for tag in ('1000x1_plain', '65x12_plain', '5x300_plain'):
        c = metric_cases()[METRIC_IDS.index(tag)]
        pred, target = torch.from_numpy(c['pred']).to(DEV), torch.from_numpy(c['target']).to(DEV)
        a, b = ops.task_moments(pred, target).cpu(), ops.task_moments(pred, target).cpu()
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_upstream_gradient_is_read_on_the_device():
    c = loss_cases()[LOSS_IDS.index('65x3_nan30')]
    pred = torch.from_numpy(c['pred']).to(DEV).requires_grad_(True)
    target = torch.from_numpy(c['target']).to(DEV)
    (amd.OGBNanLabelMSELoss()(pred, target) * 0.25).backward()
    g64 = torch.from_numpy(c['mse']['grad64']) * 0.25
    assert (pred.grad.cpu().double() - g64).abs().max().item() <= 8 * ULP * g64.abs().max().item()


def test_pna_under_the_masked_loss_end_to_end():
    """a small PNA with three task outputs under OGBNanLabelBCEWithLogitsLoss against the same model under the torch expression of the
    loss; the bound of the PNA fixture tests (grads_close 5e-4)"""
    losses = importlib.import_module('3dinfomax_amd.losses')
    mols = synth.make_dataset(8, seed=5)
    torch.manual_seed(0)
    pna = amd.PNA(**dict(PNA_SMALL, target_dim=3, hidden_dim=16, propagation_depth=2))
    with torch.no_grad():
        for n, p in pna.named_parameters():
            if n.endswith('linear.weight'):
                p.mul_(p.shape[1] * 0.7)
    pna.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    target = (torch.rand(8, 3, generator=g) < 0.5).float()
    target[torch.rand(8, 3, generator=g) < 0.3] = float('nan')
    target[0, 0], target[1, 1] = 1.0, float('nan')
    target = target.to(DEV)

    def grads(loss_of):
        pna.zero_grad(set_to_none=True)
        g2 = amd.batch([amd.bond_graph(m) for m in mols]).to(DEV)
        out = pna(g2)
        assert tuple(out.shape) == (8, 3)
        loss = loss_of(out)
        loss.backward()
        return loss.item(), {k: p.grad.detach().cpu().clone() for k, p in pna.named_parameters() if p.grad is not None}

    ours, got = grads(lambda out: amd.OGBNanLabelBCEWithLogitsLoss()(out, target))
    want, ref = grads(lambda out: losses._masked_loss_host(out, target, 0))
    print(f'e2e loss {ours:.7f} torch expression {want:.7f}')
    assert abs(ours - want) <= 1e-5 * abs(want) and set(got) == set(ref)
    grads_close(got, ref, 5e-4, what='e2e: ')


def test_metric_objects_on_device_tensors_share_one_moments_call(monkeypatch):
    calls = _counted(monkeypatch, '_moments_device')
    case = metric_cases()[METRIC_IDS.index('63x12_plain_qm9')]
    check_one_moments_call_per_pair(calls, case, lambda a: torch.from_numpy(a.copy()).to(DEV))
