"""Fixture of the fine-tuning losses (reference commons/losses.py:13-31: OGBNanLabelBCEWithLogitsLoss, OGBNanLabelMSELoss) and metrics
(reference trainer/metrics.py:15-158: PearsonR, Rsquared, MAE, MeanPredictorLoss, QM9DenormalizedL1 / L2, QM9SingleTargetDenormalizedL1):
the unmodified reference classes on seeded inputs -> tests/golden/finetune.npz.

    python tests/golden/gen_golden_finetune.py          (imports the reference checkout, as gen_golden.py does)

The arrays of all cases are stored back to back (a zip member per case and quantity would cost more than the data); loss_fixture() and
metric_fixture() below cut them apart again.

Losses ('loss/pred', 'loss/target' fp32; per kind 'loss/<bce|mse>_grad64'; 'loss/scalars' [case, kind, (loss32, loss64, gerr32)]): the
reference's loss in fp32 and in fp64 on the same inputs, its fp64 gradient of pred, and the error of its own fp32 gradient relative to
max |grad64|.  Inputs are quantised (pred and the metric inputs to 1/16, loss targets to 1/16 in [0, 1] - soft labels, valid for both
kinds) so that the file stays small; a few logits sit at +-40.  Cases: LOSS_CASES below.

Metrics ('metric/pred', 'metric/target' fp32; 'metric/values' [case, metric, (v32, v64, class_only)], metrics in the order of
METRIC_NAMES, class_only = -1: not computed for this case): the reference's value on the fp32 tensors and on their fp64 copies.
class_only = 1: the reference's own fp32 result is not finite or misses its fp64
result by more than 1e-3 relative (or the fp64 result is not finite) - such a value has no tolerance, a test compares its class
(finite / +inf / -inf / nan) only.  Datasets are small stand-in objects ('metric/ds': mean | std [| eV2meV] per case with a dataset): 'plain' has no
eV2meV (the GEOM-Drugs branch of the reference's constructors), 'qm9' has one.  The reference's denormalize() tests `if eV2meV:` on the
tensor: with one task that is the truth of its single element, with twelve it RAISES ('metric/reference_raises' [case] = 1, recorded
from the unmodified class).  The expected values of the twelve-task qm9 case are then the reference's own results column by column:
each column run through the unmodified classes as a one-task dataset (mean, std, factor of that column), L1 / L2 averaged over the
equally long columns.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

KINDS = ('bce', 'mse')
# (B, T, labels): labels = fraction of NaN targets, or 'column' (30 % + one fully unlabelled column), or 'wild' (30 % + NaN / inf in pred
# at unlabelled positions only).  Every B of {1, 2, 63, 64, 65, 257, 1000} and every T of {1, 3, 12, 65, 130}; 63 x 12, 257 x 3 and
# 1000 x 1 (more than 512 elements) take the forward's two-launch form, the others the one-launch form.
LOSS_CASES = [(1, 1, 0.0), (2, 3, 0.3), (63, 12, 'column'), (64, 1, 0.0), (65, 3, 0.3), (65, 3, 1.0), (65, 3, 'wild'),
              (257, 3, 0.3), (1000, 1, 0.3), (2, 65, 0.3), (3, 130, 0.3)]
# (B, T, content, dataset): content 'plain', 'offset' (column 0: targets of mean 50 and std 0.01), 'const' (every target 2.0).  The
# thread maps of the moments kernel: T <= 128 packed rows (1, 3, 12, 65), 129..256 one row per iteration (130), above 256 column
# tiles (300).  One row block: 1 x 1, 64 x 1, 2 x 3, 65 x 3, 64 x 3, 2 x 65; several: 1000 x 1, 257 x 3, 63 x 12, 65 x 12, 5 x 130, 5 x 300.
METRIC_CASES = [(1, 1, 'plain', None), (2, 3, 'plain', 'plain'), (63, 12, 'plain', 'qm9'), (63, 12, 'offset', 'plain'),
                (64, 1, 'plain', 'qm9'), (65, 3, 'offset', None), (257, 3, 'plain', None), (1000, 1, 'plain', None),
                (65, 12, 'plain', None), (2, 65, 'plain', None), (5, 130, 'plain', 'plain'), (5, 300, 'plain', None),
                (64, 3, 'const', None)]
METRICS = ('pearsonr', 'rsquared', 'mae', 'mean_predictor_l1', 'mean_predictor_mse')
DATASET_METRICS = ('qm9_l1', 'qm9_l2', 'qm9_single')
METRIC_NAMES = METRICS + DATASET_METRICS
SINGLE_TASK = 3              # the column QM9SingleTargetDenormalizedL1 is asked about (modulo T)


def loss_tag(B, T, labels):
    return f'{B}x{T}_' + (labels if isinstance(labels, str) else f'nan{int(round(100 * labels))}')


def metric_tag(B, T, content, dataset):
    return f'{B}x{T}_{content}' + (f'_{dataset}' if dataset else '')


def task_names(T):
    return [f'task{c}' for c in range(T)]


class StandInDataset:
    """what the metric constructors read: targets_mean, targets_std, target_tasks and, for the QM9 kind, eV2meV"""

    def __init__(self, mean, std, ev=None):
        self.targets_mean, self.targets_std = torch.as_tensor(mean), torch.as_tensor(std)
        self.target_tasks = task_names(self.targets_mean.shape[0])
        if ev is not None:
            self.eV2meV = torch.as_tensor(ev)


def loss_fixture(z):
    """-> per case {tag, B, T, labels, pred, target, 'bce' / 'mse': {loss32, loss64, gerr32, grad64}}"""
    cases, o = [], 0
    for i, (B, T, labels) in enumerate(LOSS_CASES):
        n = B * T
        c = {'tag': loss_tag(B, T, labels), 'B': B, 'T': T, 'labels': labels, 'pred': z['loss/pred'][o:o + n].reshape(B, T),
             'target': z['loss/target'][o:o + n].reshape(B, T)}
        for k, kind in enumerate(KINDS):
            l32, l64, gerr = z['loss/scalars'][i, k]
            c[kind] = {'loss32': l32, 'loss64': l64, 'gerr32': gerr, 'grad64': z[f'loss/{kind}_grad64'][o:o + n].reshape(B, T)}
        cases.append(c)
        o += n
    return cases


def metric_fixture(z):
    """-> per case {tag, B, T, content, pred, target, dataset (or None), reference_raises, values {name: (v32, v64, class_only)}}"""
    cases, o, d = [], 0, 0
    for i, (B, T, content, dsk) in enumerate(METRIC_CASES):
        n = B * T
        c = {'tag': metric_tag(B, T, content, dsk), 'B': B, 'T': T, 'content': content, 'dataset': None,
             'pred': z['metric/pred'][o:o + n].reshape(B, T), 'target': z['metric/target'][o:o + n].reshape(B, T),
             'reference_raises': int(z['metric/reference_raises'][i]),
             'values': {name: tuple(z['metric/values'][i, m]) for m, name in enumerate(METRIC_NAMES) if z['metric/values'][i, m, 2] >= 0}}
        if dsk:
            w = 3 if dsk == 'qm9' else 2
            ds = z['metric/ds'][d:d + w * T].reshape(w, T)
            c['dataset'] = StandInDataset(ds[0].copy(), ds[1].copy(), ds[2].copy() if w == 3 else None)
            d += w * T
        cases.append(c)
        o += n
    return cases


def value_class(v):
    v = float(v)
    return 'nan' if np.isnan(v) else ('+inf' if v == np.inf else ('-inf' if v == -np.inf else 'finite'))


def loss_inputs(B, T, labels):
    g = torch.Generator().manual_seed(7000 * B + 10 * T + (sum(map(ord, labels)) if isinstance(labels, str) else int(100 * labels)))
    pred = torch.round(3.0 * torch.randn(B, T, generator=g) * 16) / 16
    n = B * T
    flat = pred.reshape(-1)
    flat[torch.randperm(n, generator=g)[:n // 16]] = 40.0          # the stable form of the BCE matters out here
    flat[torch.randperm(n, generator=g)[:n // 16]] = -40.0
    target = torch.randint(0, 17, (B, T), generator=g).float() / 16
    frac = 0.3 if isinstance(labels, str) else labels
    unl = torch.rand(B, T, generator=g) < frac if frac < 1.0 else torch.ones(B, T, dtype=torch.bool)
    if labels == 'column':
        unl[:, T // 2] = True
    target[unl] = float('nan')
    if labels == 'wild':
        wild = torch.tensor([float('nan'), float('inf'), -float('inf')])
        pred[unl] = wild[torch.randint(0, 3, (int(unl.sum()),), generator=g)]
    return pred.contiguous(), target.contiguous()


def metric_inputs(B, T, content):
    g = torch.Generator().manual_seed(9000 * B + 10 * T + sum(map(ord, content)))
    target = torch.round(torch.randn(B, T, generator=g) * 16) / 16
    pred = target + torch.round(0.3 * torch.randn(B, T, generator=g) * 16) / 16
    if content == 'offset':
        target[:, 0] = 50.0 + 0.01 * torch.randn(B, generator=g)
        pred[:, 0] = target[:, 0] + 0.003 * torch.randn(B, generator=g)
    if content == 'const':
        target[:] = 2.0
    return pred.contiguous(), target.contiguous()


def dataset_arrays(T, kind):
    g = torch.Generator().manual_seed(31 * T + len(kind))
    mean = torch.round(torch.randn(T, generator=g) * 8) / 8
    std = 0.25 + torch.randint(0, 16, (T,), generator=g).float() / 8
    out = {'ds_mean': mean.numpy(), 'ds_std': std.numpy()}
    if kind == 'qm9':
        out['ds_ev'] = np.where(np.arange(T) % 3 == 1, 1.0, 1000.0).astype(np.float32) if T > 1 else np.array([1000.0], np.float32)
    return out


def import_reference():
    import gen_golden as G
    G.import_reference()
    qm9 = types.ModuleType('datasets.qm9_dataset')

    class QM9Dataset(StandInDataset):          # QM9DenormalizedL1 / L2 read eV2meV from instances of this class only
        pass
    qm9.QM9Dataset = QM9Dataset
    for name, attrs in (('ogb', ()), ('ogb.graphproppred', ('Evaluator',)), ('ogb.lsc', ('PCQM4MEvaluator',)),
                        ('datasets.geom_drugs_dataset', ('GEOMDrugs',))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, object)
        sys.modules[name] = m
    pkg = types.ModuleType('datasets')
    pkg.__path__ = [os.path.join(G.REF, 'datasets')]
    sys.modules['datasets'] = pkg
    sys.modules['datasets.qm9_dataset'] = qm9
    import commons.losses as ref_losses
    import trainer.metrics as M
    return ref_losses, M, QM9Dataset


def main():
    ref_losses, M, QM9Dataset = import_reference()
    loss_cls = {'bce': ref_losses.OGBNanLabelBCEWithLogitsLoss, 'mse': ref_losses.OGBNanLabelMSELoss}
    out = {}
    flat = {k: [] for k in ('loss/pred', 'loss/target', 'loss/bce_grad64', 'loss/mse_grad64', 'metric/pred', 'metric/target', 'metric/ds')}
    loss_scalars = np.zeros((len(LOSS_CASES), len(KINDS), 3))
    metric_values = np.full((len(METRIC_CASES), len(METRIC_NAMES), 3), -1.0)
    raised = np.zeros(len(METRIC_CASES), np.int64)

    def run_loss(kind, pred, target, dtype):
        p = pred.to(dtype).clone().requires_grad_(True)
        loss = loss_cls[kind]()(p, target.to(dtype))
        loss.backward()
        return loss.detach().numpy().copy(), p.grad.numpy().copy()

    for i, (B, T, labels) in enumerate(LOSS_CASES):
        pred, target = loss_inputs(B, T, labels)
        tag = loss_tag(B, T, labels)
        flat['loss/pred'].append(pred.numpy().ravel())
        flat['loss/target'].append(target.numpy().ravel())
        for k, kind in enumerate(KINDS):
            l32, g32 = run_loss(kind, pred, target, torch.float32)
            l64, g64 = run_loss(kind, pred, target, torch.float64)
            gmax = max(np.abs(g64).max(), 1e-300)
            gerr = float(np.abs(g32.astype(np.float64) - g64).max() / gmax)
            p = f'loss/{tag}/{kind}/'
            loss_scalars[i, k] = (float(l32), float(l64), gerr)
            flat[f'loss/{kind}_grad64'].append(g64.ravel())
            if labels == 1.0:
                assert np.isnan(l32) and np.isnan(l64) and not g64.any() and not g32.any(), tag      # NaN loss, zero gradient
            else:
                rel = abs(float(l32) - float(l64)) / abs(float(l64))
                assert np.isfinite(l32) and rel <= 1e-3, (tag, kind, rel)
                assert not g64[np.isnan(target.numpy())].any()
                print(f'{p} loss {float(l64):.6f} fp32 against fp64: loss {rel:.2e} grad {gerr:.2e}')

    def metric_objects(ds, T):
        objs = {'pearsonr': M.PearsonR(), 'rsquared': M.Rsquared(), 'mae': M.MAE(),
                'mean_predictor_l1': M.MeanPredictorLoss(torch.nn.L1Loss()), 'mean_predictor_mse': M.MeanPredictorLoss(torch.nn.MSELoss())}
        if ds is not None:
            objs.update({'qm9_l1': M.QM9DenormalizedL1(ds), 'qm9_l2': M.QM9DenormalizedL2(ds)})
            if hasattr(ds, 'eV2meV'):          # the reference's single-target class reads it unconditionally
                objs['qm9_single'] = M.QM9SingleTargetDenormalizedL1(ds, task_names(T)[SINGLE_TASK % T])
        return objs

    def by_column(name, arrays, pred, target, T):
        """the reference's own result column by column, each column a one-task QM9 dataset"""
        cols = [SINGLE_TASK % T] if name == 'qm9_single' else range(T)
        vals = []
        for c in cols:
            ds = QM9Dataset(arrays['ds_mean'][c:c + 1], arrays['ds_std'][c:c + 1], arrays['ds_ev'][c:c + 1])
            obj = {'qm9_l1': M.QM9DenormalizedL1, 'qm9_l2': M.QM9DenormalizedL2}.get(name)
            obj = obj(ds) if obj else M.QM9SingleTargetDenormalizedL1(ds, 'task0')
            vals.append(obj(pred[:, c:c + 1], target[:, c:c + 1]))
        return torch.stack(vals).mean()

    for i, (B, T, content, dsk) in enumerate(METRIC_CASES):
        pred, target = metric_inputs(B, T, content)
        tag = metric_tag(B, T, content, dsk)
        p = f'metric/{tag}/'
        flat['metric/pred'].append(pred.numpy().ravel())
        flat['metric/target'].append(target.numpy().ravel())
        ds, arrays = None, None
        if dsk:
            arrays = dataset_arrays(T, dsk)
            flat['metric/ds'] += [arrays[k] for k in ('ds_mean', 'ds_std', 'ds_ev') if k in arrays]
            ds = (QM9Dataset if dsk == 'qm9' else StandInDataset)(arrays['ds_mean'], arrays['ds_std'], arrays.get('ds_ev'))
        raises = 0
        for name, obj in metric_objects(ds, T).items():
            vals = []
            for dtype in (torch.float32, torch.float64):
                a, b = pred.to(dtype), target.to(dtype)
                try:
                    v = obj(a, b)
                except RuntimeError as e:          # `if eV2meV:` on a tensor of more than one element
                    assert 'mbiguous' in str(e) and dsk == 'qm9' and T > 1, (tag, name, e)
                    raises = 1
                    v = by_column(name, arrays, a, b, T)
                vals.append(float(v))
            v32, v64 = vals
            class_only = int(not (np.isfinite(v32) and np.isfinite(v64) and abs(v32 - v64) <= 1e-3 * abs(v64)))
            metric_values[i, METRIC_NAMES.index(name)] = (v32, v64, class_only)
            print(f'{p}{name}: fp64 {v64:.9g} fp32 {v32:.9g}' + (f' CLASS ONLY ({value_class(v64)})' if class_only else
                                                                f' rel {abs(v32 - v64) / max(abs(v64), 1e-300):.2e}'))
        raised[i] = raises
        assert raises == int(dsk == 'qm9' and T > 1), tag
    out = {k: np.concatenate(v) for k, v in flat.items()}
    out.update({'loss/scalars': loss_scalars, 'metric/values': metric_values, 'metric/reference_raises': raised})
    path = os.path.join(HERE, 'finetune.npz')
    np.savez_compressed(path, **out)
    print('wrote finetune.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 100 * 1024


if __name__ == '__main__':
    main()
