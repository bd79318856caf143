"""Fine-tuning metrics - drop-in for the classes of reference trainer/metrics.py:15-158 that configs_clean/tune_QM9_homo.yml and
configs_clean/tune_freesolv.yml list: PearsonR, Rsquared, MAE, MeanPredictorLoss, QM9DenormalizedL1, QM9DenormalizedL2 and
QM9SingleTargetDenormalizedL1.

The reference trainer calls every metric separately and `.item()`s each result (trainer/trainer.py:174-183), on every logged training
batch and every validation batch: with the 12 QM9 targets 15 chains of small device ops and 15 host synchronisations.  All of these
metrics are functions of one small table of per-task moments of (preds, targets) - include/infomax3d_hip.h: i3d_task_moments - so the
first metric asked about a (preds, targets) pair computes the table in one device pass (csrc/task.hip) and brings it to the host with
one copy; the other metric objects find it cached (a weak-reference cache of its own, keyed as the contrastive one of metrics.py).
Everything is derived from the table in numpy fp64; the value comes back as a 0-dim CPU tensor.  CPU tensors take the same derivation
from moments computed with torch in fp64 (the host-logic tests).
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .metrics import _cached, _fill, _tensor_key

N, SP, ST, SPP, STT, SPT, L1, L2, GL1, GL2 = range(10)        # columns of the table

_task_cache = {'key': None, 'values': None, 'x1': None, 'x2': None}


def _moments_host(p, t):
    """the table of i3d_task_moments from CPU tensors, in fp64"""
    p, t = p.double(), t.double()
    B, T = p.shape
    dp, dt, d, g = p - p.mean(dim=0), t - t.mean(dim=0), p - t, t - t.mean()
    cols = torch.stack([torch.full((T,), float(B), dtype=torch.float64), p.sum(0), t.sum(0), (dp * dp).sum(0), (dt * dt).sum(0),
                        (dp * dt).sum(0), d.abs().sum(0), (d * d).sum(0), g.abs().sum(0), (g * g).sum(0)], dim=1)
    return torch.cat([cols, cols.sum(dim=0, keepdim=True)]).numpy()


def _moments_device(p, t):
    """one device pass, one device-to-host copy"""
    return ops.task_moments(p, t).cpu().numpy()


def task_moments(preds, targets):
    """table [T + 1, 10] (numpy fp64) of a (preds, targets) pair, computed once per pair of tensor objects and versions"""
    if not (torch.is_tensor(preds) and torch.is_tensor(targets)) or tuple(preds.shape) != tuple(targets.shape) \
            or preds.dim() not in (1, 2) or preds.numel() == 0:
        raise ValueError('preds and targets of the same shape [batch, tasks] (or [batch]) expected, got '
                         f'{tuple(preds.shape) if torch.is_tensor(preds) else type(preds).__name__} and '
                         f'{tuple(targets.shape) if torch.is_tensor(targets) else type(targets).__name__}')
    if preds.is_cuda != targets.is_cuda:
        raise ValueError(f'preds is on {preds.device}, targets on {targets.device}')
    key = _tensor_key(preds, targets)
    table = _cached(_task_cache, key, preds, targets)
    if table is not None:
        return table
    with torch.no_grad():
        p, t = preds.detach(), targets.detach()
        if p.dim() == 1:
            p, t = p.reshape(-1, 1), t.reshape(-1, 1)
        if p.is_cuda:
            table = _moments_device(p.float().contiguous(), t.float().contiguous())
        else:
            table = _moments_host(p, t)
    return _fill(_task_cache, key, preds, targets, table)


class _TaskMetric(nn.Module):
    """value(): the metric as a Python float derived in fp64; forward(): the same as a 0-dim fp32 CPU tensor"""

    def value(self, preds, targets):
        raise NotImplementedError

    def forward(self, preds, targets):
        return torch.tensor(self.value(preds, targets), dtype=torch.float32)


def _div(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):       # a constant target: x / 0, as torch's division
        return np.float64(a) / np.float64(b)


class PearsonR(_TaskMetric):
    """reference trainer/metrics.py:15-32: per task, `+ 1e-8` in the denominator, clamped to [-1, 1], then the mean over the tasks."""

    def value(self, preds, targets):
        m = task_moments(preds, targets)[:-1]
        r = m[:, SPT] / (np.sqrt(m[:, SPP]) * np.sqrt(m[:, STT]) + 1e-8)
        return float(np.clip(r, -1.0, 1.0).mean())


class Rsquared(_TaskMetric):
    """reference trainer/metrics.py:131-145: 1 - sum (t - p)^2 / sum (t - tbar)^2 with the mean of ALL targets."""

    def value(self, preds, targets):
        tot = task_moments(preds, targets)[-1]
        return float(1.0 - _div(tot[L2], tot[GL2]))


class MAE(_TaskMetric):
    """reference trainer/metrics.py:73-79."""

    def value(self, preds, targets):
        tot = task_moments(preds, targets)[-1]
        return float(tot[L1] / tot[N])


class MeanPredictorLoss(_TaskMetric):
    """reference trainer/metrics.py:148-158: loss_func(the mean of all targets everywhere, targets).  torch.nn.L1Loss / MSELoss with
    the default reduction come from the table; any other loss_func is called as the reference calls it."""

    def __init__(self, loss_func) -> None:
        super().__init__()
        self.loss_func = loss_func

    def _column(self):
        col = {nn.L1Loss: GL1, nn.MSELoss: GL2}.get(type(self.loss_func))
        return col if getattr(self.loss_func, 'reduction', None) == 'mean' else None

    def value(self, x1, targets):
        col = self._column()
        if col is None:
            raise NotImplementedError('MeanPredictorLoss.value: only torch.nn.L1Loss / MSELoss with the default reduction come from the '
                                      'moments table; forward() calls any other loss_func')
        tot = task_moments(x1, targets)[-1]
        return float(tot[col] / tot[N])

    def forward(self, x1, targets):
        if self._column() is None:
            return self.loss_func(torch.full_like(targets, targets.mean()), targets)
        return super().forward(x1, targets)


def _denormalisation_scale(dataset):
    """per task |d denormalize / d normalized| = std_c (* eV2meV_c): the means cancel in denormalize(p) - denormalize(t).  The
    reference tests `if eV2meV:` on the tensor, which raises for more than one task; here the factor applies whenever it is not None."""
    scale = np.abs(np.asarray(torch.as_tensor(dataset.targets_std).detach().cpu().double().reshape(-1).numpy()))
    factor = getattr(dataset, 'eV2meV', None)
    if factor is not None:
        scale = scale * np.abs(torch.as_tensor(factor).detach().cpu().double().reshape(-1).numpy())
    return scale


class _Denormalized(_TaskMetric):
    def __init__(self, dataset):
        super().__init__()
        self.means, self.stds, self.eV2meV = dataset.targets_mean, dataset.targets_std, getattr(dataset, 'eV2meV', None)
        self.scale = _denormalisation_scale(dataset)

    def _columns(self, preds, targets):
        m = task_moments(preds, targets)
        if m.shape[0] - 1 != self.scale.shape[0]:
            raise ValueError(f'{type(self).__name__}: {m.shape[0] - 1} task columns, the dataset has {self.scale.shape[0]}')
        return m


class QM9DenormalizedL1(_Denormalized):
    """reference trainer/metrics.py:57-70: l1_loss of the denormalised predictions and targets."""

    def value(self, preds, targets):
        m = self._columns(preds, targets)
        return float((m[:-1, L1] * self.scale).sum() / m[-1, N])


class QM9DenormalizedL2(_Denormalized):
    """reference trainer/metrics.py:89-101: mse_loss of the denormalised predictions and targets."""

    def value(self, preds, targets):
        m = self._columns(preds, targets)
        return float((m[:-1, L2] * self.scale ** 2).sum() / m[-1, N])


class QM9SingleTargetDenormalizedL1(_Denormalized):
    """reference trainer/metrics.py:35-54: the denormalised l1_loss of one task's column."""

    def __init__(self, dataset, task: str):
        super().__init__(dataset)
        self.task_index = list(dataset.target_tasks).index(task)

    def value(self, preds, targets):
        m = self._columns(preds, targets)
        return float(m[self.task_index, L1] * self.scale[self.task_index] / m[self.task_index, N])
