"""Contrastive monitoring metrics - drop-in for the classes of reference trainer/metrics.py that
configs_clean/pre-train_QM9.yml:15-24 lists.

The reference trainer calls every metric separately and `.item()`s each result, every `log_iterations` (= 2) steps
(trainer/self_supervised_trainer.py:31-50, train.py:255-268): nine chains of small device ops and nine host syncs.
Here the first metric asked about a pair of embedding tensors computes ALL of them in one device pass (one C call,
csrc/metrics.hip) and brings them to the host with one copy; the other metric objects find the result cached, so the trainer's
loop costs one synchronisation.  Every statistic comes from CENTRED values - column means in fp64 first, distances from the Gram
matrices of the centred rows, alignment from the rows' differences, variances and covariances from the centred columns - as in the
reference (row differences, torch.pdist, cov_loss's centring, torch's two-pass std): embeddings with a common offset, a collapsed
batch and well-aligned views read as what they are (tests/test_gpu_metrics_edges.py).  The products run with exact fp32
products whatever ops.set_matmul_precision / ops.set_fp32_products say.  Same class names, constructor arguments and
call signature; the value comes back as a 0-dim CPU tensor (`.item()` works as in the trainer).  The `pos_mask`
(local-global losses) variants are outside the scope of this path and raise NotImplementedError.

The metrics of configs/contrastive_training_multiple_positives_kl_div_loss.yml see z1 [B, 2 D] and z2 [B C, D]: Conformer3DVariance /
Conformer2DVariance (reference trainer/metrics.py:177-209) share one pass of the KL loss's forward kernel, BatchVariance and
DimensionCovariance - one term per tensor - the per-tensor part of the pass above; each pair costs one synchronisation.

PositiveProb / NegativeProb (reference trainer/metrics.py:336-395, configs/old_configs/contrastive_training_multiple_positives_
likelihood_loss.yml) take the same z1 and read z2 conformer major: the forward kernel of NTXentLikelihoodLoss through strides, one
reduction of its [B, B] matrix, one synchronisation for the pair.
"""
import math
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops

# one entry: (weakref(x1), weakref(x2), key, values).  The key alone (address, version, shape) is NOT an identity: each
# training step's detached embeddings are new tensors with version 0, the same shape and - through the caching allocator -
# very likely the same address, so the cache also requires that the very tensor OBJECTS are the ones it was filled from
# (weak references: a dead tensor can never match, and the cache keeps no embedding alive).
_cache = {'key': None, 'values': None, 'x1': None, 'x2': None}


def _same_object(ref, t):
    return ref is not None and ref() is t


def _log(v):
    with np.errstate(divide='ignore'):       # exp(-t d^2) underflows to 0 for far-apart embeddings: log -> -inf, as torch.log
        return float(np.log(v))


def _tensor_key(x1, x2, *extra):
    return (x1.data_ptr(), x1._version, tuple(x1.shape), x2.data_ptr(), x2._version, tuple(x2.shape)) + extra


def _cached(cache, key, x1, x2):
    if cache['key'] == key and _same_object(cache['x1'], x1) and _same_object(cache['x2'], x2):
        return cache['values']
    return None


def _fill(cache, key, x1, x2, vals):
    cache['key'], cache['values'] = key, vals
    cache['x1'], cache['x2'] = weakref.ref(x1), weakref.ref(x2)
    return vals


def _device_pass(z1, z2, pairwise, threshold=0.5, t=2.0, alpha=2.0):
    """i3d_contrastive_metrics (csrc/metrics.hip) on z1 [B1, D1], z2 [B2, D2] -> (row totals [8], then per view: sum of the squared
    off-diagonal covariances, column means [D], unbiased column variances [D]), fp64, after the one device-to-host copy"""
    (B1, D1), (B2, D2) = z1.shape, z2.shape
    L = _lib.load()
    work = torch.empty(L.i3d_contrastive_metrics_work_floats(B1, B2, D1, D2, int(pairwise)), dtype=torch.float32, device=z1.device)
    out = torch.empty(L.i3d_contrastive_metrics_out_doubles(D1, D2), dtype=torch.float64, device=z1.device)
    _lib.check(L.i3d_contrastive_metrics(z1.data_ptr(), z2.data_ptr(), B1, B2, D1, D2, int(pairwise), float(threshold), float(t),
                                         float(alpha), work.data_ptr(), out.data_ptr(), ops._stream()), 'i3d_contrastive_metrics')
    host = out[:10 + 2 * D1 + 2 * D2].cpu().numpy()                                  # the one device-to-host copy
    o = 10 + 2 * D1
    return host[:8], (host[8], host[10:10 + D1], host[10 + D1:o]), (host[9], host[o:o + D2], host[o + D2:o + 2 * D2])


def _col_std_mean(var):
    return float(np.sqrt(var).mean())


def _all_mean_std(mean, var, n):
    """mean and unbiased standard deviation over ALL elements of an [n, D] tensor from its column means and unbiased column variances:
    sum (x - m)^2 = sum_j [(n - 1) var_j + n (mean_j - m)^2], every term a centred quantity"""
    cnt = n * mean.shape[0]
    m = mean.mean()
    with np.errstate(invalid='ignore', divide='ignore'):     # one element: 0 / 0 = NaN, as torch.std
        ss = ((n - 1) * var).sum() if n > 1 else 0.0         # (one row: var is NaN, the rows' part is zero)
        return float(m), float(math.sqrt((ss + n * ((mean - m) ** 2).sum()) / np.float64(cnt - 1)))


def _all_metrics(x1, x2, threshold=0.5, t=2.0, alpha=2.0):
    key = _tensor_key(x1, x2, float(threshold), float(t), float(alpha))
    vals = _cached(_cache, key, x1, x2)
    if vals is not None:
        return vals
    with torch.no_grad():
        z1, z2 = x1.detach().float().contiguous(), x2.detach().float().contiguous()
        if not z1.is_cuda:
            raise AssertionError('the metrics run on the HIP device (there is no CPU fallback)')
        B1, D = z1.shape
        B2 = z2.shape[0]
        if B2 < B1 or z2.shape[1] != D:                    # x2 may carry extra "noisy" rows at the end (metrics.py:222)
            raise ValueError(f'incompatible embedding shapes {tuple(z1.shape)} / {tuple(z2.shape)}')
        r, (cov1, mean1, var1), (cov2, mean2, var2) = _device_pass(z1, z2, True, threshold, t, alpha)

    tpr = r[2] / B1
    tnr = r[3] / (B1 * (B1 - 1)) if B1 > 1 else float('nan')
    vals = {
        'positive_similarity': (r[7] / B1 + 1) / 2,          # F.cosine_similarity's clamped norms (:331); the others: plain norms
        'negative_similarity': ((r[0] - r[1]) / (B1 * (B1 - 1)) + 1) / 2 if B1 > 1 else float('nan'),
        'true_positive_rate': tpr, 'true_negative_rate': tnr,
        # (:303-307 adds the two fp32 quotients: the same rounding here, so that equal counts give the reference's very value)
        'contrastive_accuracy': (np.float32(tpr) + np.float32(tnr)) / np.float32(2),
        'alignment': r[4] / B1,
        'uniformity': (_log(r[5] / (B1 * (B1 - 1) / 2)) + _log(r[6] / (B2 * (B2 - 1) / 2))) / 2 if B1 > 1 else float('nan'),
        'batch_variance': _col_std_mean(var1) + _col_std_mean(var2),
        'dimension_covariance': cov1 / D + cov2 / D,
    }
    vals['mean_pred'], vals['std_pred'] = _all_mean_std(mean1, var1, B1)
    vals['mean_targets'], vals['std_targets'] = _all_mean_std(mean2, var2, B2)
    vals = {k: float(v) for k, v in vals.items()}
    return _fill(_cache, key, x1, x2, vals)


# BatchVariance and DimensionCovariance are sums of one term per tensor: on embeddings of different widths (z1 [B, 2 D] and z2 [B C, D]
# of KLDivergenceMultiplePositives) they take this pass, the per-tensor part of the one above, with a cache of its own.
_per_tensor_cache = {'key': None, 'values': None, 'x1': None, 'x2': None}


def _per_tensor_metrics(x1, x2):
    key = _tensor_key(x1, x2)
    vals = _cached(_per_tensor_cache, key, x1, x2)
    if vals is not None:
        return vals
    with torch.no_grad():
        zs = [x.detach().float().contiguous() for x in (x1, x2)]
        if not all(z.is_cuda for z in zs):
            raise AssertionError('the metrics run on the HIP device (there is no CPU fallback)')
        if any(z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1 for z in zs):
            raise ValueError(f'incompatible embedding shapes {tuple(x1.shape)} / {tuple(x2.shape)}')
        _, *views = _device_pass(zs[0], zs[1], False)
    vals = {'batch_variance': 0.0, 'dimension_covariance': 0.0}
    for z, (cov, _, var) in zip(zs, views):
        vals['batch_variance'] += _col_std_mean(var)
        vals['dimension_covariance'] += float(cov / z.shape[1])
    return _fill(_per_tensor_cache, key, x1, x2, vals)


# Conformer3DVariance / Conformer2DVariance: the second and third per-molecule sums of the KL loss's forward kernel (csrc/klmp.hip)
_conformer_cache = {'key': None, 'values': None, 'x1': None, 'x2': None}


def _conformer_metrics(x1, x2, normalize):
    """z1 [B, 2 D] (mean | log-variance), z2 [B C, D]: the mean over molecules and features of the variance over the conformers, and of
    exp(log-variance); normalize: both on the row-normalised views (F.normalize(dim=2) of [B, 2, D] and [B, C, D])"""
    key = _tensor_key(x1, x2, bool(normalize))
    vals = _cached(_conformer_cache, key, x1, x2)
    if vals is not None:
        return vals
    if x1.dim() != 2 or x2.dim() != 2 or x1.shape[0] < 1 or x1.shape[1] != 2 * x2.shape[1] or x2.shape[0] % x1.shape[0] != 0 \
            or x2.shape[0] // x1.shape[0] < 2:
        raise ValueError(f'incompatible embedding shapes {tuple(x1.shape)} / {tuple(x2.shape)}: [batch, 2 * dim] and '
                         '[batch * conformers, dim] with at least two conformers expected')
    with torch.no_grad():
        z1, z2 = x1.detach().float().contiguous(), x2.detach().float().contiguous()
        if not (z1.is_cuda and z2.is_cuda):
            raise AssertionError('the metrics run on the HIP device (there is no CPU fallback)')
        B, D = z1.shape[0], z2.shape[1]
        if normalize:
            z1, z2 = ops.row_normalize_fwd(z1.reshape(2 * B, D))[0], ops.row_normalize_fwd(z2)[0]
        stats, _ = ops.kl_mp_fwd(z1, z2, B, z2.shape[0] // B, 1.0 / B, want_loss=False)
        host = stats.cpu().numpy()                                                  # the one device-to-host copy
    vals = {'conformer_3d_variance': float(host[:, 1].sum() / (B * D)), 'conformer_2d_variance': float(host[:, 2].sum() / (B * D))}
    return _fill(_conformer_cache, key, x1, x2, vals)


# PositiveProb / NegativeProb: the forward kernel of NTXentLikelihoodLoss (csrc/gausspair.hip) and one reduction of its [B, B] matrix
_prob_cache = {'key': None, 'values': None, 'x1': None, 'x2': None}


def _prob_metrics(x1, x2):
    """z1 [B, 2 D] (mean | log-variance), z2 [C B, D] CONFORMER major - row r is molecule r % B, conformer r // B (the reference views it
    as z2.view(-1, B, D).permute(1, 0, 2), unlike the loss): L_ij = the mean density of molecule j's conformers under molecule i's
    Gaussian; positive_prob = mean_i L_ii, negative_prob = mean_i sum_{j != i} L_ij (a sum over j)"""
    key = _tensor_key(x1, x2)
    vals = _cached(_prob_cache, key, x1, x2)
    if vals is not None:
        return vals
    if x1.dim() != 2 or x2.dim() != 2 or x1.shape[0] < 1 or x2.shape[1] < 1 or x1.shape[1] != 2 * x2.shape[1] \
            or x2.shape[0] < x1.shape[0] or x2.shape[0] % x1.shape[0] != 0:
        raise ValueError(f'incompatible embedding shapes {tuple(x1.shape)} / {tuple(x2.shape)}: [batch, 2 * dim] and '
                         '[conformers * batch, dim] expected')
    B = x1.shape[0]
    if B < 2:
        raise ValueError(f'incompatible embedding shapes {tuple(x1.shape)} / {tuple(x2.shape)}: a batch of {B} has no negatives')
    with torch.no_grad():
        z1, z2 = x1.detach().float().contiguous(), x2.detach().float().contiguous()
        if not (z1.is_cuda and z2.is_cuda):
            raise AssertionError('the metrics run on the HIP device (there is no CPU fallback)')
        lik = ops.gauss_lik_fwd(z1, z2, B, z2.shape[0] // B, conformer_major=True)
        host = ops.gauss_lik_probs(lik).cpu().numpy()                               # the one device-to-host copy
    vals = {'positive_prob': float(host[0]), 'negative_prob': float(host[1])}
    return _fill(_prob_cache, key, x1, x2, vals)


def contrastive_metrics(z2d, z3d, threshold=0.5009, t=2.0, alpha=2.0):
    """All metrics (and the four statistics of SelfSupervisedTrainer.evaluate_metrics, :33-36) as a dict of floats."""
    return dict(_all_metrics(z2d, z3d, threshold, t, alpha))


class _Metric(nn.Module):
    name = None

    def _kw(self):
        return {}

    def forward(self, x1, x2, pos_mask=None):
        if pos_mask is not None:
            raise NotImplementedError('pos_mask (local-global contrastive losses) is outside the accelerated path')
        return torch.tensor(_all_metrics(x1, x2, **{**_shared_defaults(), **self._kw()})[self.name], dtype=torch.float32)


_defaults = {'threshold': 0.5009, 't': 2.0, 'alpha': 2.0}        # train.py:261-266: the values the reference constructs with


def _shared_defaults():
    return dict(_defaults)


class PositiveSimilarity(_Metric):
    """reference trainer/metrics.py:310-333."""
    name = 'positive_similarity'


class NegativeSimilarity(_Metric):
    """reference trainer/metrics.py:443-463."""
    name = 'negative_similarity'


class _Thresholded(_Metric):
    def __init__(self, threshold=0.5):
        super().__init__()
        self.threshold = threshold

    def _kw(self):
        return {'threshold': self.threshold}


class TruePositiveRate(_Thresholded):
    """reference trainer/metrics.py:237-258."""
    name = 'true_positive_rate'


class TrueNegativeRate(_Thresholded):
    """reference trainer/metrics.py:261-283."""
    name = 'true_negative_rate'


class ContrastiveAccuracy(_Thresholded):
    """reference trainer/metrics.py:286-310."""
    name = 'contrastive_accuracy'


class Uniformity(_Metric):
    """reference trainer/metrics.py:228-234, commons/losses.py:946-951."""
    name = 'uniformity'

    def __init__(self, t=2):
        super().__init__()
        self.t = t

    def _kw(self):
        return {'t': self.t}


class Alignment(_Metric):
    """reference trainer/metrics.py:216-225."""
    name = 'alignment'

    def __init__(self, alpha=2):
        super().__init__()
        self.alpha = alpha

    def _kw(self):
        return {'alpha': self.alpha}


class _PerTensor(_Metric):
    """a sum of one term per tensor: embeddings of different widths are fine"""

    def forward(self, x1, x2, pos_mask=None):
        if pos_mask is None and x1.dim() == 2 and x2.dim() == 2 and x1.shape[1] != x2.shape[1]:
            return torch.tensor(_per_tensor_metrics(x1, x2)[self.name], dtype=torch.float32)
        return super().forward(x1, x2, pos_mask)


class BatchVariance(_PerTensor):
    """reference trainer/metrics.py:169-174."""
    name = 'batch_variance'


class DimensionCovariance(_PerTensor):
    """reference trainer/metrics.py:161-166, commons/losses.py:954-959."""
    name = 'dimension_covariance'


class _ConformerVariance(nn.Module):
    name = None

    def __init__(self, normalize=False):
        super().__init__()
        self.norm = normalize

    def forward(self, z1, z2, pos_mask=None):
        return torch.tensor(_conformer_metrics(z1, z2, self.norm)[self.name], dtype=torch.float32)


class Conformer3DVariance(_ConformerVariance):
    """reference trainer/metrics.py:177-192: mean over molecules and features of the variance over the conformers of z2."""
    name = 'conformer_3d_variance'


class Conformer2DVariance(_ConformerVariance):
    """reference trainer/metrics.py:195-209: mean of exp(log-variance), the second half of every row of z1."""
    name = 'conformer_2d_variance'


class _Prob(nn.Module):
    name = None

    def forward(self, z1, z2, pos_mask=None):
        if z1.shape[0] == z2.shape[1] == 2:          # the trainer's dictionary-init call (reference trainer/metrics.py:344)
            return torch.tensor(float('nan'))
        return torch.tensor(_prob_metrics(z1, z2)[self.name], dtype=torch.float32)


class PositiveProb(_Prob):
    """reference trainer/metrics.py:336-364: the mean over molecules of the mean density of a molecule's own conformers under its
    predicted Gaussian."""
    name = 'positive_prob'


class NegativeProb(_Prob):
    """reference trainer/metrics.py:367-395: the mean over molecules of the SUM over the other molecules of the mean density of their
    conformers under this molecule's Gaussian."""
    name = 'negative_prob'
