"""Forward + backward times of the non-contrastive losses of csrc/batchstat.hip beside the same formulas in torch eager on one MI355X.

BarlowTwinsLoss, CosineSimilarityLoss, RegularizationLoss (variance and covariance terms on, its default) and CriticLoss with --repeats
reconstructions per row (default 10), at z1, z2 [batch, dim] for every --batch (default 500, the batch of configs/old_configs/
philosophy.yml, and 250, that of configs/byol.yml) and dim 256.  Each form is the module's forward and backward; its eager twin is the
reference's expression on the same device tensors.  Kernel and eager blocks of --iters calls alternate inside one process, --rounds times,
HIP events around each block (launch gaps and allocations included).  Prints one JSON line per form and batch and writes them to --out.

    python tools/batchstat_bench.py --out profiles/batchstat_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')


def std_term(x):
    return torch.relu(1 - torch.sqrt(x.var(dim=0) + 1e-4)).mean()


def cov_term(x):
    n, dim = x.shape
    c = x - x.mean(dim=0)
    cov = c.T @ c / (n - 1)
    return (cov - torch.diag(torch.diagonal(cov))).pow(2).sum() / dim


def eager_barlow(z1, z2, scale_loss=1 / 32, lambd=3.9e-3):
    a = (z1 - z1.mean(dim=0)) / z1.std(dim=0)
    b = (z2 - z2.mean(dim=0)) / z2.std(dim=0)
    C = a.T @ b / z1.shape[0]
    on = (torch.diagonal(C) - 1).pow(2).sum()
    off = (C - torch.diag(torch.diagonal(C))).pow(2).sum()
    return scale_loss * (on + lambd * off)


def eager_cosine(z1, z2):
    return (F.normalize(z1, dim=-1) - F.normalize(z2, dim=-1)).pow(2).sum(dim=-1).mean()


def eager_regularization(z1, z2, variance_reg=1, covariance_reg=0.04):
    return F.mse_loss(z1, z2) + variance_reg * (std_term(z1) + std_term(z2)) + covariance_reg * (cov_term(z1) + cov_term(z2))


def eager_critic(z2, rec):
    return (F.normalize(z2, dim=1)[..., None].repeat(1, 1, rec.shape[2]) - F.normalize(rec, dim=1)).pow(2).sum(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[500, 250])
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for B in a.batch:
        D, R = a.dim, a.repeats
        gen = torch.Generator().manual_seed(0)
        z1 = torch.randn(B, D, generator=gen) * torch.tensor([0.5, 1.5])[torch.arange(D) % 2]
        z2 = torch.tensor([0.0, 0.5, 3.0])[torch.arange(B) % 3][:, None] * z1 + torch.randn(B, D, generator=gen)
        rec = z2[:, :, None] + torch.randn(B, D, R, generator=gen)
        z1, z2, rec = (t.to(dev).requires_grad_(True) for t in (z1, z2, rec))
        forms = [('BarlowTwinsLoss', amd.BarlowTwinsLoss(), eager_barlow, (z1, z2)),
                 ('CosineSimilarityLoss', amd.CosineSimilarityLoss(), eager_cosine, (z1, z2)),
                 ('RegularizationLoss', amd.RegularizationLoss(), eager_regularization, (z1, z2)),
                 (f'CriticLoss(R={R})', amd.CriticLoss(), eager_critic, (z2, rec))]

        def call(fn, args):
            for t in args:
                t.grad = None
            loss = fn(*args)
            loss.backward()
            return loss

        values = {}
        for name, kernel, eager, args in forms:
            for _ in range(a.warmup):
                values[name] = (call(kernel, args), call(eager, args))
        times = {(name, path): [] for name, _, _, _ in forms for path in ('kernels', 'eager')}
        for _ in range(a.rounds):
            for name, kernel, eager, args in forms:
                for path, fn in (('kernels', kernel), ('eager', eager)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(dev)
                    e0.record()
                    for _ in range(a.iters):
                        call(fn, args)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    times[name, path].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        for name, _, _, _ in forms:
            row = dict(what='loss_fwd_bwd', form=name, batch=B, dim=D, iters=a.iters, rounds=a.rounds)
            for path in ('kernels', 'eager'):
                ts = times[name, path]
                row.update({f'{path}_us_median': round(float(np.median(ts)), 1), f'{path}_us_min': round(min(ts), 1),
                            f'{path}_us_max': round(max(ts), 1)})
            row.update(loss_kernels=float(values[name][0].item()), loss_eager=float(values[name][1].item()),
                       device=torch.cuda.get_device_name(dev))
            lines.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
