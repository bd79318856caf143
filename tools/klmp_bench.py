"""Forward + backward time of KLDivergenceMultiplePositives (csrc/klmp.hip) on one MI355X against two torch-eager forms on the same
device:

  closed     the closed form the kernels compute, in elementwise torch ops
  mvn        the reference's form (commons/losses.py:279-306): two MultivariateNormal objects over torch.diag_embed covariances
             ([B, D, D] each), Cholesky factorisations and triangular solves inside torch.distributions.kl_divergence

at B = 500, C = 3, D = 256 (the batch of the sibling multi-conformer configs) and at B = 4 (the batch_size of
configs/contrastive_training_multiple_positives_kl_div_loss.yml itself).

Per (form, batch): `--runs` runs of `--steps` steps each after `--warmup` steps, HIP events around each run, the median and the range of
the per-run step time.  One JSON line each.

    python tools/klmp_bench.py --out profiles/klmp_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
from torch.distributions import MultivariateNormal, kl_divergence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')


def _statistics(z1, z2):
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.view(B, 2, D), z2.view(B, -1, D)
    return a[:, 0], a[:, 1], b.mean(1), b.var(1) + 1e-6


def eager_closed(z1, z2):
    m1, s1, m2, v2 = _statistics(z1, z2)
    return (0.5 * (s1 - torch.log(v2) + (v2 + (m2 - m1) ** 2) * torch.exp(-s1) - 1.0).sum(dim=1)).mean()


def eager_mvn(z1, z2):
    m1, s1, m2, v2 = _statistics(z1, z2)
    normal1 = MultivariateNormal(m1, torch.diag_embed(torch.exp(s1)))
    normal2 = MultivariateNormal(m2, torch.diag_embed(v2))
    return kl_divergence(normal2, normal1).mean()


def time_form(fn, z1, z2, steps, warmup, runs):
    def step():
        z1.grad = z2.grad = None
        fn(z1, z2).backward()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            step()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / steps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[500, 4])
    ap.add_argument('--conformers', type=int, default=3)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    C, D = args.conformers, args.dim
    forms = {'hip': amd.KLDivergenceMultiplePositives(), 'closed': eager_closed, 'mvn': eager_mvn}
    lines = []
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        z1 = torch.randn(B, 2 * D, generator=g).to(dev).requires_grad_(True)
        z2 = torch.randn(B * C, D, generator=g).to(dev).requires_grad_(True)
        for form, fn in forms.items():
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            steps = args.steps if form != 'mvn' else max(args.steps // 10, 1)          # a step of this form takes milliseconds
            t = time_form(fn, z1, z2, steps, args.warmup, args.runs)
            rec = dict(loss='kl', form=form, batch=B, conformers=C, dim=D, step_ms_median=float(np.median(t)), step_ms_min=min(t),
                       step_ms_max=max(t), runs=args.runs, steps=steps,
                       peak_growth_mb=(torch.cuda.max_memory_allocated() - before) / 2 ** 20, loss_value=float(fn(z1, z2)))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del z1, z2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
