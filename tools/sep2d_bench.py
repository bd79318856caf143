"""Forward + backward time of the conformer-wise losses (csrc/sep2d.hip) on one MI355X against a torch-eager restatement of the
reference's formulas on the same device.

  NTXentMultiplePositivesSeparate2D  B = 500, C = 5, D = 256 (configs/contrastive_training_multiple_positives_separate2d.yml), both forms
  NTXentMMDSeparate2D                the kernels at B = 500; eager materialises [B, B, 2C, 2C, D] several times over (9.2 GB per copy at
                                     B = 500), so both forms are also timed at --eager-batch (default 64), the largest batch eager fits

Per (loss, form, batch): `--runs` runs of `--steps` steps each after `--warmup` steps, HIP events around each run, the median and the
range of the per-run step time.  One JSON line each.

    python tools/sep2d_bench.py --out profiles/sep2d_bench.jsonl
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

TAU = 0.1


def eager_sep(z1, z2, tau=TAU):
    """reference commons/losses.py:714-736 restated"""
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.view(B, -1, D), z2.view(B, -1, D)
    sim = torch.einsum('ilk,juk->ijlu', a, b)
    na, nb = a.norm(dim=2), b.norm(dim=2)
    pos = torch.exp((a * b).sum(dim=2) / (na * nb) / tau).sum(dim=1)
    sim = torch.exp(sim / torch.einsum('il,ju->ijlu', na, nb) / tau).reshape(B, B, -1).sum(dim=2)
    return -torch.log(pos / (sim.sum(dim=1) - torch.diagonal(sim))).mean()


def eager_mmd(z1, z2, tau=TAU, kernel_num=5, kernel_mul=2.0):
    """reference commons/losses.py:428-468 restated: the [B, B, 2C, 2C, D] difference tensor and all"""
    B, D = z1.shape[0], z2.shape[1]
    x, y = F.normalize(z1.view(B, -1, D), dim=2), F.normalize(z2.view(B, -1, D), dim=2)
    C = x.shape[1]
    total = torch.cat([x.unsqueeze(0).expand(B, -1, -1, -1), y.unsqueeze(1).expand(-1, B, -1, -1)], dim=2)
    L2 = ((total.unsqueeze(2) - total.unsqueeze(3)) ** 2).sum(4)
    bw = L2.detach().sum(dim=(2, 3)) / ((2 * C) ** 2 - 2 * C) / kernel_mul ** (kernel_num // 2)
    K = sum(torch.exp(-L2 / (bw * kernel_mul ** k)[:, :, None, None]) for k in range(kernel_num))
    mmd = (K[:, :, :C, :C] + K[:, :, C:, C:] - K[:, :, :C, C:] - K[:, :, C:, :C]).mean(dim=(2, 3))
    P = torch.exp(1 / (mmd + 1) / tau)
    pos = torch.diagonal(P)
    return -torch.log(pos / (P.sum(dim=1) - pos)).mean()


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
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--eager-batch', type=int, default=64)
    ap.add_argument('--conformers', type=int, default=5)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    C, D = args.conformers, args.dim
    forms = {'sep': (amd.NTXentMultiplePositivesSeparate2D(tau=TAU), eager_sep), 'mmd': (amd.NTXentMMDSeparate2D(tau=TAU), eager_mmd)}
    plan = [('sep', 'hip', args.batch), ('sep', 'eager', args.batch), ('mmd', 'hip', args.batch), ('mmd', 'hip', args.eager_batch),
            ('mmd', 'eager', args.eager_batch)]
    lines = []
    for loss, form, B in plan:
        g = torch.Generator().manual_seed(B)
        z1 = torch.randn(B, C * D, generator=g).to(dev).requires_grad_(True)
        z2 = torch.randn(B * C, D, generator=g).to(dev).requires_grad_(True)
        fn = forms[loss][0 if form == 'hip' else 1]
        torch.cuda.reset_peak_memory_stats()
        t = time_form(fn, z1, z2, args.steps, args.warmup, args.runs)
        rec = dict(loss=loss, form=form, batch=B, conformers=C, dim=D, step_ms_median=float(np.median(t)), step_ms_min=min(t),
                   step_ms_max=max(t), runs=args.runs, steps=args.steps, peak_mb=torch.cuda.max_memory_allocated() / 2 ** 20,
                   loss_value=float(fn(z1, z2)))
        if loss == 'mmd' and B == args.eager_batch:
            rec['note'] = f'B = {B}: the largest batch at which the eager form fits'
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del z1, z2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
