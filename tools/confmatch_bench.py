"""Forward + backward time of the set-matching and per-conformer NT-Xent losses (csrc/confmatch.hip) on one MI355X against a torch-eager
restatement of the reference's formulas on the same device.

  NTXentMinimumMatching, NTXentMaximumSimilarity        B = 500, C = 5, D = 256, tau 0.1 (configs/contrastive_training_minimum_matching_loss.yml)
  NTXentMultiplePositivesV2, NTXentMultiplePositivesV3  B = 500, C = 10, D = 256 (configs/old_configs/contrastive_training_multiple_positives_V2.yml,
                                                        ..._V3.yml)

Per loss the two forms alternate inside one call: `--runs` rounds of (`--steps` steps of the kernels, `--steps` steps of eager) after
`--warmup` steps of each, HIP events around each run of steps; the median and the range of the per-run step time.  One JSON line per
(loss, form).

    python tools/confmatch_bench.py --out profiles/confmatch_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')

TAU = 0.1


def _blocks(z1, z2):
    B, D = z1.shape[0], z2.shape[1]
    a, b = z1.view(B, -1, D), z2.view(B, -1, D)
    sim = torch.einsum('ilk,juk->ijlu', a, b)
    return sim / torch.einsum('il,ju->ijlu', a.norm(dim=2), b.norm(dim=2))


def eager_min(z1, z2, tau=TAU):
    """reference commons/losses.py:769-786 restated"""
    sim = torch.exp(_blocks(z1, z2) / tau)
    pos = torch.amax(torch.diagonal(sim, dim1=2, dim2=3), dim=(1, 2))
    low = torch.amin(sim, dim=(2, 3))
    return -torch.log(pos / (low.sum(dim=1) - torch.diagonal(low))).mean()


def eager_max(z1, z2, tau=TAU):
    """reference commons/losses.py:861-878 restated"""
    sim = torch.exp(torch.amax(_blocks(z1, z2), dim=(2, 3)) / tau)
    pos = torch.diagonal(sim)
    return -torch.log(pos / (sim.sum(dim=1) - pos)).mean()


def eager_v2(z1, z2, tau=TAU):
    """reference commons/losses.py:620-635 restated"""
    B, D = z1.shape
    b = z2.view(B, -1, D)
    na, nb = z1.norm(dim=1), b.norm(dim=2)
    pos = torch.exp((z1[:, None, :] * b).sum(dim=2) / (na[:, None] * nb) / tau).sum(dim=1)
    sim = torch.exp(torch.einsum('ik,jk->ij', z1, b[:, 0, :]) / torch.einsum('i,j->ij', na, nb[:, 0]) / tau)
    return -torch.log(pos / (sim.sum(dim=1) - torch.diagonal(sim))).mean()


def eager_v3(z1, z2, tau=TAU):
    """reference commons/losses.py:668-681 restated"""
    B, D = z1.shape
    b = z2.view(B, -1, D)
    sim = torch.einsum('ik,juk->iju', z1, b) / torch.einsum('i,ju->iju', z1.norm(dim=1), b.norm(dim=2))
    sim = torch.exp(sim / tau)
    pos = sim[range(B), range(B), :]
    return -torch.log(pos / (sim.sum(dim=1) - pos)).mean()


def run_steps(fn, z1, z2, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        z1.grad = z2.grad = None
        fn(z1, z2).backward()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--matching-conformers', type=int, default=5)
    ap.add_argument('--conformers', type=int, default=10)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--losses', nargs='+', default=['min', 'max', 'v2', 'v3'])
    ap.add_argument('--forms', nargs='+', default=['hip', 'eager'], help='hip alone: what a kernel trace should see')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, D = args.batch, args.dim
    plan = [('min', amd.NTXentMinimumMatching(tau=TAU), eager_min, args.matching_conformers, True),
            ('max', amd.NTXentMaximumSimilarity(tau=TAU), eager_max, args.matching_conformers, True),
            ('v2', amd.NTXentMultiplePositivesV2(tau=TAU), eager_v2, args.conformers, False),
            ('v3', amd.NTXentMultiplePositivesV3(tau=TAU), eager_v3, args.conformers, False)]
    lines = []
    for loss, hip, eager, C, matching in plan:
        if loss not in args.losses:
            continue
        g = torch.Generator().manual_seed(B)
        z1 = torch.randn(B, C * D if matching else D, generator=g).to(dev).requires_grad_(True)
        z2 = torch.randn(B * C, D, generator=g).to(dev).requires_grad_(True)
        forms = {k: fn for k, fn in (('hip', hip), ('eager', eager)) if k in args.forms}
        times, peak = {k: [] for k in forms}, {}
        for k, fn in forms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            run_steps(fn, z1, z2, args.warmup)
            peak[k] = torch.cuda.max_memory_allocated() / 2 ** 20
        for _ in range(args.runs):
            for k, fn in forms.items():
                times[k].append(run_steps(fn, z1, z2, args.steps))
        for k, fn in forms.items():
            t = times[k]
            rec = dict(loss=loss, form=k, batch=B, conformers=C, dim=D, step_ms_median=float(np.median(t)), step_ms_min=min(t),
                       step_ms_max=max(t), runs=args.runs, steps=args.steps, peak_mb=peak[k], loss_value=float(fn(z1, z2).detach()))
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
