"""Forward + backward time of NTXentLikelihoodLoss and JSDMultiplePositivesLoss (csrc/gausspair.hip) on one MI355X against torch-eager
forms on the same device:

  eager      the closed form the kernels compute, vectorised in elementwise torch ops (fp32; the likelihood materialises [B, B, C, D]
             tensors, 1.3 GB each at B = 500, C = 5, D = 256, the JSD [B, B, D] ones)
  loop       the reference's form (commons/losses.py:569-578 and :366-375): a Python double loop of B^2 torch.distributions.Normal
             evaluations (likelihood) or of B^2 per-pair KL expressions (JSD) - at B = 4 only; at B = 500 it is 250 000 iterations

at B = 4 (the batch_size of configs/old_configs/contrastive_training_multiple_positives_likelihood_loss.yml, C = 5, D = 256) and at
B = 500 (the batch of the sibling multi-conformer configs).

Per (loss, form, batch): `--runs` runs of `--steps` steps each after `--warmup` steps, HIP events around each run, the median and the
range of the per-run step time.  One JSON line each.

    python tools/gausspair_bench.py --out profiles/gausspair_bench.jsonl
"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')


def _ntxent_direct(E):
    """mean_i (log sum_{j != i} exp(E_ij) - E_ii), the row maximum out of the exponent"""
    neg = E.masked_fill(torch.eye(E.shape[0], dtype=torch.bool, device=E.device), float('-inf'))
    mx = neg.max(dim=1).values.detach()
    return (mx + torch.log(torch.exp(neg - mx[:, None]).sum(dim=1)) - torch.diagonal(E)).mean()


def lik_eager(z1, z2, tau):
    B, D = z1.shape[0], z2.shape[1]
    m, sigma = z1[:, :D], torch.exp(z1[:, D:] / 2)
    t = (z2.view(B, -1, D)[None] - m[:, None, None, :]) / sigma[:, None, None, :]
    L = (torch.exp(-0.5 * t * t) / (sigma[:, None, None, :] * math.sqrt(2 * math.pi))).mean(dim=(2, 3))
    return _ntxent_direct(L / tau)


def lik_loop(z1, z2, tau):
    B, D = z1.shape[0], z2.shape[1]
    means, stds, x = z1[:, :D], torch.exp(z1[:, D:] / 2), z2.view(B, -1, D)
    kernel = []
    for i in range(B):
        p = torch.distributions.Normal(means[i], stds[i])
        for j in range(B):
            kernel.append(torch.exp(p.log_prob(x[j])).mean())
    return _ntxent_direct(torch.stack(kernel).view(B, B) / tau)


def _jsd_statistics(z1, z2):
    B, D = z1.shape[0], z2.shape[1]
    a = torch.nn.functional.normalize(z1.view(B, 2, D), dim=2)
    b = torch.nn.functional.normalize(z2.view(B, -1, D), dim=2)
    return a[:, 0], a[:, 1], b.mean(dim=1), b.var(dim=1)


def _jsd_from_matrix(S):
    off = ~torch.eye(S.shape[0], dtype=torch.bool, device=S.device)
    return -torch.log(torch.diagonal(S) / (S * off).sum(dim=1)).mean()


def jsd_eager(z1, z2, tau):
    m1, s, m2, v2 = _jsd_statistics(z1, z2)
    quad = ((torch.exp(s)[None] + (m2[:, None] - m1[None]) ** 2) / (v2[:, None] + 1e-5)).sum(dim=2)
    S = 0.5 * (torch.log(v2.prod(dim=1) + 1e-5)[:, None] - s.sum(dim=1)[None] - z2.shape[1] + quad)
    return _jsd_from_matrix(S)


def jsd_loop(z1, z2, tau):
    m1, s, m2, v2 = _jsd_statistics(z1, z2)
    B, D = m1.shape
    rows = []
    for a in range(B):
        for b in range(B):
            log_det = torch.log(v2[a].prod() + 1e-5) - s[b].sum()
            rows.append(0.5 * (log_det - D + (torch.exp(s[b]) / (v2[a] + 1e-5)).sum() + ((m2[a] - m1[b]) ** 2 / (v2[a] + 1e-5)).sum()))
    return _jsd_from_matrix(torch.stack(rows).view(B, B))


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
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 500])
    ap.add_argument('--conformers', type=int, default=5)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--tau', type=float, default=0.1)
    ap.add_argument('--loop-max-batch', type=int, default=4)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    C, D, tau = args.conformers, args.dim, args.tau
    hip_lik, hip_jsd = amd.NTXentLikelihoodLoss(tau=tau), amd.JSDMultiplePositivesLoss(tau=tau)
    forms = {'likelihood': {'hip': hip_lik, 'eager': lambda a, b: lik_eager(a, b, tau), 'loop': lambda a, b: lik_loop(a, b, tau)},
             'jsd': {'hip': hip_jsd, 'eager': lambda a, b: jsd_eager(a, b, tau), 'loop': lambda a, b: jsd_loop(a, b, tau)}}
    lines = []
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        z1 = torch.randn(B, 2 * D, generator=g)
        z1[:, D:] *= 0.5
        z1 = z1.to(dev).requires_grad_(True)
        z2 = torch.randn(B * C, D, generator=g).to(dev).requires_grad_(True)
        for loss, by_form in forms.items():
            for form, fn in by_form.items():
                if form == 'loop' and B > args.loop_max_batch:
                    continue
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                steps = args.steps if form != 'loop' else max(args.steps // 10, 1)          # a step of this form takes milliseconds
                t = time_form(fn, z1, z2, steps, args.warmup, args.runs)
                rec = dict(loss=loss, form=form, batch=B, conformers=C, dim=D, tau=tau, step_ms_median=float(np.median(t)),
                           step_ms_min=min(t), step_ms_max=max(t), runs=args.runs, steps=steps,
                           peak_growth_mb=(torch.cuda.max_memory_allocated() - before) / 2 ** 20, loss_value=float(fn(z1, z2).detach()))
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
        del z1, z2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
