"""Forward + backward times of the single-positive losses of csrc/hardneg.hip beside NTXent on one MI355X.

At z1, z2 [batch, dim] (default 500 x 256, tau 0.1): NTXent (csrc/ntxent.hip), InfoNCE, NTXentHard, InfoNCEHard (normalised) and
NTXentExtraNegatives with --extras private negatives per row (default 10), each the module's forward and backward.  The forms are
alternated in blocks of --iters calls inside one process, --rounds times, HIP events around each block (launch gaps and allocations
included).  Prints one JSON line per form and writes them to --out.

    python tools/hardneg_bench.py --out profiles/hardneg_bench.jsonl
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--extras', type=int, default=10)
    ap.add_argument('--tau', type=float, default=0.1)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    B, D, U = a.batch, a.dim, a.extras
    gen = torch.Generator().manual_seed(0)
    z1 = torch.randn(B, D, generator=gen)
    z2 = torch.tensor([0.0, 0.5, 3.0])[torch.arange(B) % 3][:, None] * z1 + torch.randn(B, D, generator=gen)
    z2x = torch.cat([z2, torch.randn(B * U, D, generator=gen)])
    z1, z2, z2x = (t.to(dev).requires_grad_(True) for t in (z1, z2, z2x))
    forms = [('NTXent', amd.NTXent(tau=a.tau), z2), ('InfoNCE', amd.InfoNCE(tau=a.tau), z2),
             ('NTXentHard', amd.NTXentHard(tau=a.tau), z2), ('InfoNCEHard', amd.InfoNCEHard(norm=True, tau=a.tau), z2),
             (f'NTXentExtraNegatives(U={U})', amd.NTXentExtraNegatives(tau=a.tau), z2x)]

    def call(fn, other):
        z1.grad = other.grad = None
        loss = fn(z1, other)
        loss.backward()
        return loss

    values = {}
    for name, fn, other in forms:
        for _ in range(a.warmup):
            values[name] = call(fn, other)
    times = {name: [] for name, _, _ in forms}
    for _ in range(a.rounds):
        for name, fn, other in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(a.iters):
                call(fn, other)
            e1.record()
            torch.cuda.synchronize(dev)
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    lines = [dict(what='loss_fwd_bwd', form=name, batch=B, dim=D, tau=a.tau, iters=a.iters, rounds=a.rounds,
                  us_per_call_median=round(float(np.median(ts)), 1), us_per_call_min=round(min(ts), 1), us_per_call_max=round(max(ts), 1),
                  loss=float(values[name].item()), device=torch.cuda.get_device_name(dev)) for name, ts in times.items()]
    for r in lines:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
