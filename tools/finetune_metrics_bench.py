"""Time of the fine-tuning losses and metrics (csrc/task.hip) on one MI355X against torch-eager restatements of the same formulas on the
same tensors:

  loss     forward + backward of OGBNanLabelBCEWithLogitsLoss / OGBNanLabelMSELoss at [128, 1], [1024, 12] and [512, 617] with 30 % NaN
           labels, against the reference's form (pred[is_labeled], target[is_labeled] into torch's loss)
  metrics  one Trainer.evaluate_metrics-shaped round on [128, 12]: mae_denormalized, pearsonr, rsquared and the 12 single-target metrics,
           each followed by .item(), against the reference's formulas written out below

    python tools/finetune_metrics_bench.py > profiles/finetune_metrics_<date>.txt

Wall time per call (host + device: the point of both paths is the host synchronisations they save) over windows of --seconds each
(at least --iters calls) after --warmup calls; --repeats windows per form, the two forms alternating; median, minimum and maximum of
the windows, one line per measurement.  Reads nothing outside the repository."""
import argparse
import importlib
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
amd = importlib.import_module('3dinfomax_amd')


def window(fn, iters):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def compare(forms, args):
    """{name: (median, min, max)} microseconds per call.  Every form is warmed up, its window sized to --seconds from a pilot run (a
    window of a few milliseconds measures the clock and the scheduler), and the forms alternate inside every repeat so that a
    disturbance of the shared host hits both."""
    iters = {}
    for name, fn in forms.items():
        window(fn, args.warmup)
        iters[name] = max(args.iters, int(args.seconds * 1e6 / window(fn, args.iters)))
    runs = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            runs[name].append(window(fn, iters[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in runs.items()}


def report(what, us):
    h, e = us['hip'], us['eager']
    print(f'{what}: hip {h[0]:.1f} us (min {h[1]:.1f}, max {h[2]:.1f}) eager {e[0]:.1f} us (min {e[1]:.1f}, max {e[2]:.1f}) '
          f'ratio {e[0] / h[0]:.2f}')


def eager_loss(kind):
    inner = torch.nn.BCEWithLogitsLoss() if kind == 'bce' else torch.nn.MSELoss()

    def loss(pred, target):
        labelled = ~torch.isnan(target)
        return inner(pred[labelled], target[labelled])
    return loss


def eager_metrics(std, factor, T):
    def denorm(x):
        return x * (std * factor)[None, :]          # the means cancel in the differences below

    def mae_denormalized(p, t):
        return torch.nn.functional.l1_loss(denorm(p), denorm(t))

    def pearsonr(p, t):
        sx, sy = p - p.mean(dim=0), t - t.mean(dim=0)
        r = (sx * sy).sum(dim=0) / (torch.sqrt((sx ** 2).sum(dim=0)) * torch.sqrt((sy ** 2).sum(dim=0)) + 1e-8)
        return torch.clamp(r, min=-1, max=1).mean()

    def rsquared(p, t):
        return 1 - ((t - p) ** 2).sum() / ((t - t.mean()) ** 2).sum()

    def single(c):
        return lambda p, t: torch.nn.functional.l1_loss(denorm(p)[:, c], denorm(t)[:, c])
    return [mae_denormalized, pearsonr, rsquared] + [single(c) for c in range(T)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print(f'device {torch.cuda.get_device_name(0)} torch {torch.__version__} window {args.seconds} s (at least {args.iters} calls) '
          f'repeats {args.repeats}, forms alternating')
    g = torch.Generator().manual_seed(0)
    for B, T in ((128, 1), (1024, 12), (512, 617)):
        pred = torch.randn(B, T, generator=g).to(dev).requires_grad_(True)
        target = (torch.rand(B, T, generator=g) < 0.5).float()
        target[torch.rand(B, T, generator=g) < 0.3] = float('nan')
        target = target.to(dev)
        for kind, ours in (('bce', amd.OGBNanLabelBCEWithLogitsLoss()), ('mse', amd.OGBNanLabelMSELoss())):
            def step(loss_fn):
                pred.grad = None
                loss_fn(pred, target).backward()
            us = compare({name: (lambda f=f: step(f)) for name, f in (('hip', ours), ('eager', eager_loss(kind)))}, args)
            report(f'loss {kind} [{B}, {T}] forward+backward', us)
    B, T = 128, 12
    target = torch.randn(B, T, generator=g).to(dev)
    pred = (target + 0.3 * torch.randn(B, T, generator=g).to(dev)).contiguous()
    ds = types.SimpleNamespace(targets_mean=torch.zeros(T), targets_std=torch.full((T,), 0.5), eV2meV=torch.full((T,), 1000.0),
                               target_tasks=[f'task{c}' for c in range(T)])
    ours = [amd.QM9DenormalizedL1(ds), amd.PearsonR(), amd.Rsquared()] + [amd.QM9SingleTargetDenormalizedL1(ds, t) for t in ds.target_tasks]
    eager = eager_metrics(ds.targets_std.to(dev), ds.eV2meV.to(dev), T)

    def round_of(metrics):
        p = pred.clone()                  # a new pair every round, as every batch of the trainer is
        return [m(p, target).item() for m in metrics]
    a, b = round_of(ours), round_of(eager)
    worst = max(abs(x - y) / max(abs(y), 1e-30) for x, y in zip(a, b))
    us = compare({name: (lambda m=m: round_of(m)) for name, m in (('hip', ours), ('eager', eager))}, args)
    report(f'metrics round [{B}, {T}] {len(ours)} metrics, .item() each (largest relative difference between the two forms {worst:.1e})', us)


if __name__ == '__main__':
    main()
