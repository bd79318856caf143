"""Training-step time of the distance-prediction baseline (configs_clean/pre-train_distance_predictor_baseline.yml sizes: PNA hidden
200, depth 7, transformer nhead 2 / feed-forward 200, distance_net of one Linear, L1 loss, Adam) on one MI355X.

Two forms of the same step on the same device and batch:
  hip    the package's DistancePredictor (HIP kernels end to end)
  eager  our PNAGNN, then the reference's composition in torch eager: padded [B, maxN, H] batch, nn.TransformerEncoderLayer with
         the key padding mask, the two distance_net calls on the [P, 2H] concatenations, softplus
Prints one JSON line per (form, batch) and writes them to --out.  Per-kernel times: run the hip form once under
`rocprofv3 --kernel-trace --stats` (a run of its own), then --kernel-stats on the database it wrote: per kernel the launches and
the device time per training step (warm-up steps included in the division, the trace covers them).

    python tools/distance_predictor_bench.py --batches 100 500 --steps 30 --warmup 5 --out profiles/distance_predictor_bench.jsonl
    rocprofv3 --kernel-trace --stats -d prof -o dp -- python tools/distance_predictor_bench.py --batches 100 --forms hip --steps 10 --warmup 3
    python tools/distance_predictor_bench.py --kernel-stats prof/dp_results.db --trace-steps 13
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')
dataset = importlib.import_module('3dinfomax_amd.dataset')

PNA_ARGS = dict(hidden_dim=200, mid_batch_norm=True, last_batch_norm=True, batch_norm_momentum=0.1, dropout=0.0, propagation_depth=7,
                aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'],
                readout_aggregators=['min', 'max', 'mean', 'sum'], pretrans_layers=2, posttrans_layers=1, residual=True)
MODEL = dict(target_dim=1, projection_dim=0, distance_net=True, projection_layers=1, transformer_layer=True, nhead=2,
             dim_feedforward=200)


def eager_forward(model, g, pidx, mask):
    model.node_gnn(g)
    h = g.ndata['feat']
    B, M = mask.shape
    H = h.shape[1]
    keep = ~mask.reshape(-1)
    pad = torch.zeros(B * M, H, device=h.device)
    pad[keep] = h
    h = model.transformer_layer(pad.view(B, M, H), src_key_padding_mask=mask).reshape(B * M, H)[keep]
    lin = model.distance_net.fully_connected[0].linear
    hs, hd = h[pidx[0]], h[pidx[1]]
    return F.softplus(F.linear(torch.cat([hs, hd], 1), lin.weight, lin.bias) + F.linear(torch.cat([hd, hs], 1), lin.weight, lin.bias))


def run(form, B, steps, warmup, dev):
    mols = amd.synth.make_dataset(B, seed=B)
    ds = dataset.FlatMolDataset(mols)
    [g, pidx, mask], dist = ds.assemble_distance(np.arange(B), dev)
    torch.manual_seed(0)
    model = amd.DistancePredictor(pna_args=dict(PNA_ARGS), **MODEL).to(dev).train()
    opt = amd.Adam(model.parameters(), lr=1e-3)
    loss_fn = torch.nn.L1Loss()

    def step():
        opt.zero_grad(set_to_none=True)
        gg = g.local_copy()
        y = model(gg, pidx, mask) if form == 'hip' else eager_forward(model, gg, pidx, mask)
        loss = loss_fn(y, dist)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return dict(form=form, batch=B, atoms=int(g.number_of_nodes()), pairs=int(pidx.shape[1]), steps=steps, warmup=warmup,
                ms_per_step=round(ms, 4), molecules_per_s=round(B / ms * 1e3, 1), last_loss=float(loss.item()),
                device=torch.cuda.get_device_name(dev))


def kernel_stats(db, steps):
    """table of the kernels of a rocprofv3 database (rocpd): launches and microseconds per step, share of the device time"""
    import sqlite3
    rows = sqlite3.connect(db).execute('select name, count(*), sum(duration) from kernels group by name order by sum(duration) desc')
    rows = [(n.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', ''), c, t / 1e3 / steps) for n, c, t in rows]
    total = sum(r[2] for r in rows)
    out = [f'{"us/step":>9} {"share":>6} {"calls/step":>10}  kernel', f'{total:9.1f} {100.0:6.1f} {sum(r[1] for r in rows) / steps:10.1f}  (all)']
    out += [f'{t:9.1f} {100 * t / total:6.1f} {c / steps:10.1f}  {n}' for n, c, t in rows]
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-stats', default=None, help='rocpd database of a rocprofv3 --kernel-trace run: print the kernel table')
    ap.add_argument('--trace-steps', type=int, default=13, help='training steps the traced run took (warm-up included)')
    ap.add_argument('--batches', type=int, nargs='+', default=[100, 500])
    ap.add_argument('--forms', nargs='+', default=['hip', 'eager'], choices=['hip', 'eager'])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        print(kernel_stats(a.kernel_stats, a.trace_steps))
        return
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for B in a.batches:
        for form in a.forms:          # both forms of one batch size back to back
            r = run(form, B, a.steps, a.warmup, dev)
            print(json.dumps(r), flush=True)
            lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
