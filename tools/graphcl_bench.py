"""Training-step time of the GraphCL baseline (configs_clean/pre-train_graphCL_baseline.yml sizes: PNA hidden 200, depth 7, target
256, readout min/max/mean, BatchNorm momentum 0.93, NTXent tau 0.1, Adam lr 8e-5, batch 500) on one MI355X, on drug-sized
synthetic molecules (synth.qmugs_like, ~49 atoms and ~100 directed edges: a stand-in for GEOM-Drugs).

One step = assemble the batch in the training thread, upload, model(view 1), model(view 2) (train mode), NTXent, backward, Adam:
  nodedrop   the two views of NodeDropCollate(0.2), built on the device from one upload (FlatMolDataset.assemble_nodedrop_host,
             dataset.nodedrop_to_device: csrc/nodedrop.hip)
  undropped  both "views" are the whole batch, each assembled with FlatMolDataset.assemble_2d (this form uses only what the
             package had before the node drop existed, so this file runs unchanged in such a checkout)
Prints one JSON line per run (ms_per_step: host clock around `steps` steps ending in a device synchronise;
host_enqueue_ms_per_step: the training thread's time inside the steps, i.e. to enqueue them) and appends them to --out.
Per-kernel times: run once under `rocprofv3 --kernel-trace --stats` (a run of its own), then --kernel-stats on its database.

    python tools/graphcl_bench.py --forms nodedrop undropped --steps 30 --warmup 5 --out profiles/graphcl_bench.jsonl
    rocprofv3 --kernel-trace --stats -d prof -o gcl -- python tools/graphcl_bench.py --forms nodedrop --steps 10 --warmup 3
    python tools/graphcl_bench.py --kernel-stats prof/gcl_results.db --trace-steps 13
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module('3dinfomax_amd')
dataset = importlib.import_module('3dinfomax_amd.dataset')

PNA_ARGS = dict(target_dim=256, hidden_dim=200, mid_batch_norm=True, last_batch_norm=True, readout_batchnorm=True,
                batch_norm_momentum=0.93, readout_hidden_dim=200, readout_layers=2, dropout=0.0, propagation_depth=7,
                aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'],
                readout_aggregators=['min', 'max', 'mean'], pretrans_layers=2, posttrans_layers=1, residual=True)
DROP_RATIO = 0.2


def run(form, B, steps, warmup, dev, n_batches=4):
    mols = amd.synth.make_dataset(B * n_batches, seed=21, kind='qmugs')
    ds = dataset.FlatMolDataset(mols)
    order = np.random.default_rng(0).permutation(len(ds))
    batches = [order[k * B:(k + 1) * B] for k in range(n_batches)]
    rng = np.random.default_rng(1)
    torch.manual_seed(0)
    model = amd.PNA(avg_d=1.0, device=str(dev), **PNA_ARGS).to(dev).train()
    opt = amd.Adam(model.parameters(), lr=8e-5)
    loss_fn = amd.NTXent(tau=0.1)
    sizes = []

    def views(ids):
        if form == 'nodedrop':
            (g1,), (g2,) = dataset.nodedrop_to_device(ds.assemble_nodedrop_host(ids, DROP_RATIO, rng=rng), dev)
            return g1, g2
        return ds.assemble_2d(ids, dev)[0], ds.assemble_2d(ids, dev)[0]

    def step(i):
        g1, g2 = views(batches[i % n_batches])
        if len(sizes) < n_batches:
            sizes.append((g1.number_of_nodes(), g1.number_of_edges(), g2.number_of_nodes(), g2.number_of_edges()))
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(g1), model(g2))
        loss.backward()
        opt.step()
        return loss

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize(dev)
    host = 0.0
    t0 = time.perf_counter()
    for i in range(steps):
        h0 = time.perf_counter()
        loss = step(warmup + i)
        host += time.perf_counter() - h0
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3 / steps
    s = np.array(sizes, dtype=np.float64).mean(0)
    return dict(form=form, batch=B, steps=steps, warmup=warmup, ms_per_step=round(ms, 4), molecules_per_s=round(B / ms * 1e3, 1),
                host_enqueue_ms_per_step=round(host * 1e3 / steps, 4), view_nodes=[round(s[0], 1), round(s[2], 1)],
                view_edges=[round(s[1], 1), round(s[3], 1)], last_loss=float(loss.item()), device=torch.cuda.get_device_name(dev))


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
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--forms', nargs='+', default=['nodedrop', 'undropped'], choices=['nodedrop', 'undropped'])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--tag', default=None, help='added to every JSON line (e.g. which checkout ran it)')
    ap.add_argument('--out', default=None, help='JSON lines are appended to this file')
    a = ap.parse_args()
    if a.kernel_stats:
        print(kernel_stats(a.kernel_stats, a.trace_steps))
        return
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    for form in a.forms:
        r = run(form, a.batch, a.steps, a.warmup, dev)
        if a.tag:
            r['tag'] = a.tag
        print(json.dumps(r), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
