"""The noised-3D negatives (reference configs/old_configs/contrastive_training_noised_3d.yml: PNA hidden 128 depth 6, Net3D hidden 10
depth 1 with 4 Fourier encodings, target 256, NTXentExtraNegatives tau 0.1 weight 50, NoisedDistancesCollate std 0.2 with 10 noised
copies, Adam lr 8e-5, batch 500) on one MI355X, on drug-sized synthetic molecules (synth.qmugs_like: a stand-in for GEOM-Drugs).

  builder    the device builder alone (dataset.noised_complete_graphs_on_device, csrc/noised3d.hip: one launch for the (1 + U)-fold
             batch), device events around `--builder-reps` back-to-back launches on a resident batch, beside the clean batch's
             builder (complete_graphs_on_device); bytes written per launch and the rate they amount to
  step       one training step = batch hand-over, PNA(g2d), Net3D(g3d of (1 + U) B molecules), NTXentExtraNegatives, backward, Adam,
             fed by  device: BatchStream(noised_3d=...) (host half assembled in the training thread, one upload, 3D batch with its
                             copies built on the device)
                     host:   NoisedDistancesCollate(std, U) on per-molecule graphs made once beforehand (the reference's datasets
                             cache them), then .to(device) - which builds the kernel index of both batches on the host - the way a
                             run on the reference's own data path is fed
             alternated in one call: every round times `--steps` device-fed steps and then `--host-steps` host-fed steps, each
             window ending in a device synchronise (host clock).  Same models, same optimizer state carried through.

    python tools/noised3d_bench.py --out profiles/noised3d_bench.txt
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

PNA_ARGS = dict(target_dim=256, hidden_dim=128, mid_batch_norm=True, last_batch_norm=True, readout_batchnorm=True,
                batch_norm_momentum=0.96, readout_hidden_dim=128, readout_layers=2, dropout=0.0, propagation_depth=6,
                aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'],
                readout_aggregators=['min', 'max', 'mean'], pretrans_layers=2, posttrans_layers=1, residual=True)
NET3D_ARGS = dict(target_dim=256, hidden_dim=10, hidden_edge_dim=10, node_wise_output_layers=1, message_net_layers=1,
                  update_net_layers=1, reduce_func='mean', fourier_encodings=4, propagation_depth=1, dropout=0.0, batch_norm=True,
                  readout_batchnorm=True, batch_norm_momentum=0.96, readout_hidden_dim=10, readout_layers=1,
                  readout_aggregators=['min', 'max', 'mean'])


def builder_times(ds, ids, dev, std, U, reps):
    g2, xyz, graph_ptr, n, bnn = ds.assemble_2d(ids, dev)
    N, E3 = int(xyz.shape[0]), int((n * (n - 1)).sum())
    out = dict(what='builder', batch=len(ids), num_noised=U, nodes=N, edges3d=E3, total_edges=(1 + U) * E3, reps=reps)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3 / reps
    out['clean_us'] = round(timed(lambda: dataset.complete_graphs_on_device(xyz, graph_ptr, n, bnn, g2._edge_ptr3)), 2)
    for mode in ('distances', 'coordinates'):
        us = timed(lambda: dataset.noised_complete_graphs_on_device(xyz, graph_ptr, n, bnn, std, U, mode, 0, 1, g2._edge_ptr3))
        T = 1 + U
        nbytes = T * E3 * (5 * 4 + 2 * 8 + 4) + (T * N + 1) * 4 + (T * len(ids) + 1) * 4 + (T * N * 12 if mode == 'coordinates' else 0)
        out[f'{mode}_us'] = round(us, 2)
        out[f'{mode}_bytes_written'] = nbytes
        out[f'{mode}_GB_per_s'] = round(nbytes / us / 1e3, 1)
    return out


def step_times(mols, B, dev, std, U, rounds, steps, host_steps, warmup):
    ds = dataset.FlatMolDataset(mols)
    n_batches = len(mols) // B
    stream = dataset.BatchStream(ds, B, steps=1 << 30, seed=0, noised_3d={'std': std, 'num_noised': U, 'mode': 'distances'})
    torch.manual_seed(0)
    pna = amd.PNA(avg_d=1.0, device=str(dev), **PNA_ARGS).to(dev).train()
    net = amd.Net3D(node_dim=0, edge_dim=1, avg_d=1.0, **NET3D_ARGS).to(dev).train()
    opt = amd.Adam(list(pna.parameters()) + list(net.parameters()), lr=8e-5)
    loss_fn = amd.NTXentExtraNegatives(tau=0.1, extra_negatives_weight=50)
    items = [(amd.bond_graph(m), amd.complete_graph(m)) for m in mols]          # made once, as a dataset would cache them
    collate = amd.NoisedDistancesCollate(std, U)
    order = np.random.default_rng(0).permutation(len(mols))

    def feed(form, i):
        if form == 'device':
            return dataset.BatchStream.to_device(stream[i], dev)
        ids = order[(i % n_batches) * B:(i % n_batches + 1) * B]
        (g2,), (g3,) = collate([items[j] for j in ids])
        return [g2.to(dev)], [g3.to(dev)]

    def step(form, i):
        (g2,), (g3,) = feed(form, i)
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(pna(g2), net(g3))
        loss.backward()
        opt.step()
        return loss

    def window(form, first, count):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(count):
            loss = step(form, first + i)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / count, float(loss.item())
    window('device', 0, warmup)
    window('host', 0, 1)
    res = {'device': [], 'host': []}
    k = warmup
    for _ in range(rounds):
        for form, count in (('device', steps), ('host', host_steps)):
            ms, loss = window(form, k, count)
            res[form].append(round(ms, 3))
            k += count
    return dict(what='step', batch=B, num_noised=U, std=std, rounds=rounds, device_steps_per_window=steps,
                host_steps_per_window=host_steps, device_fed_ms_per_step=res['device'], host_fed_ms_per_step=res['host'],
                device_fed_median_ms=float(np.median(res['device'])), host_fed_median_ms=float(np.median(res['host'])),
                last_loss=loss, device=torch.cuda.get_device_name(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--num-noised', type=int, default=10)
    ap.add_argument('--std', type=float, default=0.2)
    ap.add_argument('--builder-reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='device-fed steps per window')
    ap.add_argument('--host-steps', type=int, default=1, help='host-fed steps per window')
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batches', type=int, default=3, help='distinct batches of molecules')
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None, help='the JSON lines are appended to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    mols = amd.synth.make_dataset(a.batch * a.batches, seed=21, kind='qmugs')
    results = [builder_times(dataset.FlatMolDataset(mols), np.arange(a.batch), dev, a.std, a.num_noised, a.builder_reps)]
    print(json.dumps(results[-1]), flush=True)
    if not a.skip_step:
        results.append(step_times(mols, a.batch, dev, a.std, a.num_noised, a.rounds, a.steps, a.host_steps, a.warmup))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            for r in results:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
