"""Cost of BYOL's teacher update and of one whole BYOL step on one MI355X, on the models of the reference's configs/byol.yml (PNA hidden 90,
depth 6; Net3D hidden 20, depth 1; predictors 256 -> 256) at its batch of 250 molecules.

Teacher update of BOTH wrappers, three ways on the same device tensors, in blocks of --iters calls that alternate inside one process,
--rounds times:
    launch    BYOLwrapper.ma_teacher_update(): one launch of csrc/ema.hip per wrapper over a table built once, in place
    foreach   torch._foreach_mul_(teacher, d); torch._foreach_add_(teacher, student, alpha=1 - d): in place, torch's multi-tensor kernels
    loop      the reference's line per parameter, `t.data = t.data * d + s.data * (1 - d)` (trainer/byol_wrapper.py:38-40): three
              launches and a new storage per tensor
Per block two times per call: `host_us`, the host clock around the enqueueing loop alone (what the update adds to the step's host side),
and `device_us`, HIP events around the block (back-to-back calls: launch gaps and allocations included).

One whole BYOL step (reference trainer/byol_trainer.py:10-22 around trainer/trainer.py:116-124): both wrappers' forward, both loss
directions of CosineSimilarityLoss, backward, Adam, both teacher updates - with each of the three updates, alternated the same way, host
clock around --steps steps ending in a device synchronise.  (The reference's trainer calls the update of `model` only; both are timed
here because both teachers have to follow their students.)

Prints one JSON line per row and writes them to --out.

    python tools/byol_bench.py --out profiles/byol_bench.txt
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

PNA_BYOL = dict(target_dim=256, hidden_dim=90, mid_batch_norm=True, last_batch_norm=True, readout_batchnorm=True, batch_norm_momentum=0.96,
                readout_hidden_dim=90, readout_layers=0, dropout=0.0, propagation_depth=6, aggregators=['mean', 'max', 'min', 'std'],
                scalers=['identity', 'amplification', 'attenuation'], readout_aggregators=['min', 'max', 'mean'], pretrans_layers=2,
                posttrans_layers=1, residual=True)
NET3D_BYOL = dict(target_dim=256, hidden_dim=20, hidden_edge_dim=20, node_wise_output_layers=0, message_net_layers=1, update_net_layers=1,
                  reduce_func='mean', fourier_encodings=4, propagation_depth=1, dropout=0.0, batch_norm=True, readout_batchnorm=True,
                  batch_norm_momentum=0.96, readout_hidden_dim=20, readout_layers=1, readout_aggregators=['min', 'max', 'mean'])
WRAPPER = dict(predictor_layers=1, predictor_hidden_size=256, predictor_batchnorm=True, metric_dim=256, ma_decay=0.995)


def update_launch(ws):
    for w in ws:
        w.ma_teacher_update()


def update_foreach(ws):
    for w in ws:
        d = w.ma_decay
        teacher = [p.data for p in w.teacher.parameters()]
        torch._foreach_mul_(teacher, d)
        torch._foreach_add_(teacher, [p.data for p in w.student.parameters()], alpha=1. - d)


def update_loop(ws):
    for w in ws:
        for params_s, params_t in zip(w.student.parameters(), w.teacher.parameters()):
            params_t.data = params_t.data * w.ma_decay + params_s.data * (1. - w.ma_decay)


UPDATES = (('launch', update_launch), ('foreach', update_foreach), ('loop', update_loop))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=250)
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    mols = amd.synth.make_dataset(a.batch, seed=1)
    g2 = amd.batch([amd.bond_graph(m) for m in mols]).to(dev)
    g3 = amd.batch([amd.complete_graph(m) for m in mols]).to(dev)
    w2 = amd.BYOLwrapper('PNA', PNA_BYOL, avg_d=1.0, device=dev, **WRAPPER).to(dev).train()
    w3 = amd.BYOLwrapper('Net3D', NET3D_BYOL, node_dim=0, edge_dim=1, avg_d=1.0, **WRAPPER).to(dev).train()
    ws = (w2, w3)
    loss_fn = amd.CosineSimilarityLoss()
    opt = amd.Adam([p for w in ws for p in w.parameters() if p.requires_grad], lr=1e-4)
    shape = dict(batch=a.batch, atoms=g2.number_of_nodes(), bonds=g2.number_of_edges(), edges3d=g3.number_of_edges(),
                 pairs=sum(len(list(w.teacher.parameters())) for w in ws), elements=sum(p.numel() for w in ws for p in w.teacher.parameters()),
                 device=torch.cuda.get_device_name(dev))

    def step(update):
        pred2, proj2 = w2(g2.local_copy())
        pred3, proj3 = w3(g3.local_copy())
        loss = loss_fn(pred2, proj3) + loss_fn(proj2, pred3)
        loss.backward()
        opt.step()
        opt.zero_grad()
        update(ws)
        return loss

    for _, update in UPDATES:                      # every path once before anything is timed, the step's first calls included
        for _ in range(a.warmup):
            loss = step(update)
    torch.cuda.synchronize(dev)

    lines = []
    times = {name: ([], []) for name, _ in UPDATES}
    for _ in range(a.rounds):
        for name, update in UPDATES:
            for _ in range(3):                     # (after `loop` every teacher tensor is in a new storage: the table is rebuilt here)
                update(ws)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                update(ws)
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize(dev)
            times[name][0].append((t1 - t0) * 1e6 / a.iters)
            times[name][1].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    for name, _ in UPDATES:
        host, device = times[name]
        row = dict(what='teacher_update_both_wrappers', form=name, iters=a.iters, rounds=a.rounds,
                   host_us_median=round(float(np.median(host)), 1), host_us_min=round(min(host), 1), host_us_max=round(max(host), 1),
                   device_us_median=round(float(np.median(device)), 1), device_us_min=round(min(device), 1),
                   device_us_max=round(max(device), 1), **shape)
        lines.append(row)
        print(json.dumps(row), flush=True)

    times = {name: [] for name, _ in UPDATES}
    last = {}
    for _ in range(a.rounds):
        for name, update in UPDATES:
            for _ in range(3):
                loss = step(update)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step(update)
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
            last[name] = float(loss.item())
    for name, _ in UPDATES:
        ts = times[name]
        row = dict(what='byol_step', update=name, steps=a.steps, rounds=a.rounds, ms_per_step_median=round(float(np.median(ts)), 4),
                   ms_per_step_min=round(min(ts), 4), ms_per_step_max=round(max(ts), 4), last_loss=last[name], **shape)
        lines.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
