"""Training-step time of the EGNN 3D encoder at the sizes of configs/0.yml (hidden 128, depth 7, batch_norm, readout min / max / mean,
readout_hidden_dim 90, target_dim 256; mean-of-squares loss, Adam) on one MI355X, with the fused gate-and-reduce step of
csrc/egnn.hip on and off, and that step's kernels on their own.

Data: QM9-shaped synthetic molecules, complete graphs built on the device (dataset.complete_graphs_on_device) with the coordinates in
ndata['x'] and constant-ones features (the input of configs/0.yml).

  step     forward + backward + Adam step, `fused` and `composed` (EGCLayer.fused_gate_reduce) alternated in blocks of --steps inside
           one call, --rounds times; the same model object, batch and optimiser state layout
  kernel   at H = 128 on the same batch: i3d_gate_reduce_fwd / i3d_gate_reduce_bwd (+ the two column sums) against the composed
           three-launch forward (soft_edge, segment_sum, add) and five-launch backward (segment_bcast, soft_edge_bwd, two column
           sums; `dL/dh = dL/du` costs nothing in either form), HIP events around --kernel-iters back-to-back calls after a warm-up.
           gbytes_per_s is over the bytes the ALGORITHM has to move (m once and h, u, w for the forward; m, gm once and gu, w for the
           backward), the same figure for both forms, so the two rates compare directly.

Prints one JSON line per measurement and writes them to --out.

    python tools/egnn_bench.py --batches 100 500 --steps 30 --warmup 10 --out profiles/egnn_bench.txt
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
ops = importlib.import_module('3dinfomax_amd.ops')
egnn = importlib.import_module('3dinfomax_amd.egnn')
dataset = importlib.import_module('3dinfomax_amd.dataset')

MODEL = dict(node_dim=1, edge_dim=1, hidden_dim=128, target_dim=256, propagation_depth=7, batch_norm=True, readout_batchnorm=True,
             batch_norm_momentum=0.1, reduce_func='sum', dropout=0.0, readout_layers=2, readout_hidden_dim=90,
             readout_aggregators=['min', 'max', 'mean'])


def make_batch(B, dev):
    mols = amd.synth.make_dataset(B, seed=B)
    n_atoms = np.array([m.n_atoms for m in mols], dtype=np.int64)
    graph_ptr = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(n_atoms, out=graph_ptr[1:])
    xyz = torch.from_numpy(np.concatenate([m.coords for m in mols]).astype(np.float32)).to(dev)
    g = dataset.complete_graphs_on_device(xyz, torch.from_numpy(graph_ptr).to(dev), n_atoms, torch.from_numpy(n_atoms))
    g.ndata['x'] = xyz
    g.ndata['feat'] = torch.ones(xyz.shape[0], 1, device=dev)
    return g


def steps(B, n_steps, warmup, rounds, dev):
    g = make_batch(B, dev)
    torch.manual_seed(0)
    model = amd.EGNN(**MODEL).to(dev).train()
    opt = amd.Adam(model.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = (model(g.local_copy()) ** 2).mean()
        loss.backward()
        opt.step()
        return loss

    times = {'fused': [], 'composed': []}
    try:
        for r in range(rounds + 1):            # round 0 warms both forms up
            for form in ('fused', 'composed'):
                egnn.EGCLayer.fused_gate_reduce = form == 'fused'
                for _ in range(warmup if r == 0 else 2):
                    step()
                if r == 0:
                    continue
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(n_steps):
                    loss = step()
                torch.cuda.synchronize(dev)
                times[form].append((time.perf_counter() - t0) * 1e3 / n_steps)
    finally:
        egnn.EGCLayer.fused_gate_reduce = True
    out = []
    for form, ts in times.items():
        out.append(dict(what='step', form=form, batch=B, atoms=int(g.number_of_nodes()), edges=int(g.number_of_edges()),
                        steps=n_steps, rounds=rounds, ms_per_step_median=round(float(np.median(ts)), 4),
                        ms_per_step_min=round(min(ts), 4), ms_per_step_max=round(max(ts), 4), last_loss=float(loss.item()),
                        device=torch.cuda.get_device_name(dev)))
    return out


def kernels(B, iters, warmup, dev, H=128, mean=False):
    g = make_batch(B, dev)
    idx = g.index()
    N, E = idx.num_nodes, idx.num_edges
    gen = torch.Generator().manual_seed(B)
    m, h, gu = (torch.randn(r, H, generator=gen).to(dev) for r in (E, N, N))
    ws, bs = (torch.randn(1, H, generator=gen) / H ** 0.5).to(dev), torch.zeros(1, device=dev)
    _, w = ops.gate_reduce_fwd(m, ws, bs, idx.in_ptr, h, mean)

    def fused_fwd():
        return ops.gate_reduce_fwd(m, ws, bs, idx.in_ptr, h, mean)

    def composed_fwd():
        msg, _ = ops.soft_edge_fwd(m, ws, bs)
        return ops.add(ops.segment_sum(msg, idx.in_ptr, None, N, mean=mean), h)

    def fused_bwd():
        return ops.gate_reduce_bwd(gu, m, w, ws, idx.in_ptr, mean)

    def composed_bwd():
        gmsg = ops.segment_bcast(gu, idx.in_ptr, idx.dst_s, E, mean=mean)
        gm, gg = ops.soft_edge_bwd(gmsg, m, w, ws)
        return gm, ops.colsum(m, w=gg), ops.colsum(gg.view(-1, 1))

    need = {'fwd': 4 * (E * H + 2 * N * H + E + N), 'bwd': 4 * (2 * E * H + N * H + E + N)}
    out = []
    for direction, forms in (('fwd', (('fused', fused_fwd), ('composed', composed_fwd))),
                             ('bwd', (('fused', fused_bwd), ('composed', composed_bwd)))):
        for form, fn in forms:
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            us = a.elapsed_time(b) * 1e3 / iters
            out.append(dict(what='gate_reduce_' + direction, form=form, batch=B, atoms=N, edges=E, feat=H, iters=iters,
                            us_per_call=round(us, 2), algorithm_bytes=need[direction],
                            gbytes_per_s=round(need[direction] / us / 1e3, 1),
                            note='back-to-back calls between two HIP events: includes the launch gaps and the output allocations',
                            device=torch.cuda.get_device_name(dev)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[100, 500])
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = []
    for B in a.batches:
        for r in steps(B, a.steps, a.warmup, a.rounds, dev) + kernels(B, a.kernel_iters, a.warmup, dev):
            lines.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
