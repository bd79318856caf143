"""Times of the local-global pre-training mode (NTXentLocalGlobal, PNALocal; configs/old_configs/contrastive_local.yml) on one MI355X.

Data: 500 QM9-shaped synthetic molecules (N ~ 9 k atoms).

  loss     forward + backward of the loss at zn [N, 256], zg [500, 256], tau 0.1: `kernels` (csrc/localglobal.hip, one C call per
           direction) against `eager`, a torch composition of the same math on the device, written here from the formulas: a segment
           index instead of the reference's Python loop over the molecules, the negatives summed with the positive's column zeroed.
           The two are alternated in blocks of --loss-iters inside one call, --rounds times, HIP events around each block (launch gaps
           and allocations included).  max_allocated_mib: the peak of torch's allocator over one forward + backward above what was
           resident before it.
  step     one training step of PNALocal (hidden 90, depth 6, target 256) + EGNN (hidden 128, depth 7) + the loss + Adam over both
           models, wall time around windows that end in a device synchronise.

Prints one JSON line per measurement and writes them to --out.

    python tools/local_global_bench.py --out profiles/local_global_bench.txt
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

PNA_LOCAL = dict(node_dim=None, edge_dim=None, target_dim=256, hidden_dim=90, mid_batch_norm=True, last_batch_norm=True,
                 readout_batchnorm=True, readout_hidden_dim=90, dropout=0.0, propagation_depth=6,
                 aggregators=['mean', 'max', 'min', 'std'], scalers=['identity', 'amplification', 'attenuation'],
                 readout_aggregators=['min', 'max', 'mean'], pretrans_layers=2, posttrans_layers=1, residual=True)
EGNN = dict(node_dim=1, edge_dim=1, target_dim=256, hidden_dim=128, propagation_depth=7, dropout=0.0, readout_batchnorm=True,
            readout_hidden_dim=128, readout_layers=2, readout_aggregators=['min', 'max', 'mean'], batch_norm=True)


def eager_loss(zn, zg, seg, tau, eps=1e-10):
    """mean_i -log(e_{i,g(i)} / sum_{j != g(i)} e_ij), e = exp(zn_i . zg_j / ((|zn_i| |zg_j| + eps) tau)); seg [N, 1] = g"""
    sim = zn @ zg.T
    sim = sim / (zn.norm(dim=1)[:, None] * zg.norm(dim=1)[None, :] + eps)
    e = torch.exp(sim / tau)
    pos = e.gather(1, seg).squeeze(1)
    neg = e.scatter(1, seg, 0.0).sum(dim=1)
    return -torch.log(pos / neg).mean()


def loss_times(mols, dim, tau, iters, warmup, rounds, dev):
    npg = torch.tensor([m.n_atoms for m in mols])
    N, B = int(npg.sum()), len(mols)
    gen = torch.Generator().manual_seed(0)
    zn = torch.relu(torch.randn(N, dim, generator=gen)).to(dev).requires_grad_(True)       # PNALocal ends in a ReLU
    zg = torch.randn(B, dim, generator=gen).to(dev).requires_grad_(True)
    npg_dev = npg.to(dev)
    seg = torch.repeat_interleave(torch.arange(B, device=dev), npg_dev)[:, None]
    fn = amd.NTXentLocalGlobal(tau=tau)

    def kernels():
        zn.grad = zg.grad = None
        loss = fn(zn, zg, npg_dev)
        loss.backward()
        return loss

    def eager():
        zn.grad = zg.grad = None
        loss = eager_loss(zn, zg, seg, tau)
        loss.backward()
        return loss

    forms = (('kernels', kernels), ('eager', eager))
    values, peak = {}, {}
    for form, f in forms:
        for _ in range(warmup):
            values[form] = f()
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        f()
        torch.cuda.synchronize(dev)
        peak[form] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    times = {form: [] for form, _ in forms}
    for _ in range(rounds):
        for form, f in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize(dev)
            times[form].append(a.elapsed_time(b) * 1e3 / iters)
    return [dict(what='loss_fwd_bwd', form=form, nodes=N, graphs=B, dim=dim, tau=tau, iters=iters, rounds=rounds,
                 us_per_call_median=round(float(np.median(ts)), 1), us_per_call_min=round(min(ts), 1), us_per_call_max=round(max(ts), 1),
                 max_allocated_mib=round(peak[form], 1), loss=float(values[form].item()), device=torch.cuda.get_device_name(dev))
            for form, ts in times.items()]


def step_times(mols, tau, n_steps, warmup, rounds, dev):
    B = len(mols)
    n_atoms = np.array([m.n_atoms for m in mols], dtype=np.int64)
    graph_ptr = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(n_atoms, out=graph_ptr[1:])
    xyz = torch.from_numpy(np.concatenate([m.coords for m in mols]).astype(np.float32)).to(dev)
    g3 = dataset.complete_graphs_on_device(xyz, torch.from_numpy(graph_ptr).to(dev), n_atoms, torch.from_numpy(n_atoms))
    g3.ndata['x'] = xyz
    g3.ndata['feat'] = torch.ones(xyz.shape[0], 1, device=dev)
    g2 = amd.batch([amd.bond_graph(m) for m in mols]).to(dev)
    torch.manual_seed(0)
    model2d, model3d = amd.PNALocal(**PNA_LOCAL).to(dev).train(), amd.EGNN(**EGNN).to(dev).train()
    fn = amd.NTXentLocalGlobal(tau=tau)
    opt = amd.Adam(list(model2d.parameters()) + list(model3d.parameters()), lr=8e-5)
    npg = g2.batch_num_nodes()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = fn(model2d(g2.local_copy()), model3d(g3.local_copy()), npg)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        first = step()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n_steps):
            loss = step()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3 / n_steps)
    return [dict(what='step', models='PNALocal + EGNN + NTXentLocalGlobal + Adam', batch=B, atoms=int(g2.number_of_nodes()),
                 edges_2d=int(g2.number_of_edges()), edges_3d=int(g3.number_of_edges()), steps=n_steps, rounds=rounds,
                 ms_per_step_median=round(float(np.median(ts)), 3), ms_per_step_min=round(min(ts), 3), ms_per_step_max=round(max(ts), 3),
                 first_loss=float(first.item()), last_loss=float(loss.item()), device=torch.cuda.get_device_name(dev))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--tau', type=float, default=0.1)
    ap.add_argument('--loss-iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X (cuda:0): a time taken without the GPU says nothing')
    dev = torch.device('cuda:0')
    mols = amd.synth.make_dataset(a.batch, seed=a.batch)
    lines = []
    for r in loss_times(mols, a.dim, a.tau, a.loss_iters, a.warmup, a.rounds, dev) + \
            step_times(mols, a.tau, a.steps, a.warmup, a.rounds, dev):
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
